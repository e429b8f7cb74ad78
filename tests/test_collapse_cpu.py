"""No GPU: the contract of the edge-collapse decimation (include/sfmi.h) as tests/collapse_ref.py states it, on the six
small meshes; the refusals of shapeformer_amd/collapse.py, which come before anything touches the device; and the C entry points' own
argument checks, which return before any launch.  Only what the contract fixes is asserted: the status, the budget rule, the kept
topology.  The round counts are printed, not asserted (the GPU tests compare them with the device's)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collapse_ref as R   # noqa: E402

from shapeformer_amd import _lib as L   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_keeps_the_contract(name):
    v, f, target, (ov, of, status, rounds) = R.case(name)
    print(f"{name}: {len(f)} -> {len(of)} faces (target {target}), status {status}, {rounds} rounds")
    assert status == R.CASES[name][2]
    if status == 0:
        assert target - 1 <= len(of) <= target                       # the budget rule never overshoots
    else:
        assert len(of) > target
    tin, tout = R.topology_ref(v, f), R.topology_ref(ov, of)
    assert tout[5] == tin[5]                                          # Euler characteristic
    assert tout[3:5] == tin[3:5]                                      # boundary and non-manifold edges
    assert tout[2] == len(of) and tout[0] == len(ov)                  # a closed or bounded surface leaves no vertex without a face
    assert R.duplicate_faces(of) == 0
    assert np.isfinite(ov).all() and of.min() >= 0 and of.max() < len(ov)


def test_expected_topology_of_the_inputs():
    assert R.topology_ref(*R.case("grid12")[:2])[3] == 44
    for name in ("ico2", "ico3", "torus24", "torus16", "tetra"):
        assert R.topology_ref(*R.case(name)[:2])[3:5] == (0, 0)
    assert [len(R.case(n)[1]) for n in R.CASES] == [320, 1280, 576, 256, 242, 4]
    assert R.topology_ref(*R.torus_grid(16, 8, open_ring=True))[3] == 16


def test_boundary_vertices_stay_where_they_are():
    """the frozen boundary: the grid's boundary vertices all survive with their bits, and the output's boundary is made of them alone"""
    v, f, _, (ov, of, _, _) = R.case("grid12")
    before = {v[i].tobytes() for i in R.boundary_vertices(f)}
    after = {ov[i].tobytes() for i in R.boundary_vertices(of)}
    assert len(before) == 44 and after == before


def test_tetrahedron_does_not_fold():
    """rule (b): collapsing any edge of a tetrahedron would leave two coincident faces, so nothing collapses"""
    v, f, _, (ov, of, status, rounds) = R.case("tetra")
    assert status == 4 and rounds == 0 and np.array_equal(ov, v) and np.array_equal(of, f)


def test_at_or_under_budget_is_returned_as_it_is():
    v, f = R.icosphere(1)
    for target in (len(f), len(f) + 7):
        ov, of, status, rounds = R.collapse_ref(v, f, target)
        assert status == 0 and rounds == 0 and ov.tobytes() == v.tobytes() and np.array_equal(of, f)
    junk = np.array([[0, 1, 99]], np.int32)                           # not inspected: an index outside the shape passes through
    assert np.array_equal(R.collapse_ref(v, junk, 1)[1], junk)


def test_statuses_of_refused_shapes_and_the_round_cap():
    v, f = R.icosphere(1)
    bad = f.copy()
    bad[3, 1] = len(v)
    nan = v.copy()
    nan[5, 2] = np.nan
    for vv, ff, want in ((v, bad, 2), (nan, f, 3), (nan, bad, 2)):
        ov, of, status, _ = R.collapse_ref(vv, ff, 20)
        assert status == want and len(ov) == 0 and len(of) == 0
    ov, of, status, rounds = R.collapse_ref(v, f, 20, max_rounds=2)
    assert status == 5 and rounds == 2 and 20 < len(of) < len(f)
    assert R.collapse_ref(v, f, 20, max_rounds=0)[2:] == (5, 0)


def test_planted_non_manifold_edge_is_frozen():
    """three faces on one edge: its two vertices keep their positions and the edge its three faces"""
    v, f = R.icosphere(2)
    a, b = int(f[0, 0]), int(f[0, 1])
    v2 = np.concatenate([v, (1.5 * (v[a] + v[b]))[None]]).astype(np.float32)
    f2 = np.concatenate([f, [[a, b, len(v)]]]).astype(np.int32)
    tin = R.topology_ref(v2, f2)
    assert tin[4] == 1 and tin[3] == 2
    ov, of, status, _ = R.collapse_ref(v2, f2, 101)
    tout = R.topology_ref(ov, of)
    assert tout[3:] == tin[3:] and status in (0, 4)
    assert {v2[a].tobytes(), v2[b].tobytes(), v2[-1].tobytes()} <= {p.tobytes() for p in ov}


@pytest.fixture
def no_library(monkeypatch):
    def fail():
        pytest.fail("the library was loaded before the arguments were checked")
    monkeypatch.setattr(L, "lib", fail)


def test_refusals_come_before_any_device_work(no_library):
    from shapeformer_amd import collapse as C
    from shapeformer_amd import mcubes
    v, f = (torch.from_numpy(a.copy()) for a in R.tetrahedron())
    ok = dict(verts=v, faces=f, voff=[0, 4], toff=[0, 4], target=2)
    for bad, word in ((dict(target=-1), "target"), (dict(target=2.5), "target"), (dict(reg=0.0), "reg"), (dict(reg=-1e-3), "reg"),
                      (dict(reg=float("nan")), "reg"), (dict(max_rounds=-1), "max_rounds"), (dict(rounds_per_sync=0), "rounds_per_sync"),
                      (dict(voff=[0, 3]), "voff"), (dict(toff=[1, 4]), "toff"), (dict(toff=[0, 2, 4]), "batch sizes"),
                      (dict(faces=f.float()), "integer"), (dict(verts=v[:, :2]), "verts")):
        with pytest.raises(L.SfmiError, match=word):
            C.collapse_dev(**dict(ok, **bad))
    with pytest.raises(L.SfmiError, match="no CPU fallback"):               # CPU tensors: the last check
        C.collapse_dev(**ok)
    with pytest.raises(L.SfmiError, match="no CPU fallback"):
        C.mesh_topology_dev(v, f, None, None)
    with pytest.raises(L.SfmiError, match="no CPU fallback"):
        C.decimate_collapse_dev(v, f, None, None, 2)
    with pytest.raises(L.SfmiError, match="precluster"):
        C.decimate_collapse_dev(v, f, None, None, 2, precluster=0)
    with pytest.raises(L.SfmiError, match="decimate_face"):
        C.decimate_collapse_dev(v, f, None, None, -4)
    with pytest.raises(L.SfmiError, match="decimate_method"):
        mcubes.array2mesh(np.zeros((4, 4, 4), np.float32), if_decimate=True, decimate_method="igl")
    from shapeformer_amd import callbacks
    with pytest.raises(L.SfmiError, match="decimate_method"):
        callbacks._decimate_choice("edge")
    assert C.MAX_ROUNDS == R.DEFAULT_MAX_ROUNDS


def test_entry_points_refuse_before_any_launch():
    """the C side: declared in sfmi.h, exported, and SFMI_EINVAL for a NULL pointer or sizes beyond 32-bit indices (no runtime call is made)"""
    from shapeformer_amd import build as B
    B.build(verbose=False)
    names = [n for n in L.PROTOTYPES if n.startswith("sfmi_collapse_")]
    assert len(names) == 11
    lib = L.lib()
    assert lib.sfmi_collapse_workspace_bytes(2, 10, 20) > 0
    assert lib.sfmi_collapse_workspace_bytes(0, 10, 20) == 0 and lib.sfmi_collapse_workspace_bytes(1, 2 ** 30, 2 ** 30) == 0
    assert lib.sfmi_collapse_workspace_bytes(1, 10, 2 ** 28) == 0            # 9 T must fit an int
    E = L.SFMI_EINVAL
    assert lib.sfmi_collapse_init_f32(None, None, None, None, 1, 4, 4, 2, 8, None, None) == E
    assert lib.sfmi_collapse_records_i32(1, 4, 4, None, None, None, None) == E
    assert lib.sfmi_collapse_runs_i32(None, 1, 4, 4, None, None, None) == E
    assert lib.sfmi_collapse_quadrics_f64(None, None, 1, 4, 4, None, None) == E
    assert lib.sfmi_collapse_eval_f64(None, None, None, None, None, 1, 4, 4, 1e-3, None, None, None, None) == E
    assert lib.sfmi_collapse_win_i32(None, None, None, None, None, 1, 4, 4, None, None, None, None) == E
    assert lib.sfmi_collapse_apply_f32(None, None, None, None, None, None, None, 1, 4, 4, 2, 8, None, None) == E
    assert lib.sfmi_collapse_report_i32(1, 4, 4, None, None, None, None, None, None) == E
    assert lib.sfmi_collapse_finish_f32(None, 1, 4, 4, None, None, None, None, None, None) == E
    assert lib.sfmi_collapse_topology_i32(None, None, None, 1, 4, 4, None, None, None, None) == E
    buf = np.zeros(1 << 16, np.uint8)                                         # a host buffer stands in: reg <= 0 returns before it is read
    assert lib.sfmi_collapse_eval_f64(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 1, 4, 4, 0.0,
                                      buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None) == E


def test_the_cholesky_solve_has_one_copy():
    """simplify.hip and collapse.hip take the 3x3 solve from csrc/sfmi_quadric.h; both compile their own arithmetic without contraction"""
    csrc = os.path.join(ROOT, "shapeformer_amd", "csrc")
    for name in ("simplify.hip", "collapse.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "sfmi_quadric.h"' in text and "sfmi_quadric_solve(" in text and not re.search(r"\bl21\b", text), name
        assert "#pragma clang fp contract(off)" in text
    text = open(os.path.join(csrc, "collapse.hip")).read()
    assert not re.search(r"atomic(Add|Min|Max|Exch|CAS)\s*\(\s*\(?\s*(float|double)", text) and "unsafeAtomicAdd" not in text
    assert "np.linalg.solve" not in open(os.path.join(ROOT, "tests", "collapse_ref.py")).read().split('"""', 2)[2]
