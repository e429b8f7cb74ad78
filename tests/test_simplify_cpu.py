"""Mesh decimation, CPU side: the numpy statement of the contract (tests/simplify_ref.py) on inputs whose answers are
known, so that the yardstick of tests/test_simplify_gpu.py is itself pinned, and the argument checks of shapeformer_amd/simplify.py,
which refuse before anything touches a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_ref as S   # noqa: E402


@pytest.fixture(scope="module")
def mc_meshes():
    """oracle marching cubes at Q = 33 of the three analytic fields (computed once)"""
    from oracle import mc_oracle as MO
    return {n: MO.marching_cubes(F, 0.5) for n, F in S.mc_fields(33).items()}


def _corner_distances(reg):
    v, f = S.cube_mesh(16)
    assert v.shape == (1734, 3) and f.shape == (3072, 3)
    ov, of, st = S.cluster(v, f, 5, reg=reg)
    assert st == 0 and ov.shape == (26, 3) and of.shape == (48, 3)        # the cube spans 3 cells of 0.4 per axis: 3^3 - 1 on its surface
    corners = np.array([[x, y, z] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)])
    cells = np.unique(S.cell_keys(v, 5))
    slot = np.searchsorted(cells, S.cell_keys(corners, 5))
    assert np.array_equal(cells[slot], S.cell_keys(corners, 5))
    return np.linalg.norm(ov[slot].astype(np.float64) - corners, axis=1)


def test_cube_corners_are_recovered_and_reg_acts():
    # three face planes meet in a corner's cell: the quadric's minimum is the corner; reg pulls it towards the cell's mean vertex by
    # about 3 reg |m - corner| ~ 1e-8 for reg = 1e-8 (measured: 0.0 after the f32 rounding), ~ 4.3e-4 for reg = 1e-3
    d = _corner_distances(1e-8)
    assert d.max() < 1e-6, d
    d = _corner_distances(1e-3)
    assert d.min() > 1e-5 and d.max() < 1e-3, d


def test_cell_expression_and_degenerate_cells():
    # lattice vertices exactly on cell boundaries go to the upper cell, the box's upper face to the last cell
    v = np.array([[-1, -0.5, 0], [0.25, 0.5, 1], [1, 1, 1], [-3, 0, 7]], np.float32)
    assert S.cell_coords(v, 8).tolist() == [[0, 2, 4], [5, 6, 7], [7, 7, 7], [0, 4, 7]]
    assert S.cell_keys(v, 1).tolist() == [0, 0, 0, 0]
    # a cell whose faces are all of the form (a, a, b) has no quadric: its vertex is the mean of its vertices; an unused vertex keeps
    # a cell of its own
    v = np.array([[-.9, -.9, -.9], [-.8, -.7, -.9], [.5, .5, .5], [.1, -.3, .7]], np.float32)
    f = np.array([[0, 0, 2], [1, 1, 2]], np.int32)
    ov, of, st = S.cluster(v, f, 2)
    assert st == 0 and len(of) == 0 and ov.shape == (3, 3)
    assert np.allclose(ov[0], v[:2].astype(np.float64).mean(0), atol=1e-7) and np.allclose(ov[2], v[2], atol=1e-7)
    assert np.allclose(ov[1], v[3], atol=1e-7)                                # cell (1,0,1) < cell (1,1,1)
    # status codes; a flagged shape is empty
    assert S.cluster(v[:0], f[:0], 4)[2] == 1 and S.cluster(v, np.array([[0, 1, 4]]), 4)[2] == 2
    bad = v.copy()
    bad[1, 2] = np.nan
    out = S.cluster(bad, f, 4)
    assert out[2] == 3 and len(out[0]) == 0 and len(out[1]) == 0 and S.count(bad, f, 4) == (0, 0)


def test_face_budget_bisection(mc_meshes):
    (sv, sf), (tv, tf), (wv, wf) = mc_meshes["sphere"], mc_meshes["torus"], mc_meshes["two"]
    assert len(sf) == 3512 and len(tf) == 3520 and 2048 >= len(wf) > 512
    assert S.count(sv, sf, 4)[0] == 60 and S.count(sv, sf, 5)[0] == 48          # count is not monotone in G
    want = {"sphere": (5, 15, 31), "torus": (4, 13, 29)}
    for name in ("sphere", "torus", "two"):
        v, f = mc_meshes[name]
        for k, target in enumerate((64, 512, 2048)):
            G = S.bisect(v, f, target)
            if len(f) <= target:
                assert G == 0
                ov, of, st, G = S.decimate(v, f, target)
                assert G == 0 and st == 0 and np.array_equal(ov, v) and np.array_equal(of, f)       # returned unchanged
                continue
            assert 1 <= G < 512
            assert S.count(v, f, G)[0] <= target < S.count(v, f, G + 1)[0], (name, target, G)
            if name in want:
                assert G == want[name][k], (name, target, G)
            ov, of, st, G2 = S.decimate(v, f, target)
            assert G2 == G and st == 0 and len(of) == S.count(v, f, G)[0] and len(ov) == S.count(v, f, G)[1]
            assert of.min() >= 0 and of.max() < len(ov)
    assert S.bisect(wv, wf, 2048) == 0


def test_clustered_sphere_stays_on_the_sphere(mc_meshes):
    # the quadric places a cell's vertex on the planes of its faces.  A patch of the r = 0.6 sphere inside one cell (diagonal
    # c = sqrt(3) / 8) departs from its planes by at most the sagitta c^2 / (8 r) = 0.0098; the bound is twice that
    v, f = mc_meshes["sphere"]
    ov, of, st = S.cluster(v, f, 16)
    r = np.linalg.norm(ov.astype(np.float64), axis=1)
    assert st == 0 and np.abs(r - 0.6).max() < 0.02
    lo = -1 + (S.cell_coords(ov, 16) + 0.0) * (2 / 16)
    assert (ov >= lo - 1e-6).all() and (ov <= lo + 2 / 16 + 1e-6).all()          # clamped to its cell


def test_simplify_refuses_cpu_tensors_and_bad_grids():
    from shapeformer_amd import _lib as L, simplify as SD
    v, f = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)
    vo, to = [0, 3], [0, 1]
    for grid in (0, 513, -1, [4, 4], 2.5):
        with pytest.raises(L.SfmiError, match="grid"):
            SD.cluster_faces_dev(v, f, vo, to, grid)
        with pytest.raises(L.SfmiError, match="grid"):
            SD.cluster_simplify_dev(v, f, vo, to, grid)
    for call in (lambda: SD.cluster_faces_dev(v, f, vo, to, 8), lambda: SD.cluster_simplify_dev(v, f, vo, to, 8),
                 lambda: SD.decimate_dev(v, f, vo, to, 0)):
        with pytest.raises(L.SfmiError, match="no CPU fallback"):
            call()
    with pytest.raises(L.SfmiError, match="reg"):
        SD.cluster_simplify_dev(v, f, vo, to, 8, reg=0.0)
    with pytest.raises(L.SfmiError, match="bbox"):
        SD.decimate_dev(v, f, vo, to, 0, bbox=((0, 0, 0), (1, 0, 1)))


def test_launchers_refuse_before_any_launch():
    """SFMI_EINVAL for NULL pointers, a G outside [1, 512], a box without lo < hi and reg <= 0: none of these reaches a launch, so
    they can be asked without a device."""
    from shapeformer_amd import _lib as L
    lib, E = L.lib(), L.SFMI_EINVAL
    buf = np.zeros(64, np.int32)
    p = L.ptr(buf)
    g, lo, hi = np.array([8], np.int32), np.array([-1.0] * 3), np.array([1.0] * 3)
    assert lib.sfmi_simplify_words(L.ptr(g), 1) == 16 and lib.sfmi_simplify_words(L.ptr(np.array([512, 1], np.int32)), 2) == 2 ** 22 + 1
    for bad in (0, 513, -3):
        gb = np.array([bad], np.int32)
        assert lib.sfmi_simplify_words(L.ptr(gb), 1) == -1
        assert lib.sfmi_simplify_cells_f32(p, p, p, p, L.ptr(gb), p, p, 1, 3, 1, L.ptr(lo), L.ptr(hi), p, p, p, None) == E
        assert lib.sfmi_simplify_popc_i32(p, p, p, L.ptr(gb), 1, p, p, None) == E
        assert lib.sfmi_simplify_slots_i32(p, p, p, p, p, p, L.ptr(gb), 1, 3, p, None) == E
        assert lib.sfmi_simplify_solve_f32(p, p, p, p, L.ptr(gb), p, p, p, p, p, 1, 1, L.ptr(lo), L.ptr(hi), 1e-3, p, None) == E
    assert lib.sfmi_simplify_words(None, 1) == -1 and lib.sfmi_simplify_words(L.ptr(g), 0) == -1
    G = L.ptr(g)
    assert lib.sfmi_simplify_cells_f32(None, p, p, p, G, p, p, 1, 3, 1, L.ptr(lo), L.ptr(hi), p, p, p, None) == E
    assert lib.sfmi_simplify_cells_f32(p, p, p, p, G, p, p, 1, 3, 1, L.ptr(lo), L.ptr(hi), p, None, p, None) == E
    assert lib.sfmi_simplify_cells_f32(p, p, p, p, G, p, p, 1, 3, 1, L.ptr(hi), L.ptr(lo), p, p, p, None) == E      # lo > hi
    assert lib.sfmi_simplify_cells_f32(p, p, p, p, G, p, p, 1, 3, 1, None, L.ptr(hi), p, p, p, None) == E
    assert lib.sfmi_simplify_popc_i32(p, None, p, G, 1, p, p, None) == E
    assert lib.sfmi_simplify_slots_i32(p, p, p, p, None, p, G, 1, 3, p, None) == E
    assert lib.sfmi_simplify_faces_i32(p, p, p, None, p, 1, 1, p, p, p, None) == E
    assert lib.sfmi_simplify_faces_i32(p, p, p, p, p, 1, 1, p, p, None, None) == E
    assert lib.sfmi_simplify_solve_f32(p, p, p, p, G, p, p, p, p, p, 1, 1, L.ptr(lo), L.ptr(hi), 0.0, p, None) == E     # reg <= 0
    assert lib.sfmi_simplify_solve_f32(p, p, p, p, G, p, p, p, p, p, 1, 1, L.ptr(lo), L.ptr(hi), 1e-3, None, None) == E
    assert lib.sfmi_simplify_emit_i32(p, p, p, p, p, None, p, 1, 1, 1, p, None) == E
    assert lib.sfmi_simplify_emit_i32(p, p, p, p, p, p, p, 1, 1, 1, None, None) == E
    assert not buf.any()
