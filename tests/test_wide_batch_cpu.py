"""CPU: the layouts of tests/wide_batch.py hold what tests/test_wide_batch_gpu.py relies on, for both layouts and every tool's size
table; and the members chosen there keep each reference inside its own cap of excluded marginal items, by the reference alone."""
import numpy as np
import pytest

import knn_ref as KR
import wide_batch as W
from shapeformer_amd import _ragged

LAYOUTS = sorted(W.LAYOUTS)


def test_wide_pattern():
    lay = W.LAYOUTS["wide"]
    assert W.B == 261 and W.B > 256 and W.B & (W.B - 1) != 0 and len(lay.member) == W.B
    assert lay.empty == (0, 1, 2, 130, 131, 254, 260)
    assert lay.member[255:258].tolist() == [3, 4, 5]                      # three different non-empty sets astride lane 256
    full = np.nonzero(lay.member >= 0)[0]
    assert full[0] == 3 and full[-1] == 259
    assert all(lay.member[b] == b % 6 for b in full)
    assert sorted(set(lay.member[full].tolist())) == [0, 1, 2, 3, 4, 5]


def test_sparse_pattern():
    lay = W.LAYOUTS["sparse"]
    full = np.nonzero(lay.member >= 0)[0]
    assert full.tolist() == [5, 255, 256, 260] and lay.member[full].tolist() == [0, 1, 2, 3]
    assert W.SPARSE_POINT_SIZES == (1, 3, 2, 4) and lay.offsets(W.SPARSE_POINT_SIZES)[-1] == 10


def _columns(sizes):
    """a tool's member sizes as one tuple per kind of item: points -> [(n,...)], pairs / meshes / graphs -> [(a,...), (b,...)]"""
    return [tuple(sizes)] if np.ndim(sizes[0]) == 0 else [tuple(s[c] for s in sizes) for c in range(len(sizes[0]))]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tool", sorted(W.TOOLS))
def test_every_size_table(tool, layout):
    row, lay = W.TOOLS[tool], W.LAYOUTS[layout]
    sizes, sub = W.sizes_of(row, layout), W.substitute_of(row, layout)
    assert len(sizes) in ((6, 7) if layout == "wide" else (4, 5))         # the pattern's members (+ one that only fills empty slots)
    assert (row.substitute is None) == (row.rests_on is None)             # a substitution names the docstring line it rests on
    which = lay.members(sub)
    if sub is None:
        assert tuple(np.nonzero(which < 0)[0]) == lay.empty
    else:
        assert 0 <= sub < len(sizes) and (which >= 0).all() and (which[list(lay.empty)] == sub).all()
    for col in _columns(sizes):
        off = lay.offsets(col, sub)
        n = int(off[-1])
        assert np.array_equal(_ragged.host_offsets(off, n, tool), off) and off.dtype == np.int64 and len(off) == W.B + 1
        assert np.array_equal(np.diff(off), lay.sizes(col, sub))
        if layout == "sparse" and sub is None and tool != "marching_cubes":
            assert n < W.B                                                # the B-sized parts of grids and workspaces dominate
        if layout == "wide" and col == W.POINT_SIZES:
            assert 28000 < n < 30000
        # sfmi_owner: every item maps to its set, across the runs of empty sets
        want = np.repeat(np.arange(W.B), np.diff(off))
        got = W.owner(off, np.arange(n))
        assert np.array_equal(got, want)
        assert (np.diff(off)[got] > 0).all()                              # never an empty set
        for b in np.nonzero(np.diff(off) > 0)[0]:                         # the first and last item of every non-empty set
            assert W.owner(off, off[b]) == b and W.owner(off, off[b + 1] - 1) == b


def test_point_defaults():
    assert W.POINT_SIZES == (300, 1, 65, 257, 2, 64) and W.TARGET_SIZES == (257, 64, 700, 65, 3, 300)
    for name in ("knn_k8", "icp_point", "nn_dist"):
        assert W.TOOLS[name].wide == tuple(zip(W.POINT_SIZES, W.TARGET_SIZES))
    # the pair tools' documented refusal - an empty reference set with a non-empty query set - is met by no pair here
    for sizes in (W.TOOLS["knn_k8"].wide, W.TOOLS["knn_k8"].sparse):
        assert all(m > 0 for n, m in sizes if n > 0)


def test_mesh_members_are_closed():
    from oracle import mc_oracle as MO
    for v, f in W.mesh_members()[:5] + W.sparse_mesh_members()[:3]:
        assert f.min() == 0 and f.max() == len(v) - 1 and MO.edge_use(f)
        assert MO.signed_volume(v.astype(np.float64), f) > 0              # outward
    assert [len(f) for _, f in W.mesh_members()[1:4]] == [4, 8, 12]
    v, f = W.zero_area_triangle()
    assert np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0])) == 0


def test_fpfh_cap_holds_by_the_reference_alone():
    """global_reg_ref.spfh calls a point marginal when a pair feature lies at a bin edge; at most 1 % may be (test_global_reg_gpu.py)"""
    import global_reg_ref as GR
    for sizes in (W.TOOLS["fpfh"].wide, W.TOOLS["fpfh"].sparse):
        for x, n, _ in W.orient_members(sizes):
            assert GR.marginal_fraction(x, n, [0, len(x)], 16, None) <= 0.01


def test_graph_members_are_solved_by_the_reference_alone():
    import posegraph_ref as P
    assert W.GRAPH_SIZES[:6] == ((2, 1), (3, 3), (4, 6), (5, 10), (3, 3), (2, 1)) and W.GRAPH_SIZES[6] == (1, 0)
    for g in W.graph_members(W.GRAPH_NODES) + W.graph_members(W.SPARSE_GRAPH_NODES):
        ref = P.optimize(g["X0"], g["src"], g["tgt"], g["T"], g["Lam"], g["unc"])
        assert ref["status"] == 0 and max(P.graph_error(ref["X"], g["X_true"])) <= 1e-9


# ---- the references' own caps on these members (step 6 of the GPU file) ---------------------------------------------------------------

def _members():
    return [x for layout in LAYOUTS for x in W.point_members(W.TOOLS["estimate_normals"].wide if layout == "wide" else
                                                             W.TOOLS["estimate_normals"].sparse)]


def test_normals_cap_holds_by_the_reference_alone():
    """test_scan_gpu.py excludes points whose two smallest eigenvalues lie within 5 % of the largest of each other, at most 1 %"""
    for x in _members():
        if len(x) < 3:
            continue
        _, tab = KR.tree_knn(x, x, 16)
        vec, lam = KR.pca_normals(x, tab)
        gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
        assert (gap < 0.05).mean() <= 0.01, (len(x), float((gap < 0.05).mean()))


def test_outlier_bands_are_empty_by_the_reference_alone():
    """no point of a member lies within 1e-9 relative of the radius rule's threshold (radius 0.12, 4 neighbours)"""
    r2 = 0.12 ** 2
    for x in _members():
        t = KR.tree_knn(x.astype(np.float64), x.astype(np.float64), 5)[0][:, 4]
        assert not (np.abs(t - r2) <= 1e-9 * r2).any()


def test_orient_margin_by_the_reference_alone():
    """no vote of orient_ref hangs on the last bits of the set's centroid or of the viewpoint: |m . d| >= 1e-9 (test_orient_gpu.py)"""
    import orient_ref as OR
    for anchor in ("outward", "viewpoint"):
        for layout in LAYOUTS:
            row = W.TOOLS[f"orient_normals_{anchor}"]
            for i, (x, n, v) in enumerate(W.orient_members(row.wide if layout == "wide" else row.sparse)):
                _, tab = KR.tree_knn(x, x, 8)
                want = OR.orient(x, n, tab, anchor=anchor, viewpoint=v if anchor == "viewpoint" else None)
                assert want["margin"] >= 1e-9, (anchor, layout, i)


def test_hpr_cap_by_the_reference_alone():
    """the f64 restatement agrees with qhull on every member within test_hpr_gpu.py's cap, ceil(0.001 n) rows"""
    import math
    import hpr_ref as HR
    from shapeformer_amd import data as D
    CAMS = W.CAMS
    for layout in LAYOUTS:
        for i, x in enumerate(W.point_members(W.TOOLS["hidden_point_mask_f32"].wide if layout == "wide" else
                                              W.TOOLS["hidden_point_mask_f32"].sparse)):
            if len(x) < 4:
                continue
            got = x[HR.visible_mask(x, CAMS[i])]
            assert HR.rows_differing(got, D.hidden_point_removal(x, CAMS[i])) <= math.ceil(0.001 * len(HR.row_set(x)))
