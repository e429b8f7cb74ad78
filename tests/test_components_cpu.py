"""CPU tests of the mesh connected-components contract: the numpy reference of tests/components_ref.py against
scipy.sparse.csgraph.connected_components, its selection and compaction rules, and the host-side argument checks of
shapeformer_amd/components.py, which raise before the library is loaded."""
import numpy as np
import pytest
import torch

import components_ref as R


def _scipy_labels(n_vert, faces):
    """connected components of the vertex graph by scipy -> per-vertex class, -1 for vertices no face names"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    i, j = np.concatenate([f[:, 0], f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2], f[:, 2]])
    g = coo_matrix((np.ones(len(i)), (i, j)), shape=(n_vert, n_vert))
    lab = connected_components(g, directed=False)[1]
    ref = np.zeros(n_vert, bool)
    ref[f.reshape(-1)] = True
    return np.where(ref, lab, -1)


def _fixtures():
    out = {k: (v, f) for k, (v, f, _) in R.small_meshes().items()}
    for numbering in ("ascending", "descending", "permuted"):
        out["strip_" + numbering] = R.strip(500, numbering)
    tv, tf = R.tetrahedra(100)[:2]
    out["tetrahedra"] = (tv, tf)
    v, f = R.small_meshes()["disjoint"][:2]
    out["unreferenced"] = (np.concatenate([v, v]), np.concatenate([f, np.array([[7, 7, 8]], np.int32)]))
    return out


@pytest.mark.parametrize("name", sorted(_fixtures()))
def test_reference_labels_against_scipy(name):
    v, f = _fixtures()[name]
    vl, fl, C = R.labels(len(v), f)
    sl = _scipy_labels(len(v), f)
    assert np.array_equal(vl < 0, sl < 0)
    # the same partition: the pairs (ours, scipy's) are a bijection
    pairs = np.unique(np.stack([vl[vl >= 0], sl[vl >= 0]], 1), axis=0)
    assert len(pairs) == C == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))
    # the numbering rule: ascending smallest vertex index
    smallest = np.array([np.flatnonzero(vl == c).min() for c in range(C)])
    assert (np.diff(smallest) > 0).all()
    assert np.array_equal(fl, vl[np.asarray(f)[:, 0]])


def test_small_meshes_component_counts():
    for name, (v, f, C) in R.small_meshes().items():
        assert R.labels(len(v), f)[2] == C, name


def test_degenerate_face_and_unreferenced_vertices():
    v = np.arange(18, dtype=np.float32).reshape(6, 3)
    f = np.array([[1, 1, 3]], np.int32)
    vl, fl, st, s = R.components(v, f)
    assert s == 0 and vl.tolist() == [-1, 0, -1, 0, -1, -1] and fl.tolist() == [0]
    assert st["n_vert"].tolist() == [2] and st["n_face"].tolist() == [1] and st["area"].tolist() == [0.0]
    kv, kf, _, kept = R.keep(v, f)
    assert kept.tolist() == [True] and np.array_equal(kv, v[[1, 3]]) and kf.tolist() == [[0, 0, 1]]


def _table(m):
    m = np.asarray(m, np.float64)
    return dict(area=m, n_face=m.astype(np.int32), volume=-m)


def test_selection_ties_rank_by_id():
    st = _table([2.0, 5.0, 5.0, 1.0, 5.0])
    assert R.select(st, top=1).tolist() == [False, True, False, False, False]
    assert R.select(st, top=2).tolist() == [False, True, True, False, False]
    assert R.select(st, top=4).tolist() == [True, True, True, False, True]
    assert R.select(st, min_share=1.0).tolist() == [False, True, True, False, True]
    assert R.select(st).all()


def test_selection_top_and_min_share_together():
    st = _table([10.0, 0.5, 4.0, 0.05, 3.0])
    assert R.select(st, top=3, min_share=0.35).tolist() == [True, False, True, False, False]
    assert R.select(st, top=1, min_share=0.01).tolist() == [True, False, False, False, False]
    assert R.select(st, min_share=0.01).tolist() == [True, True, True, False, True]
    for by in ("faces", "volume"):
        assert np.array_equal(R.select(st, top=3, min_share=0.35, by=by), R.select(st, top=3, min_share=0.35))


def test_volume_measure_is_its_magnitude():
    """two tetrahedra, the larger one with flipped orientation: its signed volume is negative and it still ranks first by volume"""
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    v = np.concatenate([0.5 * corner, 2.0 + corner])
    f = np.concatenate([tri, 4 + tri[:, ::-1]])
    vl, fl, st, s = R.components(v, f)
    assert np.allclose(st["volume"], [0.125 / 6, -1.0 / 6], rtol=1e-12)
    assert R.select(st, top=1, by="volume").tolist() == [False, True]
    kv, kf, _, _ = R.keep(v, f, top=1, by="volume")
    assert np.array_equal(kv, v[4:]) and np.array_equal(kf, tri[:, ::-1])


def test_compaction_against_mask_and_renumber():
    v, f, tet_of, _, _ = R.tetrahedra(50, seed=3)
    v = np.concatenate([v, np.ones((7, 3), np.float32)])                    # unreferenced vertices at the end
    vl, fl, st, _ = R.components(v, f)
    kept = np.arange(50) % 3 != 0
    kv, kf = R.compact(v, f, vl, fl, kept)
    vmask = (vl >= 0) & kept[np.maximum(vl, 0)]
    fmask = kept[fl]
    assert np.array_equal(kv, v[vmask])
    remap = -np.ones(len(v), np.int64)
    remap[vmask] = np.arange(vmask.sum())
    assert np.array_equal(kf, remap[f[fmask]]) and kf.min() >= 0
    # geometry is preserved face by face
    assert np.array_equal(kv[kf], v[f[fmask]])
    # keep-all of a mesh without unreferenced vertices is the identity
    v2, f2 = R.tetrahedra(20, seed=4)[:2]
    kv2, kf2, _, k2 = R.keep(v2, f2)
    assert k2.all() and np.array_equal(kv2, v2) and np.array_equal(kf2, f2)


def test_tetrahedra_fixture_volumes():
    v, f, tet_of, vol, formula = R.tetrahedra(100)
    vl, fl, st, _ = R.components(v, f)
    assert len(st["volume"]) == 100 and (st["n_vert"] == 4).all() and (st["n_face"] == 4).all()
    first = np.array([np.flatnonzero(vl == c).min() for c in range(100)])
    assert (np.abs(st["volume"] - vol[tet_of[first]]) <= 12 * 2.0 ** -52 * st["abs_volume"]).all() and (st["volume"] > 0).all()
    assert (np.abs(st["volume"] - formula[tet_of[first]]) <= 12 * 2.0 ** -52 * st["abs_volume"]).all()


def test_status_codes():
    v = np.zeros((3, 3), np.float32)
    assert R.status_of(v[:0], np.zeros((0, 3), np.int32)) == 1
    assert R.status_of(v, np.array([[0, 1, 3]])) == 2
    bad = v.copy()
    bad[1, 2] = np.nan
    assert R.status_of(bad, np.array([[0, 1, 2]])) == 3
    vl, fl, st, s = R.components(bad, np.array([[0, 1, 2]]))
    assert s == 3 and (vl == -1).all() and (fl == -1).all() and len(st["area"]) == 0


def test_sphere_field_fixture():
    f0, f = R.sphere_field()
    assert f.shape == (33, 33, 33) and (f >= f0).all() and (f > f0).any()


# ---- the host argument checks: every one raises SfmiError naming the argument, and none loads the library

@pytest.fixture()
def no_library(monkeypatch):
    from shapeformer_amd import _lib
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", refuse)


def _args():
    return torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), [0, 4], [0, 2]


@pytest.mark.parametrize("change,word", [
    (dict(verts=torch.zeros(4, 2)), "verts"), (dict(verts=torch.zeros(12)), "verts"), (dict(faces=torch.zeros(2, 4, dtype=torch.int32)), "faces"),
    (dict(voff=[0, 3]), "voff"), (dict(voff=[1, 4]), "voff"), (dict(toff=[0, 1]), "toff"), (dict(toff=[0, 3, 2]), "toff"),
    (dict(voff=[0, 2, 4]), "shapes"), (dict(), "device"),
])
def test_mesh_argument_checks(no_library, change, word):
    from shapeformer_amd import components as C
    from shapeformer_amd._lib import SfmiError
    a = dict(zip(("verts", "faces", "voff", "toff"), _args()))
    a.update(change)
    for fn in (C.mesh_components_dev, C.keep_components_dev):
        with pytest.raises(SfmiError, match=word):
            fn(a["verts"], a["faces"], a["voff"], a["toff"])


@pytest.mark.parametrize("kw,word", [
    (dict(top=0), "top"), (dict(top=-1), "top"), (dict(top=1.5), "top"), (dict(min_share=-0.1), "min_share"), (dict(min_share=1.5), "min_share"),
    (dict(min_share=float("nan")), "min_share"), (dict(min_share=float("inf")), "min_share"), (dict(by="edges"), "by"),
])
def test_selection_argument_checks(no_library, kw, word):
    from shapeformer_amd import components as C
    from shapeformer_amd._lib import SfmiError
    with pytest.raises(SfmiError, match=word):
        C.keep_components_dev(*_args(), **kw)


def test_keep_option_forms(no_library):
    from shapeformer_amd import components as C
    from shapeformer_amd._lib import SfmiError
    assert C.parse_keep(None) is None
    assert C.parse_keep("largest") == dict(top=1)
    assert C.parse_keep(3) == dict(top=3)
    assert C.parse_keep(0.01) == dict(min_share=0.01, by="area")
    assert C.parse_keep(dict(top=2, by="volume")) == dict(top=2, by="volume")
    for bad in ("biggest", 0, 0.0, 1.5, True, dict(top=0), dict(first=1), [1]):
        with pytest.raises(SfmiError):
            C.parse_keep(bad)
