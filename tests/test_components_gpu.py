"""GPU tests of the mesh connected components (csrc/components.hip) against the numpy statement of
tests/components_ref.py.

Connected components are an integer problem: labels, counts, keep flags and compacted meshes are compared with array_equal.  Only the
f64 sums differ in order: area / volume are compared per component to within (n_face + 8) * 2^-52 * sum |term|, the reordering bound of
an f64 sum plus a few ulp per term.  All fixtures come from seeded numpy generators."""
import os

import numpy as np
import pytest
import torch

import components_ref as R

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _cat(shapes):
    """list of (verts, faces) -> ragged batch arrays"""
    v = np.concatenate([np.asarray(s[0], np.float32).reshape(-1, 3) for s in shapes]) if shapes else np.zeros((0, 3), np.float32)
    f = np.concatenate([np.asarray(s[1], np.int32).reshape(-1, 3) for s in shapes]) if shapes else np.zeros((0, 3), np.int32)
    voff = np.concatenate([[0], np.cumsum([len(s[0]) for s in shapes])]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([len(s[1]) for s in shapes])]).astype(np.int64)
    return v, f, voff, toff


def _to(dev, v, f):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev), torch.from_numpy(np.ascontiguousarray(f)).to(dev)


def _label(dev, shapes):
    from shapeformer_amd.components import mesh_components_dev
    v, f, voff, toff = _cat(shapes)
    vl, fl, coff, stats, status = mesh_components_dev(*_to(dev, v, f), voff, toff)
    return (vl.cpu().numpy(), fl.cpu().numpy(), np.asarray(coff), {k: t.cpu().numpy() for k, t in stats.items()}, status.cpu().numpy(),
            voff, toff)


def _check_labels(dev, shapes):
    """the device's labels, statistics and status of a batch against the reference, shape by shape -> the device's outputs"""
    vl, fl, coff, stats, status, voff, toff = _label(dev, shapes)
    assert vl.dtype == np.int32 and fl.dtype == np.int32 and stats["n_vert"].dtype == np.int32 and stats["area"].dtype == np.float64
    assert len(coff) == len(shapes) + 1 and coff[0] == 0 and len(stats["area"]) == coff[-1]
    for b, (v, f) in enumerate(shapes):
        rvl, rfl, rst, rs = R.components(v, f)
        assert status[b] == rs, (b, status[b], rs)
        assert np.array_equal(vl[voff[b]:voff[b + 1]], rvl), b
        assert np.array_equal(fl[toff[b]:toff[b + 1]], rfl), b
        sl = slice(coff[b], coff[b + 1])
        assert coff[b + 1] - coff[b] == len(rst["area"]), b
        assert np.array_equal(stats["n_vert"][sl], rst["n_vert"]) and np.array_equal(stats["n_face"][sl], rst["n_face"]), b
        for name in ("area", "volume"):
            tol = (rst["n_face"] + 8) * EPS * rst["abs_" + name]
            err = np.abs(stats[name][sl] - rst[name])
            assert (err <= tol).all(), (b, name, float(err.max()), float(tol[np.argmax(err - tol)]))
    return vl, fl, coff, stats, status


def _keep(dev, shapes, **kw):
    from shapeformer_amd.components import keep_components_dev
    v, f, voff, toff = _cat(shapes)
    kv, kf, kvo, kto, status, kept, coff = keep_components_dev(*_to(dev, v, f), voff, toff, **kw)
    assert kv.dtype == torch.float32 and kf.dtype == torch.int32 and kept.dtype == torch.bool
    return kv.cpu().numpy(), kf.cpu().numpy(), np.asarray(kvo), np.asarray(kto), status.cpu().numpy(), kept.cpu().numpy(), np.asarray(coff)


def _check_keep(dev, shapes, **kw):
    kv, kf, kvo, kto, status, kept, coff = _keep(dev, shapes, **kw)
    assert kvo[-1] == len(kv) and kto[-1] == len(kf) and len(kept) == coff[-1]
    for b, (v, f) in enumerate(shapes):
        rv, rf, rs, rk = R.keep(v, f, **kw)
        assert status[b] == rs
        assert np.array_equal(kept[coff[b]:coff[b + 1]], rk), b
        assert np.array_equal(kv[kvo[b]:kvo[b + 1]].view(np.int32), rv.view(np.int32)), b
        assert np.array_equal(kf[kto[b]:kto[b + 1]], rf), b
    return kv, kf, kvo, kto, status, kept, coff


def test_empty_batch(dev):
    from shapeformer_amd import components as C
    v, f = torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev, dtype=torch.int32)
    vl, fl, coff, stats, status = C.mesh_components_dev(v, f, [0], [0])
    assert vl.numel() == fl.numel() == status.numel() == 0 and list(coff) == [0] and all(t.numel() == 0 for t in stats.values())
    kv, kf, kvo, kto, status, kept, coff = C.keep_components_dev(v, f, [0], [0], top=1)
    assert kv.shape == (0, 3) and kf.shape == (0, 3) and list(kvo) == [0] and list(kto) == [0] and kept.numel() == 0 and list(coff) == [0]


def test_shape_without_vertices(dev):
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    vl, fl, coff, stats, status = _check_labels(dev, [empty])
    assert status.tolist() == [1] and coff.tolist() == [0, 0]
    kv, kf, kvo, kto, status, kept, coff = _check_keep(dev, [empty], top=1)
    assert status.tolist() == [1] and len(kv) == 0 and len(kf) == 0


@pytest.mark.parametrize("name", sorted(R.small_meshes()))
def test_small_meshes(dev, name):
    v, f, C = R.small_meshes()[name]
    vl, fl, coff, stats, status = _check_labels(dev, [(v, f)])
    assert coff[-1] == C and status.tolist() == [0]
    _check_keep(dev, [(v, f)], top=1)


@pytest.mark.parametrize("numbering", ["ascending", "descending", "permuted"])
def test_strip_is_one_component(dev, numbering):
    """5000 triangles in one component; descending indices make the longest hook chains, the shuffled face order puts both ends of a late
    union into different workgroups"""
    v, f = R.strip(5000, numbering)
    vl, fl, coff, stats, status = _check_labels(dev, [(v, f)])
    assert (vl == 0).all() and (fl == 0).all() and coff.tolist() == [0, 1]
    assert stats["n_vert"].tolist() == [5002] and stats["n_face"].tolist() == [5000]


def test_thousand_tetrahedra(dev):
    v, f, tet_of, vol, formula = R.tetrahedra(1000)
    vl, fl, coff, stats, status = _check_labels(dev, [(v, f)])
    assert coff[-1] == 1000 and (stats["n_vert"] == 4).all() and (stats["n_face"] == 4).all()
    first = np.array([np.flatnonzero(vl == c)[0] for c in range(1000)])
    assert (np.diff(first) > 0).all()                                       # numbered by smallest vertex
    assert np.array_equal(tet_of[first][vl], tet_of)                        # every component is one tetrahedron
    # the closed form s^3 / 6: the fixture's coordinates make every triple product exact, so each face term is the exact one rounded
    # once and the device's sum of four is within the sum's own bound of the formula
    want = formula[tet_of[first]]
    assert np.array_equal(want, vol[tet_of[first]])
    assert (np.abs(stats["volume"] - want) <= (4 + 8) * EPS * R.components(v, f)[2]["abs_volume"]).all()
    kv, kf, kvo, kto, _, kept, _ = _check_keep(dev, [(v, f)], top=10, by="volume")
    assert kept.sum() == 10 and set(np.flatnonzero(kept)) == set(np.argsort(-want)[:10])
    assert len(kv) == 40 and len(kf) == 40


def test_unreferenced_vertices_and_degenerate_face(dev):
    rng = np.random.default_rng(11)
    v = rng.uniform(-1, 1, (9, 3)).astype(np.float32)
    f = np.array([[6, 6, 2], [1, 4, 7]], np.int32)                          # 0, 3, 5, 8 are named by no face
    vl, fl, coff, stats, status = _check_labels(dev, [(v, f)])
    assert vl.tolist() == [-1, 0, 1, -1, 0, -1, 1, 0, -1] and fl.tolist() == [1, 0]
    assert stats["n_vert"].tolist() == [3, 2] and stats["area"][1] == 0.0 and stats["area"][0] > 0
    kv, kf, kvo, kto, _, kept, _ = _check_keep(dev, [(v, f)])
    assert kept.all() and np.array_equal(kv, v[[1, 2, 4, 6, 7]]) and kf.tolist() == [[3, 3, 1], [0, 2, 4]]


def _three_shapes():
    tv, tf = R.tetrahedra(37, seed=2)[:2]
    sv, sf = R.strip(700, "permuted", seed=3)
    dv, df, _ = R.small_meshes()["disjoint"]
    # a second, detached piece on the strip's shape, so that it has something to drop
    sv2, sf2 = np.concatenate([sv, dv + 3.0]), np.concatenate([sf, df + len(sv)])
    return [(tv, tf), (sv2, sf2.astype(np.int32)), (np.concatenate([dv, dv]), np.concatenate([df, df[:1] + 6]).astype(np.int32))]


def test_batch_equals_per_shape_calls_and_runs_repeat(dev):
    from shapeformer_amd import components as C
    shapes = _three_shapes()
    v, f, voff, toff = _cat(shapes)
    dv, df = _to(dev, v, f)
    _check_labels(dev, shapes)
    kw = dict(top=2, min_share=0.3, by="area")
    _check_keep(dev, shapes, **kw)
    runs = []
    for _ in range(2):
        lab = C.mesh_components_dev(dv, df, voff, toff)
        kept = C.keep_components_dev(dv, df, voff, toff, **kw)
        runs.append((lab, kept))
    (lab, kept), (lab2, kept2) = runs
    for a, b in ((lab[0], lab2[0]), (lab[1], lab2[1]), (lab[4], lab2[4]), (kept[0], kept2[0]), (kept[1], kept2[1]), (kept[5], kept2[5])):
        assert torch.equal(a, b)
    for k in lab[3]:
        assert torch.equal(lab[3][k], lab2[3][k]), k                         # the f64 sums included, bit for bit
    for b, (sv, sf) in enumerate(shapes):
        one = C.mesh_components_dev(*_to(dev, sv, sf), [0, len(sv)], [0, len(sf)])
        assert torch.equal(one[0], lab[0][voff[b]:voff[b + 1]]) and torch.equal(one[1], lab[1][toff[b]:toff[b + 1]])
        for k in one[3]:
            assert torch.equal(one[3][k], lab[3][k][lab[2][b]:lab[2][b + 1]]), (b, k)
        ko = C.keep_components_dev(*_to(dev, sv, sf), [0, len(sv)], [0, len(sf)], **kw)
        assert torch.equal(ko[0], kept[0][kept[2][b]:kept[2][b + 1]]) and torch.equal(ko[1], kept[1][kept[3][b]:kept[3][b + 1]])
        assert torch.equal(ko[5], kept[5][kept[6][b]:kept[6][b + 1]])


@pytest.mark.parametrize("code", [2, 3])
def test_bad_shape_comes_back_empty_and_leaves_its_neighbours_alone(dev, code):
    shapes = _three_shapes()
    v, f = shapes[1][0].copy(), shapes[1][1].copy()
    if code == 2:
        f[len(f) // 2, 1] = len(v)                                          # an index equal to the shape's vertex count
    else:
        v[len(v) // 3, 2] = np.nan
    bad = [shapes[0], (v, f), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), shapes[2]]
    vl, fl, coff, stats, status = _check_labels(dev, bad)
    assert status.tolist() == [0, code, 1, 0] and coff[2] == coff[1] == coff[3]
    kv, kf, kvo, kto, status, kept, _ = _check_keep(dev, bad, top=1)
    assert kvo[2] == kvo[1] and kto[2] == kto[1] and status.tolist() == [0, code, 1, 0]
    good = _keep(dev, [shapes[0], shapes[2]], top=1)
    assert np.array_equal(kv, good[0]) and np.array_equal(kf, good[1])


def test_keep_all_is_the_identity_and_min_share_one_keeps_the_ties(dev):
    v, f = R.tetrahedra(64, seed=7)[:2]
    kv, kf, kvo, kto, _, kept, _ = _check_keep(dev, [(v, f)])
    assert kept.all() and np.array_equal(kv.view(np.int32), v.view(np.int32)) and np.array_equal(kf, f)
    # two congruent triangles on small integers (equal areas, exactly) and a smaller one between them
    tri = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], np.float32)
    tv = np.concatenate([tri, 0.5 * tri + np.float32(8), tri + np.float32(4)])
    tf = np.arange(9, dtype=np.int32).reshape(3, 3)
    for by in ("area", "faces"):
        kv, kf, _, _, _, kept, _ = _check_keep(dev, [(tv, tf)], min_share=1.0, by=by)
        assert kept.tolist() == ([True, False, True] if by == "area" else [True, True, True])
    kv, kf, _, _, _, kept, _ = _check_keep(dev, [(tv, tf)], min_share=1.0, top=1)
    assert kept.tolist() == [True, False, False]                            # equal measures rank by id


@pytest.fixture(scope="module")
def lattice(dev):
    from shapeformer_amd.mcubes import marching_cubes_dev
    f0, fall = R.sphere_field()
    one = marching_cubes_dev(torch.from_numpy(f0)[None].to(dev))
    three = marching_cubes_dev(torch.from_numpy(fall)[None].to(dev))
    return dict(f0=f0, fall=fall, one=one, three=three)


def test_lattice_end_to_end(dev, lattice):
    from shapeformer_amd.components import keep_components_dev, mesh_components_dev
    v1, f1, _, _ = lattice["one"]
    v, f, voff, toff = lattice["three"]
    assert len(v) > len(v1)
    vl, fl, coff, stats, status = mesh_components_dev(v, f, voff, toff)
    assert coff.tolist() == [0, 3] and status.tolist() == [0] and int(vl.min()) == 0
    _check_labels(dev, [(v.cpu().numpy(), f.cpu().numpy())])
    kv, kf, kvo, kto, _, kept, _ = keep_components_dev(v, f, voff, toff, top=1)
    assert int(kept.sum()) == 1
    # the fields agree on every cell sphere 0 cuts and compaction preserves order: the large sphere's mesh, bit for bit
    assert torch.equal(kv.view(torch.int32), v1.view(torch.int32)) and torch.equal(kf, f1)
    assert kvo.tolist() == [0, len(v1)] and kto.tolist() == [0, len(f1)]


def test_array2mesh_keep_largest(dev, lattice):
    from shapeformer_amd.mcubes import array2mesh
    v1, f1 = array2mesh(lattice["f0"], device=dev)
    kv, kf = array2mesh(lattice["fall"], device=dev, keep_components="largest")
    assert kv.dtype == np.float64 and kf.dtype == np.dtype(int)
    assert np.array_equal(kv, v1) and np.array_equal(kf, f1)
    av, af = array2mesh(lattice["fall"], device=dev)
    assert len(av) > len(kv)
    dv, df = array2mesh(lattice["fall"], device=dev, keep_components="largest", if_decimate=True, decimate_face=200)
    assert 0 < len(df) <= 200 and R.labels(len(dv), df)[2] >= 1


def test_reconstruction_callback_keeps_the_largest_piece(dev, tmp_path):
    from shapeformer_amd import meshio, plugin as P
    from test_plugin_gpu import _Items, _opt
    model = P.instantiate_from_opt(P.get_opt(_opt())["pl_model_opt"])
    data = _Items(2)
    kw = dict(quant_grid_depth=4, decoder_resolution=32, max_length=512, end_tokens=[4096, 4096], visual_indices=[1])
    name = "shapeformer.models.vqdif.vqdif.VisSparseRecon3D"
    off = P.instantiate_from_opt({"class": name, "kwargs": dict(kw, data_dir=str(tmp_path / "off"))}).process(model.representer.vqvae_model, data)["1"]
    on = P.instantiate_from_opt({"class": name, "kwargs": dict(kw, data_dir=str(tmp_path / "on"), keep_components="largest")}).process(
        model.representer.vqvae_model, data)["1"]
    assert set(off) == {"recon_mesh", "mesh_path", "eval_pc"}                # what the callback returns today
    assert set(on) == set(off) | {"components"}
    rep = on["components"]
    assert set(rep) == {"count", "kept", "area_removed"} and rep["kept"] == 1 and rep["count"] >= 1 and 0.0 <= rep["area_removed"] < 1.0
    v0, f0 = meshio.read_ply(off["mesh_path"])
    v, f = meshio.read_ply(on["mesh_path"])
    vl, fl, C = R.labels(len(v), f)
    assert C == 1 and (vl == 0).all()
    assert R.labels(len(v0), f0)[2] == rep["count"]
    assert (rep["count"] == 1) == (rep["area_removed"] == 0.0) and len(f) <= len(f0)
    assert np.array_equal(on["recon_mesh"]["vert"], v) and np.array_equal(on["recon_mesh"]["face"], f)


@pytest.mark.parametrize("sparse", [False, True])
def test_completion_callback_filters_every_mesh(dev, tmp_path, sparse):
    """VisShapeFormer(keep_components=...): every written mesh is one piece, `components` names the written mesh keys, the metrics file
    carries the same entries, and the option off returns the keys it returns today"""
    import json
    from shapeformer_amd import meshio, plugin as P
    from test_plugin_gpu import _Items, _opt
    model = P.instantiate_from_opt(P.get_opt(_opt())["pl_model_opt"])
    data = _Items(1)
    kw = dict(end_tokens=[4096, 4096], top_k=100, top_p=0.4, depth=4, visual_indices=[0], sample_n=2, sample_max_step=8,
              decode_res=33 if sparse else 32, eval_metrics=True, eval_points=2048, sparse_decode=sparse, sparse_coarse=9)
    name = "shapeformer.models.shapeformer.shapeformer.VisShapeFormer"
    off = P.instantiate_from_opt({"class": name, "kwargs": dict(kw, data_dir=str(tmp_path / "off"))}).process(model, data)["0"]
    on = P.instantiate_from_opt({"class": name, "kwargs": dict(kw, data_dir=str(tmp_path / "on"), keep_components="largest")}).process(
        model, data)["0"]
    assert "components" not in off and "components" in on
    meshes = sorted(k for k in on if k.endswith("_mesh"))
    assert meshes and sorted(on["components"]) == meshes and set(meshes) <= set(off)
    assert set(on) - {"components"} <= set(off)
    for k in meshes:
        v, f = meshio.read_ply(on[k]["path"])
        assert R.labels(len(v), f)[2] == 1 and on["components"][k]["kept"] == 1
        v0, f0 = meshio.read_ply(off[k]["path"])
        assert R.labels(len(v0), f0)[2] == on["components"][k]["count"]
    if "metrics" in on:
        saved = json.load(open(tmp_path / "on" / "eval" / "0_metrics.json"))
        assert saved["components"] == {k + "_mesh": on["components"][k + "_mesh"] for k in saved["keys"]}
        assert "components" not in json.load(open(tmp_path / "off" / "eval" / "0_metrics.json"))


def test_c_abi_refusals(dev):
    """every entry refuses a null pointer and a negative count with SFMI_EINVAL, before any launch"""
    from shapeformer_amd import _lib as L
    lib, E = L.lib(), L.SFMI_EINVAL
    ibuf = torch.zeros(64, device=dev, dtype=torch.int32)
    off = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    p, o = L.ptr(ibuf), L.ptr(off)
    assert lib.sfmi_cc_chunk() == 1024
    # name -> (arguments of a well-formed call with B = 1, V = T = 4, positions of the pointers, positions of the counts)
    calls = {
        "sfmi_cc_init_f32": ([p, p, o, o, 1, 4, 4, p, p, p, None], [0, 1, 2, 3, 7, 8, 9], [4, 5, 6]),
        "sfmi_cc_hook_i32": ([p, o, o, p, 1, 4, 4, p, p, None], [0, 1, 2, 3, 7, 8], [4, 5, 6]),
        "sfmi_cc_flatten_i32": ([p, p, 4, p, p, None], [0, 1, 3, 4], [2]),
        "sfmi_cc_number_i32": ([p, o, o, p, p, p, p, o, 1, 4, 4, p, p, p, p, p, None], [0, 1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14, 15], [8, 9, 10]),
        "sfmi_cc_stats_f64": ([p, p, o, o, p, p, p, 1, 4, 4, 5, 8, p, p, p, None], [0, 1, 2, 3, 4, 5, 6, 12, 13, 14], [7, 8, 9, 10, 11]),
        "sfmi_cc_mark_i32": ([p, p, o, o, o, p, 1, 4, 4, 5, p, p, None], [0, 1, 2, 3, 4, 5, 10, 11], [6, 7, 8, 9]),
        "sfmi_cc_emit_f32": ([p, p, o, o, p, p, p, p, o, 1, 4, 4, 4, 4, p, p, None], [0, 1, 2, 3, 4, 5, 6, 7, 8, 14, 15], [9, 10, 11, 12, 13]),
    }
    for name, (args, pointers, counts) in calls.items():
        fn = getattr(lib, name)
        for i in pointers:
            bad = list(args)
            bad[i] = None
            assert fn(*bad) == E, (name, "NULL at", i)
        for i in counts:
            bad = list(args)
            bad[i] = -1
            assert fn(*bad) == E, (name, "-1 at", i)
    assert lib.sfmi_cc_init_f32(p, p, o, o, 0, 4, 4, p, p, p, None) == E    # B = 0
    assert lib.sfmi_cc_emit_f32(p, p, o, o, p, p, p, p, o, 1, 4, 4, 5, 4, p, p, None) == E   # more kept vertices than vertices
    torch.cuda.synchronize()
    assert int(ibuf.abs().sum()) == 0                                       # nothing was launched
