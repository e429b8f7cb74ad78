"""Mesh decimation on the device (csrc/simplify.hip) against the numpy statement of its contract
(tests/simplify_ref.py).  Meshes come from `marching_cubes_dev` of numpy-built f32 fields and are downloaded, so the reference and the
device see the same vertex bits.  Structure (counts, offsets, faces, the counting pass, the bisected G) is compared without a
tolerance.  Positions carry the one bound of this file:

    |v_dev - v_ref| <= 2^-22 * max|box coordinate|

Both sides accumulate in f64 and the solve's condition number is at most 1 + 1/reg ~ 1e3, so the f64 results agree to ~1e-9 of a
cell; what can show is the final rounding to f32, one ulp (2^-23 at magnitude 1) at most, and the bound is twice that.  It is
absolute because symmetric inputs give coordinates that are zero up to 1e-17."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iso_sparse_ref as R   # noqa: E402
import simplify_ref as S     # noqa: E402

pytestmark = pytest.mark.gpu

BOX = ((-0.9, -1.1, -1.0), (1.3, 0.7, 1.05))
CASES = {"G4": (4, None), "G7": (7, None), "G8": (8, None), "G16": (16, None), "G32": (32, None), "mixed": ((7, 4, 16), None),
         "box": (8, BOX)}        # G = 8 / 16 / 32 put the 33^3 lattice's vertices exactly on cell boundaries


def _tol(bbox):
    return 2.0 ** -22 * float(np.abs(np.asarray(bbox, np.float64)).max())


def _split(v, f, voff, toff):
    v, f = v.cpu().numpy(), f.cpu().numpy()
    return [(v[voff[b]:voff[b + 1]], f[toff[b]:toff[b + 1]]) for b in range(len(voff) - 1)]


@pytest.fixture(scope="module")
def mc(dev):
    """device meshes at Q = 33 (made once): the batch (sphere, empty, two) in the unit box and in BOX, sphere + torus, sphere + two"""
    from shapeformer_amd import mcubes
    F = {n: R.field(n, 33) for n in ("sphere", "empty", "two", "torus")}
    out = {}
    for name, names, bbox in (("unit", ("sphere", "empty", "two"), S.UNIT_BOX), ("box", ("sphere", "empty", "two"), BOX),
                              ("st", ("sphere", "torus"), S.UNIT_BOX), ("sw", ("sphere", "two"), S.UNIT_BOX)):
        d = mcubes.marching_cubes_dev(torch.from_numpy(np.stack([F[n] for n in names])).to(dev), 0.5, bbox)
        out[name] = dict(dev=d, host=_split(*d), bbox=bbox)
    out["fields"] = F
    return out


def _ref_batch(host, grids, bbox, reg=1e-3):
    """the reference shape by shape -> verts, faces, voff, toff, status, (surviving faces, cells) per shape"""
    V, T, vo, to, st, cnt = [], [], [0], [0], [], []
    for (v, f), g in zip(host, grids):
        ov, of, s = S.cluster(v, f, g, bbox, reg)
        V.append(ov), T.append(of), vo.append(vo[-1] + len(ov)), to.append(to[-1] + len(of)), st.append(s)
        cnt.append(S.count(v, f, g, bbox))
    return np.concatenate(V).reshape(-1, 3), np.concatenate(T).reshape(-1, 3), np.array(vo), np.array(to), np.array(st), np.array(cnt)


_runs = {}


def _run(mc, case):
    """device result and reference of a case, computed once for the structure and the position test"""
    if case not in _runs:
        from shapeformer_amd import simplify as SD
        G, bbox = CASES[case]
        m = mc["box" if bbox else "unit"]
        got = SD.cluster_simplify_dev(*m["dev"], G, bbox=m["bbox"])
        counts = SD.cluster_faces_dev(*m["dev"], G, bbox=m["bbox"])
        grids = G if isinstance(G, tuple) else (G,) * 3
        _runs[case] = (got, counts, _ref_batch(m["host"], grids, m["bbox"]), m["bbox"])
    return _runs[case]


@pytest.mark.parametrize("case", list(CASES))
def test_structure_equals_the_reference_exactly(dev, mc, case):
    (v, f, voff, toff, status), (n_surv, n_cells), want, _ = _run(mc, case)
    assert np.array_equal(voff, want[2]) and np.array_equal(toff, want[3])
    assert v.shape == (want[2][-1], 3) and v.dtype == torch.float32 and f.dtype == torch.int32
    assert np.array_equal(f.cpu().numpy(), want[1])
    assert status.cpu().tolist() == want[4].tolist() == [0, 1, 0]              # the empty field has no vertices
    assert np.array_equal(n_surv, want[5][:, 0]) and np.array_equal(n_cells, want[5][:, 1])
    assert np.array_equal(n_surv, np.diff(toff)) and np.array_equal(n_cells, np.diff(voff))
    assert toff[-1] > 0 and voff[1] == voff[2] and toff[1] == toff[2]


@pytest.mark.parametrize("case", list(CASES))
def test_positions_within_an_f32_rounding_of_the_reference(dev, mc, case):
    (v, _, voff, _, _), _, want, bbox = _run(mc, case)
    err = float(np.abs(v.cpu().numpy().astype(np.float64) - want[0].astype(np.float64)).max())
    differ = float((v.cpu().numpy() != want[0]).any(1).mean())
    print(f"simplify positions {case}: max|v_dev - v_ref| = {err:.3e} (bound {_tol(bbox):.3e}), vertices that differ: {differ:.4f}")
    assert err <= _tol(bbox)
    lo, hi = np.asarray(bbox, np.float64)
    assert (v.cpu().numpy() >= lo.astype(np.float32)).all() and (v.cpu().numpy() <= hi.astype(np.float32)).all()


def _upload(meshes, dev):
    """[(verts, faces)] -> the ragged device batch"""
    v = torch.from_numpy(np.concatenate([np.asarray(m[0], np.float32).reshape(-1, 3) for m in meshes])).to(dev)
    f = torch.from_numpy(np.concatenate([np.asarray(m[1], np.int32).reshape(-1, 3) for m in meshes])).to(dev)
    voff = np.concatenate([[0], np.cumsum([len(m[0]) for m in meshes])])
    toff = np.concatenate([[0], np.cumsum([len(m[1]) for m in meshes])])
    return v, f, voff, toff


def test_cube_corners_on_the_device(dev):
    from shapeformer_amd import simplify as SD
    cv, cf = S.cube_mesh(16)
    corners = np.array([[x, y, z] for x in (-.5, .5) for y in (-.5, .5) for z in (-.5, .5)])
    slot = np.searchsorted(np.unique(S.cell_keys(cv, 5)), S.cell_keys(corners, 5))
    dist = {}
    for reg in (1e-8, 1e-3):
        v, f, voff, toff, status = SD.cluster_simplify_dev(*_upload([(cv, cf)], dev), 5, reg=reg)
        assert status.cpu().tolist() == [0] and v.shape == (26, 3) and f.shape == (48, 3)
        assert np.array_equal(f.cpu().numpy(), S.cluster(cv, cf, 5, reg=reg)[1])
        dist[reg] = np.linalg.norm(v.cpu().numpy()[slot].astype(np.float64) - corners, axis=1)
        print(f"cube corners, reg = {reg:g}: distance to the corner {dist[reg].min():.3e} .. {dist[reg].max():.3e}")
    assert dist[1e-8].max() < 1e-6           # the regularisation moves it by ~ 3 reg |m - corner| ~ 1e-8
    assert dist[1e-3].min() > 1e-5           # ~ 4.3e-4: the parameter acts


def test_degenerate_and_stray_input(dev, mc):
    from shapeformer_amd import simplify as SD
    # cell (0,0,0) of G = 2 holds vertices 0, 1 and only faces of the form (a, a, b); vertex 3 is used by no face
    dv = np.array([[-.9, -.9, -.9], [-.8, -.7, -.9], [.5, .5, .5], [.1, -.3, .7]], np.float32)
    df = np.array([[0, 0, 2], [1, 1, 2]], np.int32)
    sphere = mc["unit"]["host"][0]
    v, f, voff, toff, status = SD.cluster_simplify_dev(*_upload([(dv, df), sphere], dev), (2, 8))
    rv, rf, st = S.cluster(dv, df, 2)
    assert status.cpu().tolist() == [0, 0] and voff.tolist()[:2] == [0, 3] and toff.tolist()[:2] == [0, 0]
    got = v.cpu().numpy()[:3]
    assert np.array_equal(got.view(np.uint32), rv.view(np.uint32))             # means of one or two vertices: no order to differ in
    assert np.abs(got[0] - (dv[0].astype(np.float64) + dv[1]) / 2).max() <= _tol(S.UNIT_BOX) and np.array_equal(got[1], dv[3])
    alone = SD.cluster_simplify_dev(*_upload([sphere], dev), 8)
    assert torch.equal(v[3:], alone[0]) and torch.equal(f, alone[1])
    # a face index outside its shape: status 2 and an empty shape; the other shape of the batch is untouched
    bad_f = sphere[1].copy()
    bad_f[17, 1] = len(sphere[0])
    for order in (0, 1):
        meshes = [(sphere[0], bad_f), sphere][::1 - 2 * order]
        v, f, voff, toff, status = SD.cluster_simplify_dev(*_upload(meshes, dev), 8)
        assert status.cpu().tolist() == [[2, 0], [0, 2]][order]
        assert np.array_equal(np.diff(voff), [[0, len(alone[0])], [len(alone[0]), 0]][order])
        assert np.array_equal(np.diff(toff), [[0, len(alone[1])], [len(alone[1]), 0]][order])
        assert torch.equal(v, alone[0]) and torch.equal(f, alone[1])
        n_surv, n_cells = SD.cluster_faces_dev(*_upload(meshes, dev), 8)
        assert n_surv[order] == 0 and n_cells[order] == 0 and n_surv[1 - order] == len(alone[1])
    neg_f = sphere[1].copy()
    neg_f[0, 0] = -1
    assert SD.cluster_simplify_dev(*_upload([(sphere[0], neg_f)], dev), 8)[4].cpu().tolist() == [2]
    # a non-finite vertex: status 3
    for val in (np.nan, np.inf):
        nan_v = sphere[0].copy()
        nan_v[5, 2] = val
        v, f, voff, toff, status = SD.cluster_simplify_dev(*_upload([sphere, (nan_v, sphere[1])], dev), 8)
        assert status.cpu().tolist() == [0, 3] and voff[2] == voff[1] and toff[2] == toff[1]
        assert torch.equal(v, alone[0]) and torch.equal(f, alone[1])
    # no vertices at all, and vertices without faces
    v, f, voff, toff, status = SD.cluster_simplify_dev(*_upload([(dv[:0], df[:0])], dev), 4)
    assert status.cpu().tolist() == [1] and v.shape == (0, 3) and f.shape == (0, 3)
    v, f, voff, toff, status = SD.cluster_simplify_dev(*_upload([(dv, df[:0])], dev), 2)
    assert status.cpu().tolist() == [0] and f.shape == (0, 3) and np.array_equal(v.cpu().numpy(), S.cluster(dv, df[:0], 2)[0])


def test_deterministic_and_batch_equals_per_shape_calls(dev, mc):
    from shapeformer_amd import simplify as SD
    m = mc["unit"]
    G = (7, 4, 16)
    a = SD.cluster_simplify_dev(*m["dev"], G)
    b = SD.cluster_simplify_dev(*m["dev"], G)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    for k, (hv, hf) in enumerate(m["host"]):
        one = SD.cluster_simplify_dev(*_upload([(hv, hf)], dev), G[k])
        assert torch.equal(one[0].view(torch.int32), a[0][a[2][k]:a[2][k + 1]].view(torch.int32))
        assert torch.equal(one[1], a[1][a[3][k]:a[3][k + 1]])
        assert one[4].cpu().tolist() == [a[4].cpu().tolist()[k]]


def test_face_budget(dev, mc):
    from shapeformer_amd import simplify as SD
    m = mc["st"]                                                              # sphere 3512 faces, torus 3520
    before = SD.read_backs
    v, f, voff, toff, status, G = SD.decimate_dev(*m["dev"], decimate_face=512)
    assert SD.read_backs - before <= 11                                        # at most 10 counting passes, one clustering pass
    want_G = [S.bisect(hv, hf, 512) for hv, hf in m["host"]]
    assert G.tolist() == want_G == [15, 13] and status.cpu().tolist() == [0, 0]
    for k, (hv, hf) in enumerate(m["host"]):
        assert toff[k + 1] - toff[k] <= 512 < S.count(hv, hf, G[k] + 1)[0]
        rv, rf, _ = S.cluster(hv, hf, G[k])
        assert np.array_equal(f.cpu().numpy()[toff[k]:toff[k + 1]], rf) and voff[k + 1] - voff[k] == len(rv)
        assert np.abs(v.cpu().numpy()[voff[k]:voff[k + 1]].astype(np.float64) - rv).max() <= _tol(S.UNIT_BOX)
    # at or below the budget: the same tensors, bit for bit
    v0, f0, voff0, toff0 = m["dev"]
    v, f, voff, toff, status, G = SD.decimate_dev(v0, f0, voff0, toff0, decimate_face=4096)
    assert torch.equal(v.view(torch.int32), v0.view(torch.int32)) and torch.equal(f, f0) and G.tolist() == [0, 0]
    assert np.array_equal(voff, voff0) and np.array_equal(toff, toff0) and status.cpu().tolist() == [0, 0]
    # one shape over and one under the budget: each by its own rule
    m = mc["sw"]                                                              # sphere 3512 faces, two spheres 1284
    v0, f0, voff0, toff0 = m["dev"]
    assert toff0[1] > 2048 >= toff0[2] - toff0[1]
    v, f, voff, toff, status, G = SD.decimate_dev(v0, f0, voff0, toff0, decimate_face=2048)
    assert G.tolist() == [S.bisect(*m["host"][0], 2048), 0] == [31, 0] and status.cpu().tolist() == [0, 0]
    alone = SD.decimate_dev(*_upload([m["host"][0]], dev), decimate_face=2048)
    assert torch.equal(v[:voff[1]].view(torch.int32), alone[0].view(torch.int32)) and torch.equal(f[:toff[1]], alone[1])
    assert toff[1] <= 2048 and np.array_equal(f[:toff[1]].cpu().numpy(), S.cluster(*m["host"][0], 31)[1])
    assert torch.equal(v[voff[1]:].view(torch.int32), v0[voff0[1]:].view(torch.int32)) and torch.equal(f[toff[1]:], f0[toff0[1]:])


def test_array2mesh_keywords(dev, mc):
    from shapeformer_amd import mcubes, simplify as SD
    occ = mc["fields"]["sphere"]
    d = mcubes.marching_cubes_dev(torch.from_numpy(occ[None]).to(dev), 0.5)
    v, f = mcubes.array2mesh(occ, device=dev)                                  # the default: today's output, bit for bit
    assert v.dtype == np.float64 and np.array_equal(v, d[0].cpu().numpy().astype(np.float64)) and np.array_equal(f, d[1].cpu().numpy())
    v, f = mcubes.array2mesh(occ, if_decimate=False, decimate_face=512, device=dev)
    assert len(f) == len(d[1])
    want = SD.decimate_dev(*d, decimate_face=512)
    v, f = mcubes.array2mesh(occ, if_decimate=True, decimate_face=512, device=dev)
    assert len(f) <= 512 and np.array_equal(f, want[1].cpu().numpy()) and np.array_equal(v, want[0].cpu().numpy().astype(np.float64))
    v, f = mcubes.array2mesh(occ, if_decimate=True, device=dev)               # 3512 faces <= 4096: unchanged
    assert np.array_equal(v, d[0].cpu().numpy().astype(np.float64)) and np.array_equal(f, d[1].cpu().numpy())
    # coords name the box for both steps
    c = np.array([BOX[0], BOX[1]])
    v, f = mcubes.array2mesh(occ, coords=c, if_decimate=True, decimate_face=512, device=dev)
    db = mcubes.marching_cubes_dev(torch.from_numpy(occ[None]).to(dev), 0.5, BOX)
    wb = SD.decimate_dev(*db, decimate_face=512, bbox=BOX)
    assert np.array_equal(f, wb[1].cpu().numpy()) and np.array_equal(v, wb[0].cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("route", ["dense", "sparse"])
def test_callback_decimate_face(dev, tmp_path, route):
    """VisShapeFormer(decimate_face=n): the written and returned meshes have at most n faces and are decimate_dev of the undecimated
    ones; eval/*.npz is what a run without the keyword writes.  The model setup of test_iso_sparse_gpu.py's callback test."""
    from test_plugin_gpu import _Items, _opt
    from shapeformer_amd import meshio, plugin as P, simplify as SD
    budget = 300
    model = P.instantiate_from_opt(P.get_opt(_opt())["pl_model_opt"])
    kw = dict(end_tokens=[4096, 4096], top_k=100, top_p=0.4, depth=4, visual_indices=[0], sample_n=2, sample_max_step=12)
    kw.update(dict(decode_res=32) if route == "dense" else dict(decode_res=65, sparse_decode=True, sparse_coarse=17))
    name = "shapeformer.models.shapeformer.shapeformer.VisShapeFormer"
    plain = P.instantiate_from_opt({"class": name, "kwargs": dict(kw, data_dir=str(tmp_path / "plain"))})
    deci = P.instantiate_from_opt({"class": name, "kwargs": dict(kw, decimate_face=budget, data_dir=str(tmp_path / "deci"))})
    assert plain.decimate_face is None and deci.decimate_face == budget
    plain.process(model, _Items(1))
    computed = np.load(tmp_path / "plain" / "computed" / "0.npy", allow_pickle=True).item()
    deci.pl_module = model
    np.random.seed(0)                                                          # the surface samples of eval/ come from numpy's global RNG
    out0 = plain.visualize_batch(computed, input_name="0", data_dir=str(tmp_path / "plain"))
    np.random.seed(0)
    out1 = deci.visualize_batch(computed, input_name="0", data_dir=str(tmp_path / "deci"))
    keys = [k for k in out0 if k.endswith("_mesh")]
    assert keys and sorted(keys) == sorted(k for k in out1 if k.endswith("_mesh"))
    shrunk = 0
    for k in keys:
        m0, m1 = out0[k], out1[k]
        v0 = torch.from_numpy(m0["vert"].astype(np.float32)).to(dev)
        want = SD.decimate_dev(v0, torch.from_numpy(m0["face"].astype(np.int32)).to(dev), [0, len(v0)], [0, len(m0["face"])], budget)
        assert len(m1["face"]) <= budget
        assert np.array_equal(m1["face"], want[1].cpu().numpy()) and np.array_equal(m1["vert"], want[0].cpu().numpy().astype(np.float64))
        v2, f2 = meshio.read_ply(m1["path"])
        assert np.array_equal(v2, m1["vert"]) and np.array_equal(f2, m1["face"])
        shrunk += len(m0["face"]) > budget
    assert shrunk > 0                                                          # the budget really bit
    e0, e1 = np.load(tmp_path / "plain" / "eval" / "0.npz"), np.load(tmp_path / "deci" / "eval" / "0.npz")
    assert sorted(e0.files) == sorted(e1.files) and all(np.array_equal(e0[k], e1[k]) for k in e0.files)


def test_sparse_recon_callback_decimate_face(dev, tmp_path):
    from test_plugin_gpu import _Items
    from shapeformer_amd import callbacks as CB, weights as W
    from shapeformer_amd.vqdif import VQDIF
    vq = VQDIF(W.make_state_dict(W.vqdif_spec(16)), res=16, device=dev)
    outs = []
    for budget in (None, 300):
        cb = CB.VisSparseRecon3D(quant_grid_depth=4, decoder_resolution=32, visual_indices=[0], decimate_face=budget,
                                 data_dir=str(tmp_path / str(budget)))
        np.random.seed(0)
        outs.append(cb.process(vq, _Items(1))["0"])
    assert len(outs[0]["recon_mesh"]["face"]) > 300 >= len(outs[1]["recon_mesh"]["face"]) > 0
    assert np.array_equal(outs[0]["eval_pc"], outs[1]["eval_pc"])


def test_refusals_before_any_launch(dev, mc):
    from shapeformer_amd import _lib as L, simplify as SD
    v, f, voff, toff = mc["unit"]["dev"]
    for grid in (0, 513, (4, 4), (4, 4, 600)):
        with pytest.raises(L.SfmiError, match="grid"):
            SD.cluster_simplify_dev(v, f, voff, toff, grid)
        with pytest.raises(L.SfmiError, match="grid"):
            SD.cluster_faces_dev(v, f, voff, toff, grid)
    for call in (lambda: SD.cluster_simplify_dev(v.cpu(), f, voff, toff, 8), lambda: SD.cluster_faces_dev(v, f.cpu(), voff, toff, 8),
                 lambda: SD.decimate_dev(v.cpu(), f.cpu(), voff, toff, 64)):
        with pytest.raises(L.SfmiError, match="no CPU fallback"):
            call()
    with pytest.raises(L.SfmiError, match="offsets"):
        SD.cluster_simplify_dev(v, f, voff[:-1], toff[:-1], 8)
    lib, E = L.lib(), L.SFMI_EINVAL
    buf = torch.zeros(4096, device=dev, dtype=torch.int32)
    p = L.ptr(buf)
    lo, hi = np.array([-1.0] * 3), np.array([1.0] * 3)
    for bad in (0, 513):
        gb = np.array([bad], np.int32)
        assert lib.sfmi_simplify_cells_f32(p, p, p, p, L.ptr(gb), p, p, 1, 3, 1, L.ptr(lo), L.ptr(hi), p, p, p, None) == E
        assert lib.sfmi_simplify_popc_i32(p, p, p, L.ptr(gb), 1, p, p, None) == E
        assert lib.sfmi_simplify_slots_i32(p, p, p, p, p, p, L.ptr(gb), 1, 3, p, None) == E
        assert lib.sfmi_simplify_solve_f32(p, p, p, p, L.ptr(gb), p, p, p, p, p, 1, 1, L.ptr(lo), L.ptr(hi), 1e-3, p, None) == E
    g = L.ptr(np.array([8], np.int32))
    assert lib.sfmi_simplify_cells_f32(p, p, p, p, g, p, p, 1, 3, 1, L.ptr(lo), L.ptr(hi), None, p, p, None) == E
    assert lib.sfmi_simplify_cells_f32(p, p, p, p, g, p, p, 1, 3, 1, L.ptr(hi), L.ptr(lo), p, p, p, None) == E
    assert lib.sfmi_simplify_faces_i32(p, p, p, p, p, 1, 1, p, None, p, None) == E
    assert lib.sfmi_simplify_solve_f32(p, p, p, p, g, p, p, p, p, p, 1, 1, L.ptr(lo), L.ptr(hi), -1.0, p, None) == E
    assert lib.sfmi_simplify_emit_i32(p, p, p, None, p, p, p, 1, 1, 1, p, None) == E
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0                                           # nothing was launched on the buffer
