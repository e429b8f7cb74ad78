"""Coarse-to-fine sparse iso-surface extraction on the device (csrc/iso_sparse.hip, the keyed form of csrc/sdf_query.hip)
against the numpy statement of the contract (tests/iso_sparse_ref.py) and the dense route it thins out.  Fields are built in numpy f32
and uploaded, so the device and the reference see identical bits; expected vertices are rows of the dense device mesh.  No tolerance
appears anywhere: every comparison is exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iso_sparse_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu


def _dense(F, iso, bbox=None):
    from shapeformer_amd import mcubes
    v, f, voff, toff = mcubes.marching_cubes_dev(F, iso) if bbox is None else mcubes.marching_cubes_dev(F, iso, bbox)
    return v.cpu().numpy(), f.cpu().numpy(), np.asarray(voff), np.asarray(toff)


def _expect_selection(Fs, iso, finals, dense):
    """the reference's selection out of the dense device mesh of every shape -> verts, faces, voff, toff"""
    v, f, voff, toff = dense
    V, T, vo, to = [], [], [0], [0]
    for b, F in enumerate(Fs):
        vb, fb = v[voff[b]:voff[b + 1]], f[toff[b]:toff[b + 1]]
        vs, ts, fn = R.select_mesh(F, iso, finals[b], len(vb), fb)
        V.append(vb[vs]), T.append(fn), vo.append(vo[-1] + len(vs)), to.append(to[-1] + len(ts))
    return np.concatenate(V).reshape(-1, 3), np.concatenate(T).reshape(-1, 3), np.array(vo), np.array(to)


def _assert_mesh(got, want):
    v, f, voff, toff = got
    assert np.array_equal(np.asarray(voff), want[2]) and np.array_equal(np.asarray(toff), want[3])
    assert np.array_equal(f.cpu().numpy(), want[1])
    assert np.array_equal(v.cpu().numpy().view(np.uint32), np.ascontiguousarray(want[0]).view(np.uint32))     # bitwise


@pytest.mark.parametrize("margin", [0, 1])
@pytest.mark.parametrize("Q0,L", [(5, 2), (9, 3)])
def test_structure_and_mesh_against_the_reference(dev, Q0, L, margin):
    from shapeformer_amd import iso_sparse as IS
    Q = (Q0 - 1) * 2 ** L + 1
    Fs = [R.field(n, Q) for n in ("sphere", "empty", "two")]
    refs = [R.hierarchy(F, Q0, L, 0.5, margin) for F in Fs]
    if (Q0, L, margin) == (9, 3, 0):      # the restricted branch is really exercised: `two` loses cut cells of its small sphere
        assert 0 < refs[2]["final"].sum() < R.dense_cut_cells(Fs[2], 0.5).sum()
    Fd = torch.from_numpy(np.stack(Fs)).to(dev)
    got = IS.extract_sparse_dev(IS.table_field(Fd), 3, Q0, L, thresh=0.5, margin=margin, return_levels=True, device=dev)
    info = got[4]
    for l in range(L + 1):
        for name in ("S", "M"):
            keys, off = info[name][l]
            want = [r[name][l] for r in refs]
            assert np.array_equal(np.asarray(off), np.concatenate([[0], np.cumsum([len(w) for w in want])])), (name, l)
            assert np.array_equal(keys.cpu().numpy(), np.concatenate(want)), (name, l)
        assert np.array_equal(info["points"][l], [r["points"][l] for r in refs]), l
    _assert_mesh(got[:4], _expect_selection(Fs, 0.5, [r["final"] for r in refs], _dense(Fd, 0.5)))
    assert got[2][1] == got[2][2] and got[3][1] == got[3][2]      # the empty shape contributes nothing
    assert len(refs[1]["M"][0]) == 0 and got[3][-1] > 0
    # deterministic from run to run
    again = IS.extract_sparse_dev(IS.table_field(Fd), 3, Q0, L, thresh=0.5, margin=margin, device=dev)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.parametrize("case", ["sphere", "torus", "open", "slab", "sphere-bbox", "sphere-isoplane", "torus-isoplane"])
def test_full_coverage_equals_the_dense_mesh(dev, case):
    from shapeformer_amd import iso_sparse as IS
    Q0, L, Q = 9, 2, 33
    name, _, variant = case.partition("-")
    F = R.field(name, Q)
    margin, bbox = 1, None
    if variant == "bbox":
        bbox = ((-2, -1, 0), (2, 1, 3))
    if variant == "isoplane":              # lattice values equal to iso exactly on a plane: v > iso puts them outside, t becomes 0 or 1
        F[:, :, 16 if name == "sphere" else 13] = 0.5
        margin = 1 if name == "sphere" else 0
    for m in ((0, 1) if not variant else (margin,)):
        ref = R.hierarchy(F, Q0, L, 0.5, m)
        assert np.array_equal(ref["final"], R.dense_cut_cells(F, 0.5)) and ref["final"].sum() > 0      # the premise: every cut cell is reached
        Fd = torch.from_numpy(F[None]).to(dev)
        kw = {} if bbox is None else dict(bbox=bbox)
        got = IS.extract_sparse_dev(IS.table_field(Fd), 1, Q0, L, thresh=0.5, margin=m, device=dev, **kw)
        want = _dense(Fd, 0.5, bbox)
        assert len(want[1]) > 100
        _assert_mesh(got, want)


@pytest.fixture(scope="module")
def model16(dev):
    """res16 hash-weight model, a seeded two-shape cloud, its applied-affine decoder grid and the dense 65^3 values (computed once)."""
    from shapeformer_amd import ops, synthetic, weights as W
    from shapeformer_amd.vqdif import VQDIF
    vq = VQDIF(W.make_state_dict(W.vqdif_spec(16)), res=16, device=dev)
    cloud = torch.from_numpy(synthetic.make_batch(7, 2, n_full=8192, n_partial=4096)["Xbd"]).to(dev)
    q = vq.quantize_cloud_dev(cloud)[0].clone()
    grid = vq.decoder_grid_cl(vq.get_code_cl(q), final_affine=True).clone()
    axis = torch.from_numpy(np.linspace(-1.0, 1.0, 65).astype(np.float32)).to(dev)
    dense = {s: ops.sdf_query_grid(axis, grid, vq.sdf_w, sigmoid=s).reshape(2, -1) for s in (False, True)}
    return dict(vq=vq, q=q, grid=grid, axis=axis, dense=dense)


@pytest.mark.parametrize("counts", [(1037, 1), (0, 70)])
@pytest.mark.parametrize("sigmoid", [False, True])
def test_keyed_query_equals_the_lattice_query_bitwise(dev, model16, counts, sigmoid):
    from shapeformer_amd import ops
    n3 = 65 ** 3
    rng = np.random.RandomState(11)
    keys = []
    for b, n in enumerate(counts):
        k = rng.choice(n3 - 2, size=n, replace=False) + 1
        if n >= 2:
            k[:2] = (0, n3 - 1)                 # the first and the last lattice point
        elif n == 1:
            k[0] = n3 - 1
        keys.append(np.sort(k).astype(np.int32))
    koff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    kd = torch.from_numpy(np.concatenate(keys)).to(dev)
    got = ops.sdf_query_keys(model16["axis"], kd, torch.from_numpy(koff).to(dev), model16["grid"], model16["vq"].sdf_w, sigmoid=sigmoid)
    want = torch.cat([model16["dense"][sigmoid][b][torch.from_numpy(keys[b]).long().to(dev)] for b in range(2)])
    assert got.shape == (sum(counts),) and torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_decoder_end_to_end(dev, model16):
    """decode_index_mesh == the reference's selection of the dense mesh of the dense decode of the same applied-affine grid."""
    vq, Q = model16["vq"], 65
    occ = model16["dense"][True].reshape(2, Q, Q, Q)
    iso = float(occ[:, ::4, ::4, ::4].median())            # hash weights: the field need not cross 0.5; the coarse lattice's median it does
    got = vq.decode_index_mesh(model16["q"], Q, coarse=17, margin=1, thresh=iso, sigmoid=True, return_levels=True)
    Fs = list(occ.cpu().numpy())
    refs = [R.hierarchy(F, 17, 2, iso, 1) for F in Fs]
    _assert_mesh(got[:4], _expect_selection(Fs, iso, [r["final"] for r in refs], _dense(occ, iso)))
    assert len(got[1]) > 100
    assert np.array_equal(got[4]["points"], np.array([r["points"] for r in refs]).T)
    assert got[4]["points"].sum() < 2 * Q ** 3


def test_callback_sparse_decode(dev, tmp_path):
    """VisShapeFormer(sparse_decode=True): every exported mesh is decode_index_mesh of its token set; eval/*.npz is written as before."""
    from test_plugin_gpu import _Items, _opt
    from shapeformer_amd import callbacks as CB, meshio, plugin as P
    model = P.instantiate_from_opt(P.get_opt(_opt())["pl_model_opt"])
    cb = P.instantiate_from_opt({"class": "shapeformer.models.shapeformer.shapeformer.VisShapeFormer", "kwargs": dict(
        end_tokens=[4096, 4096], top_k=100, top_p=0.4, depth=4, visual_indices=[0], sample_n=4, sample_max_step=12, decode_res=65,
        sparse_decode=True, sparse_coarse=17, data_dir=str(tmp_path))})
    assert cb.sparse_decode and cb.sparse_coarse == 17 and cb.sparse_margin == 1
    np.random.seed(0)
    out = cb.process(model, _Items(1))["0"]
    computed = np.load(tmp_path / "computed" / "0.npy", allow_pickle=True).item()
    sets = [(k, CB.filter_end_tokens(t, cb.end_tokens)) for k, t in cb._token_sets(computed)]
    sets = [(k, t) for k, t in sets if len(t)]
    dense = np.full((len(sets), 16 ** 3), int(computed["empty_index"]), np.int32)
    for j, (_, t) in enumerate(sets):
        dense[j, t[:, 0]] = t[:, 1]
    vq = model.representer.vqvae_model.core
    v, f, voff, toff = vq.decode_index_mesh(torch.from_numpy(dense.reshape(-1, 16, 16, 16)).to(vq.dev), 65, coarse=17, margin=1, thresh=0.5)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    exported = 0
    for j, (key, _) in enumerate(sets):
        vb, fb = v[voff[j]:voff[j + 1]], f[toff[j]:toff[j + 1]]
        if len(vb) < 10:
            assert key + "_mesh" not in out
            continue
        m = out[key + "_mesh"]
        assert np.array_equal(m["vert"], vb.astype(np.float64)) and np.array_equal(m["face"], fb)
        v2, f2 = meshio.read_ply(m["path"])
        assert np.array_equal(v2, m["vert"]) and np.array_equal(f2, fb)
        exported += 1
    assert exported > 0
    n_s = sum(1 for k in out if k.startswith("s") and k.endswith("_mesh"))
    ev = np.load(tmp_path / "eval" / "0.npz")
    assert n_s > 0 and sorted(ev.files) == sorted(["eval_pc"] + [f"recon_{i}" for i in range(n_s)]) and ev["eval_pc"].shape == (10 ** 5, 3)


def test_refusals_before_any_launch(dev, model16):
    from shapeformer_amd import _lib as L, iso_sparse as IS, ops
    lib = L.lib()
    E = L.SFMI_EINVAL
    buf = torch.zeros(4096, device=dev, dtype=torch.int32)
    p = L.ptr(buf)
    good, bad_rule, huge = (1, 5, 2, 17), (1, 5, 2, 18), (1, 646, 1, 1291)
    assert lib.sfmi_iso_sparse_workspace_bytes(1, 1291) == 0 and lib.sfmi_iso_sparse_workspace_bytes(1, 17) >= 4 * 4 * 154
    for lat in (bad_rule, huge, (1, 1, 4, 1), (1, 17, 0, 17), (0, 5, 2, 17)):
        assert lib.sfmi_iso_seed_i32(*lat, p, p, None) == E
        assert lib.sfmi_iso_popc_i32(p, p, *lat, None) == E
        assert lib.sfmi_iso_compact_i32(p, p, *lat, p, 1, None) == E
        assert lib.sfmi_iso_classify_f32(p, p, 1, 0, p, p, p, 8, 0.5, *lat, p, None) == E
        assert lib.sfmi_iso_carry_i32(p, p, 1, p, p, *lat, p, None) == E
        assert lib.sfmi_iso_refine_i32(p, p, p, 1, 0, 1, *lat, p, p, None) == E
        assert lib.sfmi_iso_mc_count_i32(p, p, p, 1, p, p, 8, *lat, p, p, None) == E
        assert lib.sfmi_iso_mc_emit_f32(p, p, p, 1, p, p, 8, p, p, p, 0.5, p, p, p, p, *lat, -1, -1, -1, 1, 1, 1, p, p, None) == E
    for margin in (2, -1):
        assert lib.sfmi_iso_refine_i32(p, p, p, 1, 0, margin, *good, p, p, None) == E
    assert lib.sfmi_iso_refine_i32(p, p, p, 1, 2, 1, *good, p, p, None) == E            # no level below the last
    assert lib.sfmi_iso_seed_i32(*good, None, p, None) == E and lib.sfmi_iso_seed_i32(*good, p, None, None) == E
    assert lib.sfmi_iso_popc_i32(None, p, *good, None) == E
    assert lib.sfmi_iso_compact_i32(p, None, *good, p, 1, None) == E and lib.sfmi_iso_compact_i32(p, p, *good, None, 1, None) == E
    assert lib.sfmi_iso_classify_f32(p, p, 1, 0, p, p, None, 8, 0.5, *good, p, None) == E
    assert lib.sfmi_iso_refine_i32(None, p, p, 1, 0, 1, *good, p, p, None) == E
    assert lib.sfmi_iso_carry_i32(p, p, 1, None, p, *good, p, None) == E and lib.sfmi_iso_carry_i32(p, p, 1, p, p, *good, None, None) == E
    assert lib.sfmi_iso_mc_count_i32(p, p, p, 1, p, p, 8, *good, None, p, None) == E
    assert lib.sfmi_iso_carry_apply_f32(None, p, 1, p, p, 1, None) == E and lib.sfmi_iso_carry_apply_f32(p, p, -1, p, p, 1, None) == E
    assert lib.sfmi_iso_select_i32(None, p, 1, p, 1, None) == E and lib.sfmi_iso_select_i32(p, p, 1, None, 1, None) == E
    assert lib.sfmi_iso_mc_emit_f32(p, p, p, 1, p, p, 8, p, p, p, 0.5, p, p, p, p, *good, -1, -1, -1, 1, 1, 1, None, p, None) == E
    torch.cuda.synchronize()
    assert int(buf.abs().sum()) == 0                                                     # nothing was launched on the buffer
    g, w, ax = model16["grid"], model16["vq"].sdf_w, model16["axis"]
    assert lib.sfmi_sdf_query_keys_f32(L.ptr(ax), 1291, p, p, 4, L.ptr(g), L.ptr(w), p, 2, 64, 0, None) == E
    assert lib.sfmi_sdf_query_keys_f32(L.ptr(ax), 65, None, p, 4, L.ptr(g), L.ptr(w), p, 2, 64, 0, None) == E
    assert lib.sfmi_sdf_query_keys_f32(L.ptr(ax), 65, p, None, 4, L.ptr(g), L.ptr(w), p, 2, 64, 0, None) == E
    field = IS.table_field(torch.zeros(1, 17, 17, 17, device=dev))
    with pytest.raises(L.SfmiError, match="margin"):
        IS.extract_sparse_dev(field, 1, 5, 2, margin=2, device=dev)
    with pytest.raises(L.SfmiError):
        IS.extract_sparse_dev(field, 1, 646, 1, device=dev)                              # Q = 1291: Q^3 >= 2^31
    with pytest.raises(L.SfmiError, match="nearest valid res = 129"):
        model16["vq"].decode_index_mesh(model16["q"], 128)
    with pytest.raises(L.SfmiError, match="margin"):
        model16["vq"].decode_index_mesh(model16["q"], 65, coarse=17, margin=2)
    with pytest.raises(L.SfmiError):
        model16["vq"].decode_index_mesh(model16["q"], 1291, coarse=646)
