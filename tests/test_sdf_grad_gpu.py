"""GPU tests of the gradient kernel (sfmi_sdf_query_grad_f32): value and d value / d point of the fused implicit
decoder against the float64 statement of tests/sdf_grad_ref.py, its ragged form, the Newton-step and normal epilogues, and the
meshing routes that hang off them.

The gradient gate: a point whose float64 minimum |pre-activation| is below 2e-5 is excluded (a ReLU there may legitimately fall on
the other side in float32; at most 2 % of the points may be); on the others the kernel's max abs error against float64 is at most
4 x E_ref, E_ref being the max abs error of the oracle's own float32 autograd against float64 on the same points (the kernel sums
in another order and runs a second 16-matrix chain)."""
import os

import numpy as np
import pytest
import torch

import sdf_grad_ref as R

pytestmark = pytest.mark.gpu

EXCLUDE_BELOW, EXCLUDE_CAP, GATE = 2e-5, 0.02, 4.0


@pytest.fixture(scope="module")
def packs(dev, vq16_sd):
    from shapeformer_amd import ops
    return (torch.from_numpy(ops.sdf_pack_weights(vq16_sd)).to(dev), torch.from_numpy(ops.sdf_pack_weights_grad(vq16_sd)).to(dev))


def _cl(grid, dev):
    return grid.permute(0, 2, 3, 4, 1).contiguous().to(dev)


@pytest.fixture(scope="module")
def case(dev, vq16_sd, packs):
    """B = 2, N = 4096 cell-interior points, seed 1: float64 truth, the oracle's float32 autograd, the kernel's outputs."""
    from shapeformer_amd import ops
    grid, x = R.rand_grid(2, 1), R.interior_points(2, 4096, 1)
    v64, g64, margin = R.value_grad(vq16_sd, grid, x)
    _, g32 = R.oracle_grad_f32(vq16_sd, grid, x)
    grid_cl = _cl(grid, dev)
    val, grad = ops.sdf_query_grad(x.to(dev), grid_cl, packs[1])
    return dict(grid=grid, grid_cl=grid_cl, x=x, v64=v64, g64=g64, g32=g32, margin=margin, val=val, grad=grad)


def _gate(name, got, g64, g32, margin):
    keep = margin >= EXCLUDE_BELOW
    share = 1.0 - float(keep.double().mean())
    e_ref = float((g32.double() - g64)[keep].abs().max())
    err = float((got.double() - g64)[keep].abs().max())
    print(f"{name}: excluded {100 * share:.2f} %, max |grad| {float(g64.abs().max()):.1f}, E_ref {e_ref:.3e}, kernel error {err:.3e}, "
          f"ratio {err / e_ref:.2f}")
    assert share <= EXCLUDE_CAP
    assert err <= GATE * e_ref, (err, e_ref)
    return err / e_ref


@pytest.mark.parametrize("B,N", [(1, 1), (2, 31), (1, 32), (3, 1000)])
def test_values_are_the_value_kernels_bit_for_bit(dev, packs, B, N):
    from shapeformer_amd import ops
    grid_cl = _cl(R.rand_grid(B, 1), dev)
    g = torch.Generator().manual_seed(7 + N)
    xyz = torch.rand(B, N, 3, generator=g) * 2.6 - 1.3            # clamped axes included
    xyz[:, 0] = torch.tensor([1.0, -1.0, 0.0])
    xyz = xyz.to(dev)
    val, grad = ops.sdf_query_grad(xyz, grid_cl, packs[1])
    assert val.shape == (B, N, 1) and grad.shape == (B, N, 3) and bool(torch.isfinite(grad).all())
    assert torch.equal(val, ops.sdf_query(xyz, grid_cl, packs[0]))


def test_gradient_against_float64(case):
    assert case["grad"].shape == (2, 4096, 3)
    _gate("interior points", case["grad"].cpu(), case["g64"], case["g32"], case["margin"])
    assert float((case["val"].cpu()[..., 0].double() - case["v64"]).abs().max()) < 2e-4 + 1e-4 * float(case["v64"].abs().max())


def test_clamped_axes(dev, vq16_sd, packs, case):
    """Outside the box on an axis the gather is constant along it: that component is the fc_p term alone."""
    from shapeformer_amd import ops
    x = R.clamped_points(3)[None]
    grid = case["grid"][:1]
    _, g64, margin = R.value_grad(vq16_sd, grid, x)
    _, g32 = R.oracle_grad_f32(vq16_sd, grid, x)
    _, grad = ops.sdf_query_grad(x.to(dev), case["grid_cl"][:1], packs[1])
    _gate("clamped axes", grad.cpu(), g64, g32, margin)
    # (1.2, 0, 0): the x component must be the fc_p term alone, far below the interior slopes the gather contributes
    assert abs(float(grad[0, 0, 0])) < 0.1 * float(g64.abs().max())


def test_ragged_form_equals_the_per_shape_dense_calls(dev, packs):
    from shapeformer_amd import ops
    grid_cl = _cl(R.rand_grid(3, 4), dev)
    x = (torch.rand(70, 3, generator=torch.Generator().manual_seed(11)) * 2.4 - 1.2).to(dev)
    off = torch.tensor([0, 5, 5, 70], dtype=torch.int32, device=dev)      # an empty shape; the tile 0..31 straddles shapes 0 and 2
    val, grad = ops.sdf_query_grad(x, grid_cl, packs[1], off=off)
    assert val.shape == (70,) and grad.shape == (70, 3)
    for b, (lo, hi) in ((0, (0, 5)), (2, (5, 70))):
        v1, g1 = ops.sdf_query_grad(x[None, lo:hi], grid_cl[b:b + 1], packs[1])
        assert torch.equal(val[lo:hi], v1[0, :, 0]) and torch.equal(grad[lo:hi], g1[0])
    nrm = ops.sdf_normals(x, grid_cl, packs[1], off=off)
    x1, v1 = ops.sdf_refine_step(x, grid_cl, packs[1], 0.25, 0.01, off=off)
    assert torch.equal(v1, val)
    g = grad.double()
    g2 = (g * g).sum(-1, keepdim=True)
    assert float((nrm.double() + g / g2.sqrt()).abs().max()) < 1e-6
    want = R.newton_step(x.double(), val.double(), g, 0.25, 0.01)
    assert float((x1.double() - want).abs().max()) < 1e-6 and float((x1 - x).norm(dim=-1).max()) <= 0.01 * (1 + 1e-5)


def test_normal_points_out_of_the_occupied_side(dev, packs, case):
    """Occupancy rises inward, so the logit falls along the normal -g/|g|."""
    from shapeformer_amd import ops
    x = case["x"].to(dev)
    nrm = ops.sdf_normals(x, case["grid_cl"], packs[1])
    ln = nrm.norm(dim=-1)
    assert bool((((ln - 1).abs() < 1e-5) | (ln == 0)).all())
    v1 = ops.sdf_query(x + 1e-3 * nrm, case["grid_cl"], packs[0])
    share = float((v1 < case["val"]).double().mean())
    print(f"logit falls along the normal at {100 * share:.2f} % of the points")
    assert share >= 0.98


def test_c_abi_refusals(dev, packs):
    from shapeformer_amd import _lib as L
    lib, E = L.lib(), L.SFMI_EINVAL
    buf = torch.zeros(4096, device=dev)
    off = torch.tensor([0, 8], dtype=torch.int32, device=dev)
    p, o, w = L.ptr(buf), L.ptr(off), L.ptr(packs[1])
    ok = lambda **k: dict(dict(xyz=p, poff=o, N=8, grid=p, w=w, val=p, vc=8, grad=p, gc=24, xo=None, xc=0, no=None, nc=0, B=1, G=2), **k)
    call = lambda a: lib.sfmi_sdf_query_grad_f32(a["xyz"], a["poff"], a["N"], a["grid"], a["w"], a["val"], a["vc"], a["grad"], a["gc"], 0.0, 0.0,
                                                 a["xo"], a["xc"], a["no"], a["nc"], a["B"], a["G"], None)
    for bad in (dict(xyz=None), dict(poff=None), dict(grid=None), dict(w=None), dict(val=None), dict(grad=None), dict(N=0), dict(N=-1),
                dict(N=1 << 31), dict(G=1), dict(B=0), dict(vc=7), dict(gc=23), dict(xo=p, xc=23), dict(no=p, nc=23)):
        assert call(ok(**bad)) == E, bad


@pytest.fixture(scope="module")
def decoded(dev, vq16_sd):
    """The fixture field: codes of a synthetic cloud, the 33^3 lattice, marching cubes at the median logit."""
    from shapeformer_amd import mcubes, synthetic
    from shapeformer_amd.vqdif import VQDIF
    vq = VQDIF(vq16_sd, res=16, device=dev)
    Xbd = torch.from_numpy(synthetic.make_shape(3, 8192, 4096)["Xbd"])[None].to(dev)
    q = vq.quantize_cloud_dev(Xbd)[0].clone()
    Q = 33
    logits = vq.decode_index(q, grid_Q=Q)["logits"].clone()
    level = float(logits.median())
    v, f, voff, toff = mcubes.marching_cubes_dev(logits.reshape(1, Q, Q, Q), level)
    return dict(vq=vq, q=q, Q=Q, level=level, v=v, f=f, voff=voff, toff=toff)


def test_refinement_on_a_decoded_field(dev, decoded):
    from shapeformer_amd import ops
    vq, Q, level, v, voff = decoded["vq"], decoded["Q"], decoded["level"], decoded["v"], decoded["voff"]
    assert v.shape[0] > 1000
    grid = vq.decoder_grid_cl(vq.get_code_cl(decoded["q"]))
    thresh = 1.0 / (1.0 + np.exp(-level))                          # refine_mesh_dev works at log(thresh / (1 - thresh)) = level
    steps, max_step = 2, 1.0 / (Q - 1)
    v2 = vq.refine_mesh_dev(grid, v, voff, thresh=thresh, steps=steps, max_step=max_step)
    res = lambda p: float((ops.sdf_query(p[None], grid, vq.sdf_w)[0, :, 0] - level).abs().median())
    before, after = res(v), res(v2)
    print(f"median |logit - level|: {before:.3e} -> {after:.3e} (1/{before / max(after, 1e-30):.0f})")
    assert after <= before / 20
    assert v2.shape == v.shape and float((v2 - v).norm(dim=-1).max()) <= steps * max_step * (1 + 1e-5)      # f32 rounding of the clamp
    with pytest.raises(ValueError, match="max_step"):
        vq.refine_mesh_dev(grid, v, voff, thresh=thresh)
    nrm = vq.vertex_normals_dev(grid, v2, voff)
    ln = nrm.norm(dim=-1)
    assert nrm.shape == v2.shape and bool((((ln - 1).abs() <= 1e-5) | (ln == 0)).all()) and float((ln > 0).double().mean()) > 0.99


def test_decode_index_mesh_keywords(dev, decoded):
    vq, q = decoded["vq"], decoded["q"]
    a = vq.decode_index_mesh(q, 65)
    b = vq.decode_index_mesh(q, 65, refine_steps=0, normals=False)
    assert len(a) == len(b) == 4 and all(torch.equal(torch.as_tensor(x), torch.as_tensor(y)) for x, y in zip(a, b))
    c = vq.decode_index_mesh(q, 65, refine_steps=2, normals=True)
    assert len(c) == 5 and torch.equal(c[1], a[1]) and np.array_equal(c[2], a[2]) and np.array_equal(c[3], a[3])     # faces, offsets
    assert c[0].shape == a[0].shape and c[4].shape == a[0].shape
    if len(a[0]):
        assert float((c[0] - a[0]).norm(dim=-1).max()) <= 2 * (1.0 / 64) * (1 + 1e-5)
        grid = vq.decoder_grid_cl(vq.get_code_cl(q))
        assert torch.equal(c[4], vq.vertex_normals_dev(grid, c[0], c[2]))
    out = vq.decode_index_grad(q, decoded["v"][None, :100])
    assert out["logits"].shape == (1, 100, 1) and out["grad"].shape == (1, 100, 3)
    assert torch.equal(out["logits"], vq.decode_index(q, decoded["v"][None, :100])["logits"])


def test_sparse_recon_callback_refines_and_writes_normals(dev, tmp_path, monkeypatch):
    """VisSparseRecon3D on the demo_ds fixture: with refine_steps / vertex_normals the PLY carries unit normals; with the defaults the
    files are what they always were (positions and faces of the marching-cubes mesh of the stored logits, the same `computed` keys)."""
    from shapeformer_amd import mcubes, meshio, ops, plugin as P
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ds_dir = os.path.join(gold, "demo_ds")
    opt = P.get_opt(os.path.join(ds_dir, "demo_vqdif.yaml"))
    monkeypatch.chdir(ds_dir)
    model = P.instantiate_from_opt(opt["pl_model_opt"])
    dm = P.instantiate_from_opt(opt["datamodule_opt"])
    dm.setup("test")
    outs = {}
    for name, extra in (("plain", {}), ("smooth", dict(refine_steps=2, vertex_normals=True))):
        cbo = dict(opt["callbacks"]["vis_recon"], kwargs=dict(opt["callbacks"]["vis_recon"]["kwargs"], data_dir=str(tmp_path / name), **extra))
        np.random.seed(0)
        outs[name] = P.instantiate_from_opt(cbo).process(model, dm.test_set)
    Q = opt["callbacks"]["vis_recon"]["kwargs"]["decoder_resolution"]
    meshes = 0
    for i in sorted(outs["plain"]):
        comp = np.load(tmp_path / "plain" / "computed" / f"{i}.npy", allow_pickle=True).item()
        assert set(comp) == {"logits", "quant_ind", "sparse", "grid_mask", "batch"}
        occ = ops.sigmoid(torch.from_numpy(comp["logits"]).to(dev))[..., 0]
        v, f = mcubes.marching_cubes_dev(occ[:1].reshape(1, Q, Q, Q), 0.5)[:2]
        v, f = v.cpu().numpy().astype(np.float64), f.cpu().numpy().astype(int)
        m0, m1 = outs["plain"][i]["recon_mesh"], outs["smooth"][i]["recon_mesh"]
        assert np.array_equal(m0["vert"], v) and np.array_equal(m0["face"], f) and "normal" not in m0
        meshio.write_mesh(str(tmp_path / "w"), v, f, "want")
        assert open(tmp_path / "plain" / "meshes" / f"{i}.ply", "rb").read() == open(tmp_path / "w" / "meshes" / "want.ply", "rb").read()
        assert b"property double nx" not in open(tmp_path / "plain" / "meshes" / f"{i}.ply", "rb").read()
        if len(v) < 10:
            continue
        meshes += 1
        v2, f2, n2 = meshio.read_ply(outs["smooth"][i]["mesh_path"], with_normals=True)
        assert np.array_equal(f2, f) and np.array_equal(v2, m1["vert"]) and np.array_equal(n2, m1["normal"])
        assert 0 < np.abs(v2 - v).max() <= 2 * (1.0 / (Q - 1)) * (1 + 1e-5)
        ln = np.linalg.norm(n2, axis=1)
        assert np.all((np.abs(ln - 1) <= 1e-5) | (ln == 0)) and np.mean(ln > 0) > 0.99
    assert meshes > 0


@pytest.mark.parametrize("route", ["dense", "sparse"])
def test_shapeformer_callback_refine_decimate_normals(dev, tmp_path, route):
    """VisShapeFormer(refine_steps=2, vertex_normals=True, decimate_face=n) on both meshing routes: extract -> refine -> decimate ->
    normals at the vertices that are written; without the keywords the meshes are those of the unchanged route, and the files carry
    no normals.  The model setup of test_simplify_gpu.py's callback test."""
    from test_plugin_gpu import _Items, _opt
    from shapeformer_amd import meshio, plugin as P
    model = P.instantiate_from_opt(P.get_opt(_opt())["pl_model_opt"])
    kw = dict(end_tokens=[4096, 4096], top_k=100, top_p=0.4, depth=4, visual_indices=[0], sample_n=2, sample_max_step=12)
    kw.update(dict(decode_res=32) if route == "dense" else dict(decode_res=65, sparse_decode=True, sparse_coarse=17))
    Q = kw["decode_res"]
    name = "shapeformer.models.shapeformer.shapeformer.VisShapeFormer"
    mk = lambda tag, **extra: P.instantiate_from_opt({"class": name, "kwargs": dict(kw, data_dir=str(tmp_path / tag), **extra)})
    plain, smooth, both = mk("plain"), mk("smooth", refine_steps=2, vertex_normals=True), mk("both", refine_steps=2, vertex_normals=True,
                                                                                              decimate_face=300)
    assert plain.refine_steps == 0 and not plain.vertex_normals and smooth.refine_steps == 2 and smooth.vertex_normals
    plain.process(model, _Items(1))
    computed = np.load(tmp_path / "plain" / "computed" / "0.npy", allow_pickle=True).item()
    outs = {}
    for tag, cb in (("plain", plain), ("smooth", smooth), ("both", both)):
        cb.pl_module = model
        np.random.seed(0)
        outs[tag] = cb.visualize_batch(computed, input_name="0", data_dir=str(tmp_path / tag))
    keys = [k for k in outs["plain"] if k.endswith("_mesh")]
    assert keys and all(sorted(k for k in o if k.endswith("_mesh")) == sorted(keys) for o in outs.values())
    unit = lambda n: bool(np.all((np.abs(np.linalg.norm(n, axis=1) - 1) <= 1e-5) | (np.linalg.norm(n, axis=1) == 0)))
    for k in keys:
        m0, m1, m2 = outs["plain"][k], outs["smooth"][k], outs["both"][k]
        assert "normal" not in m0 and b"property double nx" not in open(m0["path"], "rb").read()
        assert np.array_equal(m1["face"], m0["face"]) and m1["vert"].shape == m0["vert"].shape
        assert 0 < np.linalg.norm(m1["vert"] - m0["vert"], axis=1).max() <= 2 * (1.0 / (Q - 1)) * (1 + 1e-5)
        for m in (m1, m2):
            v, f, n = meshio.read_ply(m["path"], with_normals=True)
            assert np.array_equal(v, m["vert"]) and np.array_equal(f, m["face"]) and np.array_equal(n, m["normal"])
            assert n.shape == v.shape and unit(n) and np.mean(np.linalg.norm(n, axis=1) > 0) > 0.99
        assert len(m2["face"]) <= 300
    e1, e2 = np.load(tmp_path / "smooth" / "eval" / "0.npz"), np.load(tmp_path / "both" / "eval" / "0.npz")
    assert sorted(e1.files) == sorted(e2.files) and all(np.array_equal(e1[k], e2[k]) for k in e1.files)      # sampled from the refined, undecimated mesh
