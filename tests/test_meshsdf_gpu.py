"""GPU: mesh signed distance and occupancy (csrc/meshsdf.hip, shapeformer_amd/meshsdf.py) against the f64 restatement in
tests/meshsdf_ref.py (Ericson closest point, van Oosterom-Strackee solid angle, brute force), analytic shapes, and the
marching-cubes round trip; then the store builder end to end into one VQDIF training step."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import meshsdf_ref as R   # noqa: E402
from test_mcubes_cpu import _sphere, _torus   # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-7


def _t(x, dev, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)


def _soup(rs, n_tri, scale=1.0):
    """random triangles on a 1/64 lattice (exact in f32) plus degenerate ones: repeated vertex, collinear (exact midpoint),
    a point, and a duplicate face."""
    v = rs.randint(-64, 65, (3 * n_tri, 3)).astype(np.float64) / 64 * scale
    f = np.arange(3 * n_tri).reshape(-1, 3)
    k = n_tri // 8
    v[3 * np.arange(k) + 1] = v[3 * np.arange(k)]                                  # repeated vertex
    j = np.arange(k, 2 * k)
    v[3 * j + 2] = (v[3 * j] + v[3 * j + 1]) / 2                                    # collinear
    j = np.arange(2 * k, 2 * k + 3)
    v[3 * j + 1] = v[3 * j + 2] = v[3 * j]                                          # points
    f = np.concatenate([f, f[-5:]])                                                # duplicate faces (higher index never wins)
    return v.astype(np.float32), f


def _queries(rs, v, n):
    near = v[rs.randint(0, len(v), n // 2)] + rs.randn(n // 2, 3).astype(np.float32) * 0.01
    far = rs.uniform(-2, 2, (n - n // 2, 3)).astype(np.float32)
    return np.concatenate([near, far]).astype(np.float32)


def _check_against_oracle(q, v, f, S, I, C, W):
    o = R.brute(q, v.astype(np.float64), f)
    d = np.abs(S.astype(np.float64))
    t = np.sqrt(o["d2"])
    assert (np.abs(d - t) <= RTOL * t + ATOL).all(), np.abs(d - t).max()
    # the face: the oracle's wherever its best two faces are apart by more than the tolerance
    sep = np.sqrt(o["d2_second"]) - t > RTOL * t + ATOL
    assert (I[sep] == o["I"][sep]).all()
    # C lies on face I (its f64 closest point to C is C) and |q - C| is the distance
    Cf = C.astype(np.float64)
    vv = v.astype(np.float64)
    on = R.closest_on_triangle(Cf, vv[f[I, 0]], vv[f[I, 1]], vv[f[I, 2]])
    assert np.abs(on - Cf).max() < 1e-5
    dq = np.sqrt(((q.astype(np.float64) - Cf) ** 2).sum(1))
    assert (np.abs(dq - d) <= 1e-6 * d + 1e-6).all()
    assert np.abs(W - o["W"]).max() < 1e-4
    return o


def test_random_soups_against_f64_oracle(dev):
    from shapeformer_amd import meshsdf as MS
    rs = np.random.RandomState(0)
    for n_tri, n_q in [(40, 700), (333, 1500)]:
        v, f = _soup(rs, n_tri, scale=0.5)             # |coordinates| <= 0.5: 1e-7 absolute is about one f32 ulp of them
        q = _queries(rs, v, n_q)
        S, I, C, W, st = MS.signed_distance_dev(_t(q, dev), _t(v, dev), _t(f, dev, torch.int32), return_winding=True)
        assert st.cpu().tolist() == [0]
        S, I, C, W = S.cpu().numpy(), I.cpu().numpy(), C.cpu().numpy(), W.cpu().numpy()
        assert np.isfinite(S).all() and np.isfinite(C).all() and np.isfinite(W).all()
        _check_against_oracle(q, v, f, S, I, C, W)
        # |q - C|^2 in f32, direct form, is d2 bit for bit
        dq = q - C
        d2 = np.fmax(0, (dq[:, 0] * dq[:, 0] + dq[:, 1] * dq[:, 1] + dq[:, 2] * dq[:, 2]))
        assert np.abs(np.sqrt(d2) - np.abs(S)).max() <= 1e-6 * np.abs(S).max() + 1e-7


def test_closed_meshes_cube_and_icosphere(dev):
    from shapeformer_amd import meshsdf as MS
    rs = np.random.RandomState(1)
    q = np.concatenate([rs.uniform(-2, 2, (3000, 3)), rs.uniform(-1, 1, (1000, 3))]).astype(np.float32)
    S, I, C, st = MS.signed_distance_dev(_t(q, dev), _t(R.CUBE_V, dev), _t(R.CUBE_F, dev, torch.int32))
    S = S.cpu().numpy().astype(np.float64)
    box = R.box_sdf(q.astype(np.float64))
    assert np.abs(S - box).max() < 1e-6
    # icosphere: S ~ |p| - r within the chord error; sign exact away from the surface
    v, f = R.icosphere(3, r=0.7)
    chord = 0.7 * (1 - np.cos(np.max(np.arccos(np.clip((v[f[:, 0]] * v[f[:, 1]]).sum(1) / 0.49, -1, 1)))))
    q = rs.uniform(-1, 1, (4000, 3)).astype(np.float32)
    S, I, C, W, st = MS.signed_distance_dev(_t(q, dev), _t(v, dev), _t(f, dev, torch.int32), return_winding=True)
    S, W = S.cpu().numpy().astype(np.float64), W.cpu().numpy()
    ana = np.linalg.norm(q.astype(np.float64), axis=1) - 0.7
    assert np.abs(S - ana).max() <= chord + 1e-6
    o = R.brute(q, v.astype(np.float32).astype(np.float64), f)
    far = np.abs(o["S"]) > 1e-4
    assert (np.sign(S[far]) == np.sign(o["S"][far])).all()
    assert (np.abs(np.abs(W[far]) - np.round(np.abs(W[far]))) < 1e-3).all()


def test_open_meshes_fractional_winding(dev):
    from shapeformer_amd import meshsdf as MS
    rs = np.random.RandomState(2)
    v, f = R.icosphere(2, r=0.6)
    keep = v[f].mean(1)[:, 2] > 0                                                   # hemisphere
    f = f[keep]
    tri_v, tri_f = np.array([[-0.5, -0.4, 0.1], [0.6, -0.3, 0.0], [0.0, 0.7, -0.1]]), np.array([[0, 1, 2]])
    for vv, ff in [(v, f), (tri_v, tri_f)]:
        vv = vv.astype(np.float32)
        q = rs.uniform(-1, 1, (2000, 3)).astype(np.float32)
        S, I, C, W, st = MS.signed_distance_dev(_t(q, dev), _t(vv, dev), _t(ff, dev, torch.int32), return_winding=True)
        _check_against_oracle(q, vv, ff, S.cpu().numpy(), I.cpu().numpy(), C.cpu().numpy(), W.cpu().numpy())


def test_ties_lowest_face_wins(dev):
    from shapeformer_amd import meshsdf as MS
    # two mirror-image triangles at x = +-1; queries on the plane x = 0 are equidistant (exactly, in f32)
    v = np.array([[1, -1, -1], [1, 1, -1], [1, 0, 1], [-1, -1, -1], [-1, 1, -1], [-1, 0, 1]], np.float32)
    q = np.array([[0, 0, 0], [0, 0.25, -0.5], [0, 3, 3]], np.float32)
    for f in (np.array([[0, 1, 2], [3, 4, 5]]), np.array([[3, 4, 5], [0, 1, 2]])):
        S, I, C, st = MS.signed_distance_dev(_t(q, dev), _t(v, dev), _t(f, dev, torch.int32))
        assert I.cpu().tolist() == [0, 0, 0]
        assert np.allclose(C.cpu().numpy()[:, 0], v[f[0, 0], 0])


def test_determinism_batch_and_split(dev):
    from shapeformer_amd import meshsdf as MS
    rs = np.random.RandomState(3)
    meshes = [_soup(rs, n) for n in (50, 400, 90)]
    qs = [_queries(rs, m[0], n) for m, n in zip(meshes, (3000, 500, 1200))]
    v = np.concatenate([m[0] for m in meshes])
    f = np.concatenate([m[1] for m in meshes])
    voff = np.concatenate([[0], np.cumsum([len(m[0]) for m in meshes])])
    toff = np.concatenate([[0], np.cumsum([len(m[1]) for m in meshes])])
    qoff = np.concatenate([[0], np.cumsum([len(x) for x in qs])])
    args = (_t(np.concatenate(qs), dev), _t(v, dev), _t(f, dev, torch.int32), qoff, voff, toff)
    a = MS.signed_distance_dev(*args, return_winding=True)
    b = MS.signed_distance_dev(*args, return_winding=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    S, I, C, W, st = (x.cpu().numpy() for x in a)
    for k in range(3):
        s1, i1, c1, w1, st1 = (x.cpu().numpy() for x in MS.signed_distance_dev(
            _t(qs[k], dev), _t(meshes[k][0], dev), _t(meshes[k][1], dev, torch.int32), return_winding=True))
        sl = slice(qoff[k], qoff[k + 1])
        assert np.array_equal(i1, I[sl]) and np.array_equal(c1, C[sl]) and np.array_equal(np.abs(s1), np.abs(S[sl]))
        assert np.array_equal(np.sign(s1), np.sign(S[sl])) and np.abs(w1 - W[sl]).max() < 1e-5
    # a few queries against many faces (split into many chunks) == the same queries against the faces in one chunk: the
    # chunking depends on the query count, so compare 100 queries alone against the same 100 inside 60000 queries
    v, f = _soup(rs, 12000)
    q = _queries(rs, v, 100)
    big = np.concatenate([q, rs.uniform(-1, 1, (60000, 3)).astype(np.float32)])
    s1, i1, c1, _ = MS.signed_distance_dev(_t(q, dev), _t(v, dev), _t(f, dev, torch.int32))
    s2, i2, c2, _ = MS.signed_distance_dev(_t(big, dev), _t(v, dev), _t(f, dev, torch.int32))
    assert torch.equal(s1.abs(), s2[:100].abs()) and torch.equal(i1, i2[:100]) and torch.equal(c1, c2[:100])


def test_status_codes(dev):
    from shapeformer_amd import _lib as L
    from shapeformer_amd import meshsdf as MS
    rs = np.random.RandomState(4)
    v0, f0 = R.CUBE_V.astype(np.float32), R.CUBE_F.copy()
    f_bad = R.CUBE_F.copy()
    f_bad[5, 1] = 8                                                                 # outside the 8 vertices of its shape
    v = np.concatenate([v0, v0, v0])
    f = np.concatenate([f0, f_bad, f0])
    voff, toff = np.array([0, 8, 16, 24]), np.array([0, 12, 24, 36])
    q = rs.uniform(-2, 2, (300, 3)).astype(np.float32)
    qoff = np.array([0, 100, 200, 300])
    S, I, C, W, st = MS.signed_distance_dev(_t(q, dev), _t(v, dev), _t(f, dev, torch.int32), qoff, voff, toff, return_winding=True)
    assert st.cpu().tolist() == [0, MS.STATUS_BAD_INDEX, 0]
    S, I, C, W = S.cpu().numpy(), I.cpu().numpy(), C.cpu().numpy(), W.cpu().numpy()
    assert np.isnan(S[100:200]).all() and (I[100:200] == -1).all() and np.isnan(C[100:200]).all() and (W[100:200] == 0).all()
    box = R.box_sdf(q.astype(np.float64))
    assert np.abs(S[:100] - box[:100]).max() < 1e-6 and np.abs(S[200:] - box[200:]).max() < 1e-6
    occ, st = MS.mesh_occupancy_dev(_t(v, dev), _t(f, dev, torch.int32), voff, toff, grid_dim=8, return_status=True)
    assert st.cpu().tolist() == [0, 2, 0] and occ[1].sum().item() == 0 and occ[0].sum().item() > 0
    # an empty shape through the C ABI (the Python layer refuses queries against no faces): status 1, NaN / -1 / 0
    lib = L.lib()
    vv, ff = _t(np.concatenate([v0, v0]), dev), _t(f0, dev, torch.int32)
    qq = _t(q[:200], dev)
    offs = [torch.from_numpy(np.array(x, np.int64)).to(dev) for x in ([0, 100, 200], [0, 8, 16], [0, 0, 12])]
    S = torch.empty(200, device=dev)
    I = torch.empty(200, device=dev, dtype=torch.int32)
    W = torch.empty(200, device=dev)
    st = torch.empty(2, device=dev, dtype=torch.int32)
    ws = torch.empty(int(lib.sfmi_mesh_sdf_workspace_bytes(2, 200, 12)), device=dev, dtype=torch.uint8)
    L.check(lib.sfmi_mesh_sdf_f32(L.ptr(qq), L.ptr(offs[0]), L.ptr(vv), L.ptr(ff), L.ptr(offs[1]), L.ptr(offs[2]), 2, 200, 12, L.ptr(S),
                                  L.ptr(I), None, L.ptr(W), L.ptr(st), L.ptr(ws), L.stream_ptr()), "sfmi_mesh_sdf_f32")
    assert st.cpu().tolist() == [MS.STATUS_NO_FACES, 0]
    S, I, W = S.cpu().numpy(), I.cpu().numpy(), W.cpu().numpy()
    assert np.isnan(S[:100]).all() and (I[:100] == -1).all() and (W[:100] == 0).all()
    assert np.abs(S[100:] - box[100:200]).max() < 1e-6


def test_marching_cubes_round_trip(dev):
    from shapeformer_amd import mcubes, meshsdf as MS
    from shapeformer_amd.data import make_grid
    G = 64
    fields = np.stack([_sphere(G), _torus(G)]).astype(np.float32)
    v, f, voff, toff = mcubes.marching_cubes_dev(_t(fields, dev), 0.5)
    occ, st = MS.mesh_occupancy_dev(v, f, voff, toff, grid_dim=G, return_status=True)
    assert st.cpu().tolist() == [0, 0]
    occ = occ.cpu().numpy()
    want = fields >= 0.5
    step = 2 / (G - 1)
    X = make_grid([-1, -1, -1.], [1., 1, 1], [G] * 3)
    d = np.stack([np.abs(np.linalg.norm(X, axis=1) - 0.6),
                  np.abs(np.sqrt((np.sqrt(X[:, 0] ** 2 + X[:, 1] ** 2) - 0.55) ** 2 + X[:, 2] ** 2) - 0.22)])
    for b in range(2):
        diff = occ[b].reshape(-1) != want[b].reshape(-1)
        assert diff.mean() < 0.01, diff.mean()
        assert (d[b][diff] <= step).all()
    # the lattice the kernel generates is data.make_grid's: the signed distance of the explicit lattice has the same sign
    S, _, _, _ = MS.signed_distance_dev(_t(X.astype(np.float32), dev), v[:int(voff[1])], f[:int(toff[1])])
    assert np.array_equal((S.cpu().numpy() < 0), occ[0].reshape(-1).astype(bool))


def test_sdf_sampling_dev(dev):
    from shapeformer_amd import meshsdf as MS
    v, f = R.icosphere(3, r=0.6)
    vv, ff = _t(v, dev), _t(f, dev, torch.int32)
    vo, to = np.array([0, len(v)]), np.array([0, len(f)])
    n = 20000
    Xbd, Xtg, Ytg = MS.sdf_sampling_dev(vv, ff, vo, to, sample_N=n, seed=5)
    assert Xbd.dtype == Xtg.dtype == Ytg.dtype == torch.float16
    assert Xbd.shape == (1, n, 3) and Xtg.shape == (1, n, 3) and Ytg.shape == (1, n)
    X, Y = Xtg[0].float().cpu().numpy(), Ytg[0].float().cpu().numpy()
    assert np.abs(X).max() <= np.float16(0.99) and np.abs(np.linalg.norm(Xbd[0].float().cpu().numpy(), axis=1) - 0.6).max() < 0.01
    r = np.linalg.norm(X, axis=1)
    away = np.abs(r - 0.6) > 0.01
    assert (np.sign(Y[away]) == np.sign(r[away] - 0.6)).all()
    near = np.abs(r[:n // 2] - 0.6)
    assert 0.005 < np.median(near) < 0.02                                          # near_std = 0.015
    again = MS.sdf_sampling_dev(vv, ff, vo, to, sample_N=n, seed=5)
    other = MS.sdf_sampling_dev(vv, ff, vo, to, sample_N=n, seed=6)
    assert all(torch.equal(a, b) for a, b in zip((Xbd, Xtg, Ytg), again))
    assert not torch.equal(Xtg, other[1])
    # the numpy-signature versions
    S, I, C = MS.signed_distance(np.zeros((1, 3)), v, f)
    assert S.dtype == np.float64 and I.dtype == np.int64 and abs(S[0] + 0.6) < 0.01
    sdf = MS.mesh2sdf(v, f, gridDim=8)
    assert sdf.shape == (512, 4) and (np.sign(sdf[:, 3]) == np.sign(np.linalg.norm(sdf[:, :3], axis=1) - 0.6)).all()
    a, b, c = MS.SDF_sampling(v, f, sample_N=1000)
    assert a.dtype == np.float16 and a.shape == (1000, 3) and c.shape == (1000,)


def test_make_dataset_end_to_end_into_vqdif_training_step(dev, tmp_path):
    from shapeformer_amd import data as D, make_dataset as MD, meshio
    from shapeformer_amd import weights as Wt
    from shapeformer_amd.train_vqdif import VQDIFTrainer
    v, f = R.icosphere(2, r=3.0)
    (tmp_path / "a.obj").write_text("".join(f"v {x} {y} {z}\n" for x, y, z in v) + "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f))
    cv, cf = R.CUBE_V * [1, 0.5, 0.25] + 4, R.CUBE_F
    (tmp_path / "b.off").write_text(f"OFF\n{len(cv)} {len(cf)} 0\n" + "".join(f"{x} {y} {z}\n" for x, y, z in cv)
                                    + "".join(f"3 {a} {b} {c}\n" for a, b, c in cf))
    meshio.write_ply(str(tmp_path / "c.ply"), v * [1, 2, 1], f)
    paths = [str(tmp_path / n) for n in ("a.obj", "b.off", "c.ply")]
    MD.main(paths + ["--out", str(tmp_path / "root"), "--dataset", "mine", "--split", "train", "--grid", "16", "--boundary-n", "4096",
                     "--cate", "round=*.obj", "--cate", "round2=*c.ply", "--batch", "2"])
    ds = D.Imnet2LowResDataset(dataset="mine", split="train", root=str(tmp_path / "root"), grid_dim=16, boundary_N=2048,
                               cate=["round", "round2"], Xbd_as_Xct=True)
    assert len(ds) == 2
    items = [ds[i] for i in range(2)]
    occ0 = items[0]["Ytg"][:, 0].reshape(16, 16, 16)
    X = D.make_grid([-1, -1, -1.], [1., 1, 1], [16] * 3)
    r = np.linalg.norm(X, axis=1).reshape(16, 16, 16)
    assert occ0[r < 0.9].all() and not occ0[r > 1.05].any()                        # the normalised sphere, radius ~1
    Ytg = np.load(tmp_path / "root" / "mine" / "train" / "Ytg.npy")
    assert Ytg.shape == (3, 16 ** 3 // 8) and np.unpackbits(Ytg[1]).sum() > 0
    batch = {k: np.stack([it[k] for it in items]) for k in ("Xbd", "Xtg", "Ytg")}
    tr = VQDIFTrainer(Wt.make_state_dict(Wt.vqdif_spec(16)), res=16, device=dev)
    out = tr.training_step(dict(Xbd=batch["Xbd"], Xtg=batch["Xtg"][:, :1024], Ytg=batch["Ytg"][:, :1024]))
    assert np.isfinite(float(out["loss"]))
