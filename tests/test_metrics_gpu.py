"""GPU: completion metrics (csrc/pointdist.hip, shapeformer_amd/metrics.py) against the reference's own method restated here:
scipy cKDTree(q).query(p, k=1) (xgutils/geoutil.py:362-377), distances compared in float64 on the same f32 inputs."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree
from scipy.stats import chi2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from test_mcubes_cpu import _sphere, _torus   # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-12


def _truth(p, q):
    """cKDTree nearest neighbour of each p in q -> (f64 squared distance, index)."""
    p64, q64 = p.astype(np.float64), q.astype(np.float64)
    _, ind = cKDTree(q64).query(p64, k=1, workers=16)
    d2 = ((p64 - q64[ind]) ** 2).sum(1)
    return d2, ind


def _check_nn(p, q, d2, idx):
    """|d2 - d2_64| <= 1e-6 d2_64 + 1e-12; idx is cKDTree's or has an f64 distance within the same tolerance of the minimum."""
    t, ind = _truth(p, q)
    d2 = d2.astype(np.float64)
    assert (np.abs(d2 - t) <= RTOL * t + ATOL).all(), np.abs(d2 - t).max()
    mine = ((p.astype(np.float64) - q.astype(np.float64)[idx]) ** 2).sum(1)
    assert ((idx == ind) | (np.abs(mine - t) <= RTOL * t + ATOL)).all()


def _sphere_pts(rs, n, r=0.5, jitter=0.002):
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * r + rs.randn(n, 3) * jitter).astype(np.float32)


def test_nn_dist_ragged_against_ckdtree(dev):
    from shapeformer_amd import metrics as M
    rs = np.random.RandomState(0)
    pn, qn = [1, 63, 64, 65, 1000, 4097], [4097, 1000, 65, 64, 63, 1]
    P = [rs.uniform(-1, 1, (n, 3)).astype(np.float32) for n in pn]
    Q = [rs.uniform(-1, 1, (n, 3)).astype(np.float32) for n in qn]
    po, qo = np.concatenate([[0], np.cumsum(pn)]), np.concatenate([[0], np.cumsum(qn)])
    d2, idx = M.nn_dist(torch.from_numpy(np.concatenate(P)).to(dev), torch.from_numpy(np.concatenate(Q)).to(dev),
                        p_off=torch.from_numpy(po).to(dev), q_off=torch.from_numpy(qo), return_index=True)
    d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
    for b in range(len(pn)):
        _check_nn(P[b], Q[b], d2[po[b]:po[b + 1]], idx[po[b]:po[b + 1]])


def test_nn_dist_1e5_surface_pair(dev):
    from shapeformer_amd import metrics as M
    rs = np.random.RandomState(1)
    p, q = _sphere_pts(rs, 10 ** 5), _sphere_pts(rs, 10 ** 5)
    d2, idx = M.nn_dist(torch.from_numpy(p).to(dev), torch.from_numpy(q).to(dev), return_index=True)
    _check_nn(p, q, d2.cpu().numpy(), idx.cpu().numpy())


def test_ties_degenerate_sets_and_determinism(dev):
    from shapeformer_amd import metrics as M
    from shapeformer_amd._lib import SfmiError
    rs = np.random.RandomState(2)
    u = rs.uniform(-1, 1, (2000, 3)).astype(np.float32)
    # duplicates in Q: the first copy wins, also across the Q chunks of a split launch (50 copies over 10^5 points)
    q = torch.from_numpy(np.tile(u, (50, 1))).to(dev)
    p = torch.from_numpy(rs.uniform(-1, 1, (3000, 3)).astype(np.float32)).to(dev)
    d2, idx = M.nn_dist(p, q, return_index=True)
    assert (idx.cpu().numpy() < 2000).all()
    mine = ((p.cpu().numpy().astype(np.float64) - u.astype(np.float64)[idx.cpu().numpy()]) ** 2).sum(1)
    t, _ = _truth(p.cpu().numpy(), u)
    assert (np.abs(mine - t) <= RTOL * t + ATOL).all()
    # P = Q: exact zeros, index of the first occurrence
    w = torch.from_numpy(np.concatenate([u[:700], u[:700], u[700:900]])).to(dev)
    d2w, iw = M.nn_dist(w, w, return_index=True)
    want = np.concatenate([np.arange(700), np.arange(700), 1400 + np.arange(200)])
    assert (d2w == 0).all() and np.array_equal(iw.cpu().numpy(), want)
    # an empty reference set with queries
    with pytest.raises(SfmiError):
        M.nn_dist(p, q, p_off=[0, 1000, 3000], q_off=[0, 0, q.shape[0]])
    # run to run: bit-identical
    d2b, idxb = M.nn_dist(p, q, return_index=True)
    assert torch.equal(d2, d2b) and torch.equal(idx, idxb)
    # batched (B,N,3) form equals the ragged form
    pb, qb = p[:2000].reshape(2, 1000, 3), q[:4000].reshape(2, 2000, 3)
    db, ib = M.nn_dist(pb, qb, return_index=True)
    dr, ir = M.nn_dist(p[:2000], q[:4000], p_off=[0, 1000, 2000], q_off=[0, 2000, 4000], return_index=True)
    assert torch.equal(db.reshape(-1), dr) and torch.equal(ib.reshape(-1), ir)


def test_reference_signature_functions(dev):
    from shapeformer_amd import metrics as M
    rs = np.random.RandomState(3)
    p1, p2 = rs.uniform(-1, 1, (3000, 3)).astype(np.float32), rs.uniform(-1, 1, (2500, 3)).astype(np.float32)
    dist, ind = M.points_dist(p1, p2, return_ind=True)
    tdist, tind = cKDTree(p2.astype(np.float64)).query(p1.astype(np.float64), k=1)
    assert dist.dtype == np.float64 and ind.dtype == np.int64
    assert (np.abs(dist ** 2 - tdist ** 2) <= RTOL * tdist ** 2 + ATOL).all()
    assert np.array_equal(M.points_dist(p1, p2), dist)
    d1, d2 = M.chamfer_dist(p1, p2)
    t1 = cKDTree(p2.astype(np.float64)).query(p1.astype(np.float64), k=1)[0] ** 2
    t2 = cKDTree(p1.astype(np.float64)).query(p2.astype(np.float64), k=1)[0] ** 2
    assert (np.abs(d1 - t1) <= RTOL * t1 + ATOL).all() and (np.abs(d2 - t2) <= RTOL * t2 + ATOL).all()
    # common.py chamfer_distance_naive in float64 torch on (B,T,3) batches
    a = torch.from_numpy(rs.uniform(-1, 1, (3, 700, 3)).astype(np.float32))
    b = torch.from_numpy(rs.uniform(-1, 1, (3, 700, 3)).astype(np.float32))
    dist64 = (a.double().view(3, 700, 1, 3) - b.double().view(3, 1, 700, 3)).pow(2).sum(-1)
    naive = dist64.min(dim=1)[0].mean(dim=1) + dist64.min(dim=2)[0].mean(dim=1)
    c = M.chamfer_distance(a.to(dev), b.to(dev))
    assert c.device == a.to(dev).device and torch.allclose(c.cpu().double(), naive, rtol=1e-6, atol=0)
    c1, c2, i12, i21 = M.chamfer_distance(a.to(dev), b.to(dev), give_id=True)
    assert torch.allclose(c1.cpu().double(), dist64.min(dim=2)[0].mean(dim=1), rtol=1e-6, atol=0)
    assert torch.allclose(c2.cpu().double(), dist64.min(dim=1)[0].mean(dim=1), rtol=1e-6, atol=0)
    assert i12.dtype == torch.int64 and i12.shape == (3, 700) and i21.shape == (3, 700)
    for bb in range(3):                      # the indices: cKDTree's, or as near within the tolerance
        for x, y, ii in ((a[bb].numpy(), b[bb].numpy(), i12[bb].cpu().numpy()), (b[bb].numpy(), a[bb].numpy(), i21[bb].cpu().numpy())):
            _check_nn(x, y, ((x.astype(np.float64) - y.astype(np.float64)[ii]) ** 2).sum(1), ii)
    cn = M.chamfer_distance(a.numpy(), b.numpy(), use_kdtree=False)
    assert isinstance(cn, np.ndarray) and np.allclose(cn, naive.numpy(), rtol=1e-6, atol=0)


def _np_metrics(Xct, S, Xbd, tau):
    """The module docstring's formulas on cKDTree distances (float64)."""
    def d(a, b):
        return cKDTree(b.astype(np.float64)).query(a.astype(np.float64), k=1)[0]

    def cd(a, b):
        return (d(a, b) ** 2).mean() + (d(b, a) ** 2).mean()
    k = len(S)
    uhd = np.array([d(Xct, s).max() for s in S])
    tmd = sum(sum(cd(S[i], S[j]) for j in range(k) if j != i) / (k - 1) for i in range(k))
    f = []
    for s in S:
        P, R = (d(s, Xbd) <= tau).mean(), (d(Xbd, s) <= tau).mean()
        f.append(0.0 if P + R == 0 else 2 * P * R / (P + R))
    return uhd, tmd, np.array([cd(s, Xbd) for s in S]), np.array(f)


def test_metrics_against_numpy_restatement(dev):
    from shapeformer_amd import metrics as M
    rs = np.random.RandomState(4)
    S = [_sphere_pts(rs, n, r=0.5 + 0.01 * i, jitter=0.01) for i, n in enumerate((3000, 2500, 4100, 1777))]
    Xbd = _sphere_pts(rs, 5000, r=0.5, jitter=0.005)
    Xct = Xbd[Xbd[:, 2] > 0.1][:1500]
    tau = 0.02
    uhd, tmd, cd, f = _np_metrics(Xct, S, Xbd, tau)
    St = [torch.from_numpy(s).to(dev) for s in S]
    per, mean = M.uhd(torch.from_numpy(Xct).to(dev), St)
    assert np.allclose(per, uhd, rtol=1e-6, atol=0) and abs(mean - uhd.mean()) <= 1e-6 * uhd.mean()
    assert abs(M.tmd(St) - tmd) <= 1e-5 * tmd
    Xb = torch.from_numpy(Xbd).to(dev)
    for i in range(4):
        assert abs(M.chamfer(St[i], Xb) - cd[i]) <= 1e-5 * cd[i]
        assert abs(M.fscore(St[i], Xb, tau) - f[i]) <= 2.0 / 1777
    ev = M.evaluate(Xct, St, Xbd=Xbd, tau=tau)
    assert ev["k"] == 4 and np.allclose(ev["uhd_per"], uhd, rtol=1e-6) and abs(ev["tmd"] - tmd) <= 1e-5 * tmd
    assert np.allclose(ev["cd_per"], cd, rtol=1e-5) and np.allclose(ev["fscore_per"], f, atol=2.0 / 1777)
    # one TMD launch == the 12 directions as separate calls, bit for bit
    d, off, pairs = M.tmd_directions(St)
    assert len(pairs) == 12
    for n, (i, j) in enumerate(pairs):
        assert torch.equal(d[int(off[n]):int(off[n + 1])], M.nn_dist(St[i], St[j]))


def _mc_batch(dev, occs):
    from shapeformer_amd import mcubes
    return mcubes.marching_cubes_dev(torch.from_numpy(np.stack(occs).astype(np.float32)).to(dev), 0.5)


def _check_on_faces(pts, face, v, f):
    a, b, c = (v[f[face, k]].astype(np.float64) for k in range(3))
    e1, e2, x = b - a, c - a, pts.astype(np.float64) - a
    G = np.stack([np.stack([(e1 * e1).sum(1), (e1 * e2).sum(1)], 1), np.stack([(e1 * e2).sum(1), (e2 * e2).sum(1)], 1)], 1)
    rhs = np.stack([(x * e1).sum(1), (x * e2).sum(1)], 1)
    st = np.linalg.solve(G, rhs[..., None])[..., 0]
    rec = a + st[:, :1] * e1 + st[:, 1:] * e2
    assert np.abs(rec - pts).max() <= 1e-5
    assert st.min() >= -1e-5 and (st.sum(1) <= 1 + 1e-5).all()


def _area(v, f):
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)


def test_mesh_sampling_sphere(dev):
    from shapeformer_amd import metrics as M
    v, f, voff, toff = _mc_batch(dev, [_sphere(64)])
    n = 10 ** 5
    pts, status, face = M.sample_mesh_dev(v, f, voff, toff, n, seed=7, return_face=True)
    assert pts.shape == (n, 3) and status.tolist() == [0]
    P, F, V, T = pts.cpu().numpy(), face.cpu().numpy(), v.cpu().numpy(), f.cpu().numpy()
    _check_on_faces(P, F, V, T)
    # chi^2 of the per-face counts against the areas, faces grouped into 64 bins of equal area
    area = _area(V, T)
    cum = np.cumsum(area) / area.sum()
    bins = np.minimum((cum * 64).astype(int), 63)
    obs = np.bincount(bins[F], minlength=64)
    exp = np.bincount(bins, weights=area, minlength=64) / area.sum() * n
    assert chi2.sf(((obs - exp) ** 2 / exp).sum(), 63) > 1e-3
    # on the marching-cubes surface: radius within the vertices' range, same mean
    rv, rp = np.linalg.norm(V, axis=1), np.linalg.norm(P, axis=1)
    assert rp.max() <= rv.max() + 1e-6 and rp.min() >= rv.min() - 0.01 and abs(rp.mean() - rv.mean()) < 2e-3
    # determinism / seeds
    p2, _ = M.sample_mesh_dev(v, f, voff, toff, n, seed=7)
    p3, _ = M.sample_mesh_dev(v, f, voff, toff, n, seed=8)
    assert torch.equal(pts, p2) and not torch.equal(pts, p3)


def test_mesh_sampling_ragged_batch_and_status(dev):
    from shapeformer_amd import metrics as M
    from shapeformer_amd._lib import SfmiError
    v, f, voff, toff = _mc_batch(dev, [_sphere(40, r=0.5), _torus(40), _sphere(40, r=0.3, c=(0.2, 0, 0))])
    n = 20000
    pts, status, face = M.sample_mesh_dev(v, f, voff, toff, n, seed=3, return_face=True)
    assert status.tolist() == [0, 0, 0]
    V, T = v.cpu().numpy(), f.cpu().numpy()
    for b in range(3):
        vb, fb = V[voff[b]:voff[b + 1]], T[toff[b]:toff[b + 1]]
        _check_on_faces(pts[b * n:(b + 1) * n].cpu().numpy(), face[b * n:(b + 1) * n].cpu().numpy(), vb, fb)
        one, st1, f1 = M.sample_mesh_dev(v[voff[b]:voff[b + 1]], f[toff[b]:toff[b + 1]], None, None, n, seed=3, return_face=True)
        assert torch.equal(one, pts[b * n:(b + 1) * n]) and torch.equal(f1, face[b * n:(b + 1) * n])
    # a zero-area shape: NaN points, status 1; its neighbours are untouched
    dv = torch.tensor([[0, 0, 0], [1, 1, 1], [2, 2, 2]], dtype=torch.float32, device=dev)
    vv = torch.cat([v[:voff[1]], dv])
    ff = torch.cat([f[:toff[1]], torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)])
    p2, s2 = M.sample_mesh_dev(vv, ff, [0, voff[1], voff[1] + 3], [0, toff[1], toff[1] + 1], n, seed=3)
    assert s2.tolist() == [0, 1] and torch.isnan(p2[n:]).all() and torch.equal(p2[:n], pts[:n])
    with pytest.raises(SfmiError):
        M.sample_mesh_dev(vv, ff, [0, voff[1], voff[1] + 3], [0, toff[1] + 1, toff[1] + 1], n)


def test_callback_eval_metrics(dev, tmp_path):
    """VisShapeFormer(eval_metrics=True) on the test_plugin_gpu setup: metrics JSON == metrics.evaluate on the returned device
    samples; eval/0.npz and every .ply byte-identical to a run with the flag off."""
    from test_plugin_gpu import _Items, _opt
    from shapeformer_amd import metrics as M, plugin as P
    model = P.instantiate_from_opt(P.get_opt(_opt())["pl_model_opt"])
    data = _Items(1)
    outs = {}
    for flag in (False, True):
        cb = P.instantiate_from_opt({"class": "shapeformer.models.shapeformer.shapeformer.VisShapeFormer", "kwargs": dict(
            end_tokens=[4096, 4096], top_k=100, top_p=0.4, depth=4, visual_indices=[0], sample_n=4, sample_max_step=12, decode_res=32,
            data_dir=str(tmp_path / str(flag)), eval_metrics=flag, eval_points=20000)})
        np.random.seed(0)
        outs[flag] = cb.process(model, data)["0"]
    off, on = tmp_path / "False", tmp_path / "True"
    plys = sorted(os.listdir(off / "meshes"))
    assert plys == sorted(os.listdir(on / "meshes"))
    for name in plys:
        assert (off / "meshes" / name).read_bytes() == (on / "meshes" / name).read_bytes()
    if not any(p.startswith("0_s") for p in plys):
        pytest.fail("no completion mesh to score")
    assert (off / "eval" / "0.npz").read_bytes() == (on / "eval" / "0.npz").read_bytes()
    assert not (off / "eval" / "0_metrics.json").exists() and "metrics" not in outs[False]
    res = json.loads((on / "eval" / "0_metrics.json").read_text())
    nums = [x for k, x in res.items() if k != "keys" for x in (x if isinstance(x, list) else [x])]
    assert np.isfinite(nums).all() and {"uhd", "uhd_per", "cd", "fscore"} <= set(res)
    item = data[0]
    again = M.evaluate(item["Xct"], outs[True]["metrics_pc"], Xbd=item["Xbd"], tau=0.01)
    for k, x in again.items():
        assert res[k] == pytest.approx(x, rel=1e-12, abs=0), k
    assert res == outs[True]["metrics"]
