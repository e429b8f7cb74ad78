"""GPU tests of exact k-nearest neighbours and the scan-cleaning front end (shapeformer_amd/scan.py, csrc/knn.hip)
against tests/knn_ref.py: cKDTree for the ranks, PCL's formula for the outlier mask, np.linalg.eigh in f64 for the normals.  Shapes are
the smallest that reach each path: every instance bucket's edges, sets smaller than k, the split path with its merge, a two-point set."""

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import knn_ref as R
from shapeformer_amd import _lib as L
from shapeformer_amd import metrics as M
from shapeformer_amd import scan
from shapeformer_amd._lib import SfmiError

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 63, 64, 65, 300, 1000, 4097]
KS = [1, 2, 8, 9, 16, 17, 32, 33, 64]            # the edges of the instance buckets 8 / 16 / 32 / 64


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


@pytest.fixture(scope="module")
def ragged():
    rs = np.random.RandomState(0)
    p = (rs.rand(sum(SIZES), 3) - 0.5).astype(np.float32)
    q = (rs.rand(sum(SIZES), 3) - 0.5).astype(np.float32)
    return p, q, _off(SIZES), _off(SIZES[::-1])


@pytest.fixture(scope="module")
def split_case():
    rs = np.random.RandomState(1)
    return (rs.rand(100, 3) - 0.5).astype(np.float32), (rs.rand(40000, 3) - 0.5).astype(np.float32)


# ---- 1. ranks against cKDTree

@pytest.mark.parametrize("k", KS)
def test_ranks_against_ckdtree(dev, ragged, k):
    p, q, po, qo = ragged
    d2, idx = _np(*scan.knn_dev(_t(p, dev), _t(q, dev), k, po, qo))
    assert d2.shape == (len(p), k) and d2.dtype == np.float32 and idx.dtype == np.int32
    R.check_order(d2, idx)
    for b in range(len(SIZES)):
        s = slice(po[b], po[b + 1])
        R.check_ranks(d2[s], idx[s], p[s], q[qo[b]:qo[b + 1]], k)        # includes: rows of a set smaller than k end in (+inf, -1)


@pytest.mark.parametrize("k", [1, 8, 17, 64])
def test_ranks_exclude_self(dev, ragged, k):
    p, _, po, _ = ragged
    pt = _t(p, dev)
    d2, idx = _np(*scan.knn_dev(pt, pt, k, po, po, exclude_self=True))
    R.check_order(d2, idx)
    for b in range(len(SIZES)):
        s = slice(po[b], po[b + 1])
        R.check_ranks(d2[s], idx[s], p[s], p[s], k, exclude_self=True)
    assert np.isposinf(d2[0]).all() and (idx[0] == -1).all()             # the one-point set offers nothing


# ---- 2. order and ties

def test_ties_take_the_lower_index(dev):
    u = (np.random.RandomState(2).rand(500, 3) - 0.5).astype(np.float32)
    d2, idx = _np(*scan.knn_dev(_t(u, dev), _t(np.tile(u, (3, 1)), dev), 3))
    i = np.arange(500)
    assert np.array_equal(idx, np.stack([i, i + 500, i + 1000], 1)) and np.all(d2 == 0)
    # k past the three copies: the fourth entry is a different point
    d2, idx = _np(*scan.knn_dev(_t(u, dev), _t(np.tile(u, (3, 1)), dev), 6))
    assert np.array_equal(idx[:, :3], np.stack([i, i + 500, i + 1000], 1)) and np.all(d2[:, 3] > 0)
    assert np.array_equal(idx[:, 4], idx[:, 3] + 500) and np.array_equal(idx[:, 5], idx[:, 3] + 1000)
    R.check_order(d2, idx)


def test_exclude_self_skips_by_index_not_by_distance(dev):
    u = (np.random.RandomState(3).rand(500, 3) - 0.5).astype(np.float32)
    pq = _t(np.tile(u, (2, 1)), dev)
    d2, idx = _np(*scan.knn_dev(pq, pq, 1, exclude_self=True))
    assert np.array_equal(idx[:, 0], (np.arange(1000) + 500) % 1000) and np.all(d2 == 0)       # its duplicate remains a neighbour
    d2, idx = _np(*scan.knn_dev(pq, pq, 1))
    assert np.array_equal(idx[:, 0], np.arange(1000) % 500)                                    # without: the lower of the two copies


# ---- 3. the split path

@pytest.mark.parametrize("k", [8, 16, 32, 64])                           # every instance of knn_merge_kernel<K>
def test_split_path(dev, split_case, k):
    p, q = split_case
    lib = L.lib()
    assert lib.sfmi_knn_workspace_bytes(1, 100, 40000, k) > 100 * k * 8                       # this shape takes partial lists
    pt, qt = _t(p, dev), _t(q, dev)
    d2t, idxt = scan.knn_dev(pt, qt, k)
    d2, idx = _np(d2t, idxt)
    R.check_order(d2, idx)
    R.check_ranks(d2, idx, p, q, k)
    # the same queries against the same references as the first set of a two-set batch: another split, the same bits
    p2, q2 = np.concatenate([p, p[:7]]), np.concatenate([q, q[:3000]])
    e2, edx = scan.knn_dev(_t(p2, dev), _t(q2, dev), k, [0, 100, 107], [0, 40000, 43000])
    assert torch.equal(e2[:100], d2t) and torch.equal(edx[:100], idxt)
    R.check_ranks(*_np(e2[100:], edx[100:]), p[:7], q[:3000], k)
    # anchors: column 0 is nn_dist, and two runs agree
    n2, ni = M.nn_dist(pt, qt, return_index=True)
    assert torch.equal(d2t[:, 0], n2) and torch.equal(idxt[:, 0], ni)
    again = scan.knn_dev(pt, qt, k)
    assert torch.equal(again[0], d2t) and torch.equal(again[1], idxt)


def test_split_path_ties_and_exclude_self(dev):
    # 20000 points twice over: each point's duplicate lies in another chunk of the split, and ties must come out in index order
    u = (np.random.RandomState(4).rand(20000, 3) - 0.5).astype(np.float32)
    q = np.tile(u, (2, 1))
    assert L.lib().sfmi_knn_workspace_bytes(1, 100, 40000, 16) > 100 * 16 * 8
    d2, idx = _np(*scan.knn_dev(_t(u[:100], dev), _t(q, dev), 16))
    assert np.array_equal(idx[:, 0], np.arange(100)) and np.array_equal(idx[:, 1], np.arange(100) + 20000) and np.all(d2[:, :2] == 0)
    assert np.array_equal(idx[:, 3], idx[:, 2] + 20000)
    R.check_order(d2, idx)
    R.check_ranks(d2, idx, u[:100], q, 16)
    assert L.lib().sfmi_knn_workspace_bytes(1, 40000, 40000, 8) > 40000 * 8 * 8
    qt = _t(q, dev)
    d2, idx = _np(*scan.knn_dev(qt, qt, 8, exclude_self=True))
    assert np.array_equal(idx[:, 0], (np.arange(40000) + 20000) % 40000) and np.all(d2[:, 0] == 0)
    R.check_order(d2, idx)


@pytest.fixture(scope="module")
def doubled():
    """the 40000-point duplicated cloud of test_split_path_ties_and_exclude_self"""
    return np.tile((np.random.RandomState(4).rand(20000, 3) - 0.5).astype(np.float32), (2, 1))


@pytest.mark.parametrize("k", [16, 32, 64])
def test_split_path_exclude_self(dev, doubled, k):
    """exclude_self under a split for the other three merge instances: by the plan in knn.hip the 40000 x 40000 search is cut into
    16, 7 and 5 chunks for K = 16, 32 and 64, so a point's duplicate lies in another chunk than the point"""
    q = doubled
    assert L.lib().sfmi_knn_workspace_bytes(1, 40000, 40000, k) > 40000 * k * 8              # this shape takes partial lists
    qt = _t(q, dev)
    d2, idx = _np(*scan.knn_dev(qt, qt, k, exclude_self=True))
    assert np.array_equal(idx[:, 0], (np.arange(40000) + 20000) % 40000) and np.all(d2[:, 0] == 0)
    assert np.array_equal(idx[:, 2], (idx[:, 1] + 20000) % 40000)        # the next neighbour's two copies, the lower index first
    assert np.all(idx[:, 1] < 20000) and np.all(d2[:, 1] == d2[:, 2])
    R.check_order(d2, idx)
    R.check_ranks(d2, idx, q, q, k, exclude_self=True)


# ---- 4. anchors inside the project

def test_anchors(dev, ragged):
    p, q, po, qo = ragged
    pt, qt = _t(p, dev), _t(q, dev)
    n2, ni = M.nn_dist(pt, qt, po, qo, return_index=True)
    for k in (1, 8, 16, 32, 64):
        d2, idx = scan.knn_dev(pt, qt, k, po, qo)
        assert torch.equal(d2[:, 0], n2) and torch.equal(idx[:, 0], ni)
        again = scan.knn_dev(pt, qt, k, po, qo)
        assert torch.equal(again[0], d2) and torch.equal(again[1], idx)
    # a smaller k is a prefix of a larger one, across instances
    d64, i64 = scan.knn_dev(pt, qt, 64, po, qo)
    for k in (2, 9, 17, 33):
        d2, idx = scan.knn_dev(pt, qt, k, po, qo)
        assert torch.equal(d2, d64[:, :k]) and torch.equal(idx, i64[:, :k])
    # the batched form is the ragged form
    rs = np.random.RandomState(5)
    pb, qb = _t(rs.rand(3, 70, 3).astype(np.float32), dev), _t(rs.rand(3, 90, 3).astype(np.float32), dev)
    for ex, qq in ((False, qb), (True, pb)):
        db, ib = scan.knn_dev(pb, qq, 9, exclude_self=ex)
        n, m = pb.shape[1], qq.shape[1]
        dr, ir = scan.knn_dev(pb.reshape(-1, 3), qq.reshape(-1, 3), 9, [0, n, 2 * n, 3 * n], [0, m, 2 * m, 3 * m], exclude_self=ex)
        assert db.shape == (3, n, 9) and torch.equal(db.reshape(-1, 9), dr) and torch.equal(ib.reshape(-1, 9), ir)
    # empty query sets are fine, also against empty reference sets
    d2, idx = scan.knn_dev(pt[:5], qt[:9], 4, [0, 0, 5, 5], [0, 0, 9, 9])
    assert d2.shape == (5, 4)
    assert scan.knn_dev(pt[:0], qt[:0], 4)[0].shape == (0, 4)
    with pytest.raises(SfmiError, match="reference set is empty"):
        scan.knn_dev(pt[:5], qt[:9], 4, [0, 2, 5], [0, 0, 9])


# ---- 5. outlier masks

@pytest.fixture(scope="module")
def dirty():
    """1000 + 20, 4000 + 80 and a 10-point set"""
    rs = np.random.RandomState(6)
    a = R.planted(1)
    b = np.concatenate([R.sphere(4000, 7, r=0.4), (rs.rand(80, 3) * 2 - 1).astype(np.float32)])
    c = (rs.rand(10, 3) - 0.5).astype(np.float32)
    return np.concatenate([a, b, c]), _off([len(a), len(b), len(c)])


def _band_compare(keep, stat, thr, what):
    """keep must equal stat <= thr except where stat lies within 1e-9 relative of thr; at most 0.1 % of the points may be excepted"""
    fin = np.isfinite(thr)                                               # an infinite threshold (a set smaller than k + 1) has no band
    band = np.zeros(len(keep), bool)
    band[fin] = np.abs(stat[fin] - thr[fin]) <= 1e-9 * np.abs(thr[fin])
    print(f"{what}: {int(band.sum())} of {len(keep)} points in the band")
    assert band.mean() <= 1e-3
    assert np.array_equal(keep[~band].astype(bool), (stat <= thr)[~band])


def test_statistical_outlier_mask(dev, dirty):
    x, off = dirty
    xt = _t(x, dev)
    keep, count, stat = scan.statistical_outlier_mask_dev(xt, off, k=16, std_ratio=2.0)
    assert keep.dtype == torch.uint8 and count.dtype == torch.int32 and stat.dtype == torch.float64
    assert keep.shape == (len(x),) and count.shape == (3,) and stat.shape == (len(x),)
    d2, _ = scan.knn_dev(xt, xt, 16, off, off, exclude_self=True)
    m = R.mean_dist(d2.cpu().numpy())                                    # the restatement on the device's own d2
    keep, count, stat = _np(keep, count, stat)
    fin = np.isfinite(m)
    assert np.array_equal(np.isposinf(stat), ~fin) and np.allclose(stat[fin], m[fin], rtol=1e-13, atol=0)
    assert torch.equal(scan.knn_mean_dist_dev(xt, off, 16), _t(stat, dev))
    _band_compare(keep, m, R.sor_threshold(m, off, 16, 2.0), "statistical")
    assert keep[off[2]:].all() and np.isposinf(stat[off[2]:]).all()       # 10 points, k = 16: everything is kept
    assert np.array_equal(count, [keep[off[b]:off[b + 1]].sum() for b in range(3)])
    assert 0 < count[0] < 1020 and 0 < count[1] < 4080 and count[2] == 10
    # a batch equals its sets one by one
    for b in range(3):
        kb, cb, sb = scan.statistical_outlier_mask_dev(xt[off[b]:off[b + 1]], None, k=16, std_ratio=2.0)
        assert np.array_equal(kb.cpu().numpy(), keep[off[b]:off[b + 1]]) and int(cb[0]) == count[b]


def test_planted_outliers_are_removed(dev):
    x = R.planted(0)
    off = _off([len(x)])
    m = R.host_mean_dist(x, off, 8)                                      # the restatement from scratch, asserted first
    thr = R.sor_threshold(m, off, 8, 1.0)
    want = m <= thr
    assert want[:1000].all() and not want[1000:].any() and not (np.abs(m - thr) <= 1e-9 * thr).any()
    assert (~R.sor_mask(m, off, 8, 2.0)[1000:]).sum() < 20               # why not 2.0: the outliers inflate sigma
    keep, count, _ = scan.statistical_outlier_mask_dev(_t(x, dev), None, k=8, std_ratio=1.0)
    assert np.array_equal(keep.cpu().numpy().astype(bool), want) and int(count[0]) == 1000
    # the batched form, and the cleaned cloud: only kept points, bit for bit
    xb = _t(np.stack([x, x[::-1]]), dev)
    kb, cb, sb = scan.statistical_outlier_mask_dev(xb, k=8, std_ratio=1.0)
    assert kb.shape == (2, 1020) and sb.shape == (2, 1020) and cb.tolist() == [1000, 1000]
    assert np.array_equal(kb[0].cpu().numpy().astype(bool), want) and np.array_equal(kb[1].cpu().numpy().astype(bool), want[::-1])
    out, cnt = scan.clean_cloud_dev(xb, k=8, std_ratio=1.0)
    assert out.shape == (2, 1020, 3) and out.dtype == torch.float32 and cnt.tolist() == [1000, 1000]
    out2, _ = scan.clean_cloud_dev(xb, k=8, std_ratio=1.0, out_N=333, seed=3)
    assert out2.shape == (2, 333, 3)
    inl = {r.tobytes() for r in x[:1000]}
    for o in (out, out2):
        assert all(r.tobytes() in inl for r in o.cpu().numpy().reshape(-1, 3))
    assert torch.equal(scan.clean_cloud_dev(xb, k=8, std_ratio=1.0)[0], out)
    assert len({r.tobytes() for r in out[0].cpu().numpy()}) > 500        # a draw over the kept points, not one of them repeated


def test_radius_outlier_mask(dev, dirty):
    x, off = dirty
    radius, mn = 0.05, 4
    keep, count = scan.radius_outlier_mask_dev(_t(x, dev), off, radius, mn)
    assert keep.dtype == torch.uint8 and keep.shape == (len(x),) and count.dtype == torch.int32
    keep, count = _np(keep, count)
    want, t_mn = np.zeros(len(x), bool), np.full(len(x), np.inf)
    for b in range(3):
        xb = x[off[b]:off[b + 1]].astype(np.float64)
        n = cKDTree(xb).query_ball_point(xb, radius, return_length=True) - 1          # the point itself is in its own ball
        want[off[b]:off[b + 1]] = n >= mn
        t_mn[off[b]:off[b + 1]] = R.tree_knn(xb, xb, mn + 1)[0][:, mn]                # f64 squared distance of the deciding neighbour
    # the device compares f32 distances (direct form, ~3 * 2^-24 relative) with f32(radius^2); on this input the closest deciding
    # distance is 2e-3 relative away from radius^2 (printed below), so rounding decides no point and the band is empty
    r2 = radius ** 2
    band = np.abs(t_mn - r2) <= 1e-9 * r2
    print(f"radius: {int(band.sum())} of {len(x)} points in the band; closest |t - r^2| / r^2 = {np.abs(t_mn - r2).min() / r2:.3g}")
    assert band.mean() <= 1e-3
    assert np.array_equal(keep[~band].astype(bool), want[~band])
    assert np.array_equal(count, [keep[off[b]:off[b + 1]].sum() for b in range(3)]) and 0 < count[0] < 1020


# ---- 6. normals

@pytest.fixture(scope="module")
def ball():
    x = R.sphere(4096, 0)
    _, tab = cKDTree(x.astype(np.float64)).query(x.astype(np.float64), 16)
    vec, lam = R.pca_normals(x, tab)
    return x, vec, lam


def test_normals_against_eigh(dev, ball):
    x, _, _ = ball
    xt = _t(x, dev)
    normal, var = scan.estimate_normals_dev(xt, None, 16)
    assert normal.shape == (4096, 3) and normal.dtype == torch.float32 and var.shape == (4096,) and var.dtype == torch.float32
    _, tab = scan.knn_dev(xt, xt, 16)                                    # the device's own neighbour table (the point included)
    assert torch.equal(tab[:, 0], torch.arange(4096, device=dev, dtype=torch.int32))
    vec, lam = R.pca_normals(x, tab.cpu().numpy())
    n, v = normal.cpu().numpy().astype(np.float64), var.cpu().numpy().astype(np.float64)
    gap = (lam[:, 1] - lam[:, 0]) / lam[:, 2]
    ok = gap >= 0.05
    ang = R.angle(n, vec)
    print(f"normals: min gap {gap.min():.4f}, {int((~ok).sum())} excluded, max angle {ang[ok].max():.3g} rad")
    assert (~ok).mean() <= 0.01 and np.all(ang[ok] <= 1e-5)
    assert np.all(np.abs(np.linalg.norm(n, axis=1) - 1) <= 1e-6)
    want = lam[:, 0] / lam.sum(1)
    assert np.all(np.abs(v - want) <= 1e-5 * want + 1e-9)
    assert np.all(np.abs(n).max(1) == n.max(1))                          # no viewpoint: the largest component is positive


def test_normals_geometry_and_orientation(dev, ball):
    x, vec, lam = ball
    rad = x.astype(np.float64) / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)
    a = np.degrees(R.angle(vec, rad))                                    # the restatement first
    assert np.median(a) < 2.5 and a.max() < 15 and ((lam[:, 1] - lam[:, 0]) / lam[:, 2]).min() >= 0.05
    xt = _t(x, dev)
    normal, _ = scan.estimate_normals_dev(xt, None, 16, viewpoint=np.zeros(3))
    n = normal.cpu().numpy().astype(np.float64)
    a = np.degrees(R.angle(n, rad))
    print(f"normals: median angle to the radius {np.median(a):.2f} deg, max {a.max():.2f} deg")
    assert np.median(a) < 2.5 and a.max() < 15
    assert np.all((n * x).sum(1) < 0)                                    # towards the viewpoint at the origin
    far, _ = scan.estimate_normals_dev(xt, None, 16, viewpoint=torch.tensor([[0.0, 0.0, 100.0]]))
    f = far.cpu().numpy().astype(np.float64)
    assert np.all((f * (np.array([0, 0, 100.0]) - x)).sum(1) >= 0)
    free, _ = scan.estimate_normals_dev(xt, None, 16)
    assert np.all(np.abs(np.abs(free.cpu().numpy()) - np.abs(normal.cpu().numpy())) == 0)      # the sign is all a viewpoint changes


def test_normals_ragged_with_a_two_point_set(dev, ball):
    x, _, _ = ball
    pts = np.concatenate([x[:300], x[300:302], x[302:1000]])
    off = _off([300, 2, 698])
    normal, var = scan.estimate_normals_dev(_t(pts, dev), off, 16, viewpoint=np.zeros((3, 3)))
    n, v = _np(normal, var)
    assert np.all(n[300:302] == 0) and np.isnan(v[300:302]).all()
    rest = np.r_[0:300, 302:1000]
    assert np.isfinite(v[rest]).all() and np.all(np.abs(np.linalg.norm(n[rest].astype(np.float64), axis=1) - 1) <= 1e-6)
    for s in (slice(0, 300), slice(302, 1000)):                          # a batch equals its sets one by one
        nb, vb = scan.estimate_normals_dev(_t(pts[s], dev), None, 16, viewpoint=np.zeros(3))
        assert np.array_equal(nb.cpu().numpy(), n[s]) and np.array_equal(vb.cpu().numpy(), v[s])
    nb3, vb3 = scan.estimate_normals_dev(_t(x[:1024].reshape(4, 256, 3), dev), None, 8)
    assert nb3.shape == (4, 256, 3) and vb3.shape == (4, 256)


# ---- 7. wiring

def test_points_dist_k(dev, ragged):
    p, q, po, qo = ragged
    p1, p2 = p[po[5]:po[6]], q[qo[1]:qo[2]]                              # 300 against 1000
    dist, ind = M.points_dist(p1, p2, k=5, return_ind=True)
    assert dist.shape == (300, 5) and dist.dtype == np.float64 and ind.shape == (300, 5) and ind.dtype == np.int64
    R.check_ranks((dist ** 2).astype(np.float32), ind.astype(np.int32), p1, p2, 5)
    td, ti = cKDTree(p2.astype(np.float64)).query(p1.astype(np.float64), 5)
    assert np.allclose(dist, td, rtol=1e-6, atol=1e-9) and (ind == ti).mean() > 0.99
    assert np.array_equal(M.points_dist(p1, p2, k=5), dist)
    assert M.points_dist(p1, p2, k=2).shape == (300, 2) and M.points_dist(p1, p2).shape == (300,)      # k = 1 stays a vector
    with pytest.raises(SfmiError, match="k must be"):
        M.points_dist(p1, p2, k=65)


def test_callback_clean_context(dev, tmp_path):
    """VisShapeFormer(clean_context=None) computes what a callback built without the argument computes; with it, the planted cloud's
    outliers never reach the encoder and `context_kept` says how many points did.  The model setup of test_simplify_gpu.py."""
    from test_plugin_gpu import _opt
    from shapeformer_amd import plugin as P
    model = P.instantiate_from_opt(P.get_opt(_opt())["pl_model_opt"])
    kw = dict(end_tokens=[4096, 4096], top_k=100, top_p=0.4, depth=4, visual_indices=[0], sample_n=2, sample_max_step=12, decode_res=32)
    name = "shapeformer.models.shapeformer.shapeformer.VisShapeFormer"
    x = R.planted(0)
    batch = {"Xct": torch.from_numpy(x)[None]}
    outs = {}
    for tag, extra in (("plain", {}), ("none", dict(clean_context=None)), ("clean", dict(clean_context={"k": 8, "std_ratio": 1.0}))):
        cb = P.instantiate_from_opt({"class": name, "kwargs": dict(kw, data_dir=str(tmp_path / tag), **extra)})
        cb.pl_module = model
        outs[tag] = cb.compute_batch(dict(batch), input_name="0")
    a, b = outs["plain"], outs["none"]
    assert sorted(a) == sorted(b) and "context_kept" not in a
    for key in a:
        if key != "batch":
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True) if a[key] is not None else b[key] is None, key
    assert outs["clean"]["context_kept"] == 1000
    assert sorted(set(outs["clean"]) - {"context_kept"}) == sorted(a)
    # the cleaned condition is the encoding of the cleaned cloud
    pipe = model.pipe
    cleaned, _ = scan.clean_cloud_dev(batch["Xct"].to(dev), k=8, std_ratio=1.0)
    enc = pipe.encode_cloud(cleaned)
    assert np.array_equal(outs["clean"]["c_ind"], enc["c_tokens"][:, :int(enc["Lc"][0])].long().cpu().numpy())
