"""numpy / scipy restatement of the contract of shapeformer_amd/scan.py, for tests/test_scan_gpu.py and
tests/test_scan_cpu.py: scipy's cKDTree for the neighbour ranks, PCL's formula for the statistical outlier mask, np.linalg.eigh in
f64 for the normals.  Everything here runs on the host in f64 on the f32 inputs the device gets."""
import numpy as np
from scipy.spatial import cKDTree

RTOL, ATOL = 1e-6, 1e-12        # on squared distances: the tolerances of tests/test_metrics_gpu.py (f32 direct form: ~3 * 2^-24 relative)


def tree_knn(p, q, k):
    """cKDTree(q).query(p, k) on f64 copies -> (t (N,k) f64 squared distances recomputed directly from the f32 inputs, idx (N,k) int64);
    ranks the set does not offer: t = inf, idx = -1."""
    p64, q64 = np.asarray(p, np.float64), np.asarray(q, np.float64)
    _, idx = cKDTree(q64).query(p64, k=k)
    idx = np.asarray(idx, np.int64).reshape(len(p64), k)
    miss = idx >= len(q64)
    safe = np.where(miss, 0, idx)
    t = ((p64[:, None, :] - q64[safe]) ** 2).sum(-1)
    t[miss] = np.inf
    idx[miss] = -1
    return t, idx


def check_ranks(d2, idx, p, q, k, exclude_self=False):
    """The rank rule: rank by rank |d2 - t| <= RTOL * t + ATOL with t the f64 squared distance of cKDTree's neighbour of that rank; each
    index equals cKDTree's or its own f64 distance is within that tolerance of t; indices within a row are distinct; rows of a set
    smaller than k end in (+inf, -1) at exactly the right column.  d2 (N,k) f32, idx (N,k) int32 (numpy).  Raises AssertionError."""
    p64, q64 = np.asarray(p, np.float64), np.asarray(q, np.float64)
    N = len(p64)
    if exclude_self:
        t, ti = tree_knn(p, q, k + 1)
        # drop the query's own index from each row (it is among the zero-distance entries, not necessarily first among duplicates)
        rows_t, rows_i = [], []
        for i in range(N):
            own = np.nonzero(ti[i] == i)[0]
            cut = own[0] if len(own) else ti.shape[1] - 1
            rows_t.append(np.delete(t[i], cut))
            rows_i.append(np.delete(ti[i], cut))
        t, ti = np.array(rows_t).reshape(N, -1), np.array(rows_i).reshape(N, -1)
        pad = k - t.shape[1]
        if pad > 0:
            t = np.concatenate([t, np.full((N, pad), np.inf)], 1)
            ti = np.concatenate([ti, np.full((N, pad), -1, np.int64)], 1)
        t, ti = t[:, :k], ti[:, :k]
    else:
        t, ti = tree_knn(p, q, k)
    assert d2.shape == (N, k) and idx.shape == (N, k) and d2.dtype == np.float32 and idx.dtype == np.int32
    offered = len(q64) - (1 if exclude_self else 0)
    fin = np.isfinite(t)
    assert np.array_equal(fin, np.broadcast_to(np.arange(k)[None, :] < offered, (N, k)))
    assert np.array_equal(np.isposinf(d2), ~fin) and np.array_equal(idx == -1, ~fin)
    err = np.abs(d2.astype(np.float64)[fin] - t[fin])
    assert np.all(err <= RTOL * t[fin] + ATOL), float(err.max())
    assert np.all((idx[fin] >= 0) & (idx[fin] < len(q64)))
    own = ((p64[:, None, :] - q64[np.where(fin, idx, 0)]) ** 2).sum(-1)
    same = idx == ti
    assert np.all(same[fin] | (np.abs(own[fin] - t[fin]) <= RTOL * t[fin] + ATOL))
    if exclude_self:
        assert not np.any(idx == np.arange(N)[:, None])
    s = np.sort(np.where(fin, idx, -1 - np.arange(k)[None, :]), axis=1)          # padding made distinct
    assert np.all(s[:, 1:] != s[:, :-1])


def check_order(d2, idx):
    """every row ascending in (d2, idx) lexicographic order (the +inf / -1 tail excepted: it only has to stay +inf / -1)"""
    a, b = d2[:, :-1], d2[:, 1:]
    tail = np.isposinf(b)
    assert np.all((a < b) | ((a == b) & (idx[:, :-1] < idx[:, 1:])) | tail)
    assert np.all(idx[:, 1:][tail] == -1)


def mean_dist(d2):
    """(N,k) f32 squared distances -> (N,) f64 mean Euclidean distance"""
    return np.sqrt(np.asarray(d2, np.float64)).mean(1)


def sor_threshold(m, off, k, std_ratio):
    """PCL StatisticalOutlierRemoval: per set mu + std_ratio * sigma (sigma with n - 1) broadcast to the points -> (N,) f64;
    +inf for the points of a set with fewer than k + 1 points (they are all kept)"""
    thr = np.empty(len(m), np.float64)
    for b in range(len(off) - 1):
        v = m[off[b]:off[b + 1]]
        thr[off[b]:off[b + 1]] = np.inf if len(v) < k + 1 else v.mean() + std_ratio * v.std(ddof=1)
    return thr


def sor_mask(m, off, k, std_ratio):
    return m <= sor_threshold(m, off, k, std_ratio)


def host_mean_dist(points, off, k):
    """the statistic from scratch on the host: mean distance to the k nearest other points of the same set, f64"""
    out = np.full(len(points), np.inf)
    for b in range(len(off) - 1):
        x = np.asarray(points[off[b]:off[b + 1]], np.float64)
        if len(x) >= k + 1:
            d, _ = cKDTree(x).query(x, k=k + 1)
            out[off[b]:off[b + 1]] = d[:, 1:].mean(1)
    return out


def pca_normals(points, table):
    """points (n,3), table (n,k) local neighbour indices (-1 skipped) -> unit eigenvector of the smallest eigenvalue (n,3) f64 (sign
    free), eigenvalues ascending (n,3) f64, of the neighbours' covariance about their centroid.  Fewer than 3 neighbours: NaN rows."""
    x = np.asarray(points, np.float64)
    vec, lam = np.full((len(x), 3), np.nan), np.full((len(x), 3), np.nan)
    for i in range(len(x)):
        nb = table[i][table[i] >= 0]
        if len(nb) < 3:
            continue
        y = x[nb] - x[nb].mean(0)
        w, v = np.linalg.eigh(y.T @ y / len(nb))
        vec[i], lam[i] = v[:, 0], w
    return vec, lam


def angle(a, b):
    """angle between the LINES of unit-ish vectors a, b (n,3): asin of the cross-product norm after normalising, f64"""
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    b = b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.arcsin(np.clip(np.linalg.norm(np.cross(a, b), axis=1), 0.0, 1.0))


def sphere(n, seed, r=0.5, jitter=0.002):
    rs = np.random.RandomState(seed)
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * r + rs.randn(n, 3) * jitter).astype(np.float32)


def planted(seed=0, n=1000, n_out=20, r=0.5, jitter=0.002, gap=0.1):
    """n jittered samples of a sphere followed by n_out uniform points of [-1, 1]^3 at least `gap` away from its surface -> (n + n_out, 3) f32"""
    rs = np.random.RandomState(seed + 1000)
    out = []
    while len(out) < n_out:
        c = rs.uniform(-1, 1, 3)
        if abs(np.linalg.norm(c) - r) >= gap:
            out.append(c)
    return np.concatenate([sphere(n, seed, r, jitter), np.asarray(out, np.float32)])
