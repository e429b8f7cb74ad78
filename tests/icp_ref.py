"""Iterative closest point, the numpy statement of the contract of include/sfmi.h (csrc/register.hip).

One pair at a time, brute force.  The transform and the squared distances are stated bit for bit (numpy rounds every product and sum
on its own; fmaf through f64, as tests/segment_ref.py); the sums are stated as per-inlier terms, so a caller gets both their f64 sum
and sum |term|, the scale of the bound 4 n eps sum |term| on any other summation order.  Also here: the scenes of the tests, cut from
tests/golden/demo_ds/armchair/Xbd.npy, PCA normals on the host, and a merge of scans."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demo_ds", "armchair", "Xbd.npy")
NS, SD2, CNT = 29, 27, 28
MIN_CORR = {"point": 3, "plane": 6}
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float64)


# ---- poses ---------------------------------------------------------------------------------------------------------------------------

def rodrigues(w):
    """exp([w]x) = I + a K + c K^2, the series below |w| = 1e-4"""
    w = np.asarray(w, np.float64)
    t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    t = np.sqrt(t2)
    if t < 1e-4:
        a, c = 1.0 - t2 / 6.0 + t2 * t2 / 120.0, 0.5 - t2 / 24.0 + t2 * t2 / 720.0
    else:
        a, c = np.sin(t) / t, (1.0 - np.cos(t)) / t2
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + a * K + c * (K @ K)


def pose12(R, t):
    return np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1).reshape(12)


def pose44(p):
    return np.concatenate([np.asarray(p, np.float64).reshape(3, 4), [[0, 0, 0, 1.0]]])


def apply_step(pose, xi):
    """R <- dR R, t <- dR t + v"""
    T = np.asarray(pose, np.float64).reshape(3, 4)
    dR = rodrigues(xi[:3])
    return pose12(dR @ T[:, :3], dR @ T[:, 3] + xi[3:])


def transform(p, pose):
    """x' = f32(((r0 x + r1 y) + r2 z) + t), the f32 point widened first"""
    T = np.asarray(pose, np.float64).reshape(3, 4)
    p = np.asarray(p, np.float32).reshape(-1, 3).astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([(((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32) for r in range(3)], 1)


# ---- correspondences ----------------------------------------------------------------------------------------------------------------

def _fmaf(a, b, c):
    """fmaf on f32 arrays: the product is exact in f64, one f64 add, one rounding to f32 (as tests/segment_ref.py)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def nn(a, q):
    """nn_dist's rule: (idx int32, d2 f32), the lowest index among equal f32 distances, (-1, +inf) without a candidate"""
    a, q = np.asarray(a, np.float32).reshape(-1, 3), np.asarray(q, np.float32).reshape(-1, 3)
    idx, d2 = np.full(len(a), -1, np.int32), np.full(len(a), np.inf, np.float32)
    if len(q) == 0:
        return idx, d2
    for i0 in range(0, len(a), 512):
        with np.errstate(all="ignore"):
            d = a[i0:i0 + 512, None, :] - q[None, :, :]
            m = _fmaf(d[..., 2], d[..., 2], _fmaf(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))
        m = np.where(np.isnan(m), np.float32(np.inf), m)
        j = np.argmin(m, 1)
        v = m[np.arange(len(j)), j]
        idx[i0:i0 + 512] = np.where(np.isinf(v), -1, j)
        d2[i0:i0 + 512] = v
    return idx, d2


def maxd2_of(max_dist):
    return np.float32(float(max_dist) ** 2)


# ---- the normal equations -----------------------------------------------------------------------------------------------------------

def terms(a, q, nrm, idx, d2, max_dist, metric):
    """(inliers, 29) f64: every inlier's contribution to A (21 upper entries, row-major) | J^T r (6) | d2 | 1"""
    inl = (idx >= 0) & (d2 <= maxd2_of(max_dist))
    a = np.asarray(a, np.float32)[inl].astype(np.float64)
    qq = np.asarray(q, np.float32).reshape(-1, 3)[idx[inl]].astype(np.float64)
    k = len(a)
    out = np.zeros((k, NS))
    ax, ay, az = a[:, 0], a[:, 1], a[:, 2]
    dx, dy, dz = ax - qq[:, 0], ay - qq[:, 1], az - qq[:, 2]
    if metric == "plane":
        n = np.asarray(nrm, np.float32).reshape(-1, 3)[idx[inl]].astype(np.float64)
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        r = (dx * nx + dy * ny) + dz * nz
        J = [ay * nz - az * ny, az * nx - ax * nz, ax * ny - ay * nx, nx, ny, nz]
        e = 0
        for i in range(6):
            for j in range(i, 6):
                out[:, e] = J[i] * J[j]
                e += 1
        for i in range(6):
            out[:, 21 + i] = J[i] * r
    else:
        one = np.ones(k)
        out[:, 0], out[:, 1], out[:, 2] = ay * ay + az * az, -(ax * ay), -(ax * az)
        out[:, 6], out[:, 7], out[:, 11] = ax * ax + az * az, -(ay * az), ax * ax + ay * ay
        out[:, 4], out[:, 5] = -az, ay
        out[:, 8], out[:, 10] = az, -ax
        out[:, 12], out[:, 13] = -ay, ax
        out[:, 15], out[:, 18], out[:, 20] = one, one, one
        out[:, 21], out[:, 22], out[:, 23] = ay * dz - az * dy, az * dx - ax * dz, ax * dy - ay * dx
        out[:, 24], out[:, 25], out[:, 26] = dx, dy, dz
    out[:, SD2] = d2[inl].astype(np.float64)
    out[:, CNT] = 1.0
    return out


def sums_of(t):
    """-> (sums (29,), sum |term| (29,)) of `terms`"""
    return t.sum(0), np.abs(t).sum(0)


def system(s):
    """sums (29,) -> A (6,6), g (6,)"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = s[:21]
    A = A + np.triu(A, 1).T
    return A, -s[21:27]


def cholesky_ok(A):
    """the pivots of the contract: positive, finite and above 1e-12 x the largest diagonal entry"""
    A = A.copy()
    big = max(A.diagonal().max(), 0.0)
    for j in range(6):
        d = A[j, j] - (A[j, :j] ** 2).sum()
        if not d > 0 or not np.isfinite(d) or d <= 1e-12 * big:
            return False
        A[j, j] = np.sqrt(d)
        for i in range(j + 1, 6):
            A[i, j] = (A[i, j] - (A[i, :j] * A[j, :j]).sum()) / A[j, j]
    return True


def evaluate(src, tgt, nrm, pose, max_dist, metric="point"):
    """-> dict(a, idx, d2, sums, abs, fitness, rmse) under `pose`"""
    a = transform(src, pose)
    idx, d2 = nn(a, tgt)
    s, sa = sums_of(terms(a, tgt, nrm, idx, d2, max_dist, metric))
    n, count = len(a), s[CNT]
    return dict(a=a, idx=idx, d2=d2, sums=s, abs=sa, fitness=count / n if n else 0.0, rmse=np.sqrt(s[SD2] / count) if count > 0 else 0.0)


def step(pose, s, metric):
    """one Gauss-Newton step from the sums -> (pose', xi, status): status -1 when the step was taken, else 2 or 3 and the pose stays"""
    if s[CNT] < MIN_CORR[metric]:
        return np.array(pose, np.float64), None, 2
    A, g = system(s)
    if not cholesky_ok(A):
        return np.array(pose, np.float64), None, 3
    xi = np.linalg.solve(A, g)
    return apply_step(pose, xi), xi, -1


def icp(src, tgt, max_dist, metric="point", normals=None, init=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6):
    """-> pose (12,), fitness, rmse, iterations, status: the loop of the contract for one pair"""
    pose = IDENTITY.copy() if init is None else np.asarray(init, np.float64).reshape(-1)[:12].copy()
    src, tgt = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(tgt, np.float32).reshape(-1, 3)
    bad = not (np.isfinite(src).all() and np.isfinite(tgt).all() and np.isfinite(pose).all())
    if metric == "plane":
        bad = bad or not np.isfinite(np.asarray(normals, np.float32)).all()
    if bad:
        return pose, 0.0, 0.0, 0, 4
    pf = pr = None
    for k in range(max_iter + 1):
        e = evaluate(src, tgt, normals, pose, max_dist, metric)
        if k == max_iter:
            return pose, e["fitness"], e["rmse"], k, 1
        if k > 0 and abs(e["fitness"] - pf) < rel_fitness and abs(e["rmse"] - pr) < rel_rmse:
            return pose, e["fitness"], e["rmse"], k, 0
        pose, _, st = step(pose, e["sums"], metric)
        if st >= 0:
            return pose, e["fitness"], e["rmse"], k, st
        pf, pr = e["fitness"], e["rmse"]


# ---- scenes -------------------------------------------------------------------------------------------------------------------------

def fixture():
    return np.load(FIXTURE).astype(np.float32).reshape(-1, 3)


def motion(seed, deg):
    """a rotation of `deg` degrees about a random axis and a translation of N(0, 0.03)"""
    rs = np.random.RandomState(1000 + seed)
    ax = rs.randn(3)
    ax /= np.linalg.norm(ax)
    return rodrigues(ax * np.deg2rad(deg)), rs.randn(3) * 0.03


def moved(q, R, t):
    """the points whose image under (R, t) is q, rounded to f32: a scan of q in its own frame"""
    return ((np.asarray(q, np.float64) - t) @ R).astype(np.float32)


def pca_normals(p, k=16):
    """unit normals by PCA over the k nearest neighbours (the point included), the largest component positive; f32"""
    from scipy.spatial import cKDTree
    p64 = np.asarray(p, np.float64)
    _, nb = cKDTree(p64).query(p64, k=k)
    c = p64[nb] - p64[nb].mean(1, keepdims=True)
    _, v = np.linalg.eigh(np.einsum("nki,nkj->nij", c, c))
    n = v[:, :, 0]
    sg = np.sign(n[np.arange(len(n)), np.abs(n).argmax(1)])
    n = n * np.where(sg == 0, 1.0, sg)[:, None]
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def scene(kind, seed=0, deg=5):
    """-> dict(src, tgt, nrm, R, t).  "S" subset: target = 1400 random points of the fixture, source = 700 of those; "D" disjoint: the
    source is the other 648 points; "H" halves: target x < 0.25, source x > -0.25.  The source is moved by motion(seed, deg)."""
    X = fixture()
    perm = np.random.RandomState(7).permutation(len(X))
    if kind == "S":
        tgt, s = X[perm[:1400]], X[perm[:1400]][np.random.RandomState(8).permutation(1400)[:700]]
    elif kind == "D":
        tgt, s = X[perm[:1400]], X[perm[1400:]]
    elif kind == "H":
        tgt, s = X[X[:, 0] < 0.25], X[X[:, 0] > -0.25]
    else:
        raise ValueError(kind)
    R, t = motion(seed, deg)
    return dict(src=moved(s, R, t), tgt=np.ascontiguousarray(tgt), nrm=pca_normals(tgt), R=R, t=t)


def pose_error(pose, R, t):
    """(|| R - Rt ||_F, max |t - tt|)"""
    T = np.asarray(pose, np.float64).reshape(-1)[:12].reshape(3, 4)
    return np.linalg.norm(T[:, :3] - R), np.abs(T[:, 3] - t).max()


# ---- merging scans ------------------------------------------------------------------------------------------------------------------

def chamfer(a, b):
    """mean squared nearest distance a -> b plus b -> a, in f64"""
    from scipy.spatial import cKDTree
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (cKDTree(b).query(a)[0] ** 2).mean() + (cKDTree(a).query(b)[0] ** 2).mean()


def merge(clouds, max_dist, **kw):
    """scans 1.. registered onto scan 0 (point metric) and transformed -> (merged cloud, poses, statuses); status >= 2 is left out"""
    out, poses, stats = [np.asarray(clouds[0], np.float32)], [IDENTITY.copy()], [0]
    for c in clouds[1:]:
        pose, _, _, _, st = icp(c, clouds[0], max_dist, "point", **kw)
        poses.append(pose)
        stats.append(st)
        if st < 2:
            out.append(transform(c, pose))
    return np.concatenate(out), np.stack(poses), np.array(stats)
