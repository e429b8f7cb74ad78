"""numpy restatement of the two contracts of csrc/downsample.hip (shapeformer_amd/scan.py farthest_point_sample_dev and
voxel_downsample_dev), for tests/test_downsample_gpu.py and tests/test_downsample_cpu.py.  Everything runs on the host."""
import math

import numpy as np

from knn_ref import ATOL, RTOL      # on squared distances: the f32 direct form's error


def _fmaf(a, b, c):
    """fmaf on f32 arrays: the product is exact in f64, one f64 add, one rounding to f32 (exact whenever the f32 result is)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def direct_d2(p, s):
    """f32 (m,3) points, f32 (3,) s -> fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with f32 differences: nn_dist's direct form"""
    d = p - s[None, :]
    return _fmaf(d[:, 2], d[:, 2], _fmaf(d[:, 1], d[:, 1], d[:, 0] * d[:, 0]))


def fps(points, n, start=None, valid=None):
    """The contract of farthest_point_sample_dev for one set, as a loop on f32 arrays -> idx (n,) int32, d2 (n,) f32, count, status.
    Exact (the bits any correct implementation gives) on inputs whose differences, squares and sums are exact in f32."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    cand = np.ones(len(p), bool) if valid is None else np.asarray(valid) != 0
    idx, d2 = np.full(n, -1, np.int32), np.zeros(n, np.float32)
    if not cand.any():
        return idx, d2, 0, 1
    if not np.isfinite(p[cand]).all():
        return idx, d2, 0, 2
    count = min(n, int(cand.sum()))
    dist = np.where(cand, np.float32(np.inf), np.float32(-1))            # -1: not, or no longer, a candidate
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(count):
            s = int(start) if t == 0 and start is not None else int(np.argmax(dist))      # argmax: the first, i.e. lowest, index of the maximum
            idx[t], d2[t] = s, dist[s]
            dist = np.where(dist < 0, dist, np.minimum(dist, direct_d2(p, p[s])))
            dist[s] = -1
    return idx, d2, count, 0


def fps_brute(points, n):
    """the definition from scratch, f64: pick t maximises the distance to the set of earlier picks, the lowest index on a tie"""
    p = np.asarray(points, np.float64)
    picks = [0]
    while len(picks) < min(n, len(p)):
        d = ((p[:, None, :] - p[picks][None]) ** 2).sum(-1).min(1)
        d[picks] = -1
        picks.append(int(np.argmax(d)))
    return np.asarray(picks[:n], np.int32)


def check_greedy(points, idx, d2, count, start=None, valid=None):
    """For arbitrary floats: rebuild the running minimum in f64 along the device's OWN picks and demand that every pick is a true arg
    max within 2 * RTOL * max + ATOL and that the reported d2 is within RTOL * t + ATOL of the f64 value t.  Raises AssertionError."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    cand = np.ones(len(p), bool) if valid is None else np.asarray(valid) != 0
    n = len(idx)
    assert idx.dtype == np.int32 and d2.dtype == np.float32 and d2.shape == (n,)
    assert count == min(n, int(cand.sum()))
    assert np.all(idx[count:] == -1) and np.all(d2[count:] == 0)
    dist = np.where(cand, np.inf, -np.inf)
    for t in range(count):
        s = int(idx[t])
        assert 0 <= s < len(p) and dist[s] > -np.inf, (t, s)            # a candidate, not picked before
        if t == 0:
            assert s == (int(start) if start is not None else int(np.flatnonzero(cand)[0])) and np.isposinf(d2[0])
        else:
            mx = dist.max()
            assert dist[s] >= mx - (2 * RTOL * mx + ATOL), (t, s, dist[s], mx)
            assert abs(float(d2[t]) - dist[s]) <= RTOL * dist[s] + ATOL, (t, float(d2[t]), dist[s])
        dist = np.minimum(dist, ((p - p[s]) ** 2).sum(-1))
        dist[s] = -np.inf


def cells(points, voxel):
    """f32 (n,3) -> int64 (n,3) cells (cx, cy, cz): floor((double(x) - double(lo)) / double(voxel)), lo the f32 minimum per axis"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    return np.floor((p.astype(np.float64) - p.min(0).astype(np.float64)) / np.float64(voxel)).astype(np.int64)


def voxel_down(points, voxel, pick="centroid"):
    """The contract of voxel_downsample_dev for one set -> out (m,3) f32, first (m,) int32, count (m,) int32, the voxels ascending in
    (cz, cy, cx).  Centroids: math.fsum (the correctly rounded sum) / count, rounded to f32."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    c = cells(p, voxel)
    assert c.min() >= 0 and c.max() < 65536
    key = (c[:, 2] * 65536 + c[:, 1]) * 65536 + c[:, 0]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    ends = np.concatenate([starts[1:], [len(p)]])
    first, count = order[starts].astype(np.int32), (ends - starts).astype(np.int32)
    if pick == "first":
        return p[first], first, count
    p64 = p.astype(np.float64)
    out = np.array([[math.fsum(p64[order[s:e], a]) / (e - s) for a in range(3)] for s, e in zip(starts, ends)], np.float64)
    return out.astype(np.float32), first, count


def voxel_brute(points, voxel):
    """the definition with a dictionary: {(cz, cy, cx): ascending list of indices}, sorted by cell"""
    table = {}
    for i, (cx, cy, cz) in enumerate(cells(points, voxel)):
        table.setdefault((int(cz), int(cy), int(cx)), []).append(i)
    return [table[k] for k in sorted(table)]


def ulps(a, b):
    """distance in f32 steps between two f32 arrays of finite values"""
    def lin(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(lin(a) - lin(b))


def dyadic(rs, n):
    """integers in [-512, 512] / 1024 as f32: every difference, square and sum of three squares is exact in f32, and ties abound"""
    return (rs.randint(-512, 513, (n, 3)) / 1024.0).astype(np.float32)


def two_density(seed):
    """a sphere of radius 0.5 scanned at two densities (12 000 points on x > 0, 600 on x <= 0, jitter 0.002) and 20 planted outliers
    at radius 0.8 - 1.0, after them -> (12620, 3) f32"""
    rs = np.random.RandomState(seed)
    sph = lambda n: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rs.randn(n, 3))
    a = sph(40000); a = a[a[:, 0] > 0][:12000]
    b = sph(4000);  b = b[b[:, 0] <= 0][:600]
    s = np.concatenate([a, b]) * 0.5 + rs.randn(12600, 3) * 0.002
    out = sph(20) * rs.uniform(0.8, 1.0, (20, 1))
    p = np.concatenate([s, out]).astype(np.float32)
    return p
