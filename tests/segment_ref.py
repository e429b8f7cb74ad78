"""numpy statement of the contracts of csrc/segment.hip: plane scoring, plane refit, Euclidean clusters, the
hypothesis draws, the upright rotation, and the test scene."""
from __future__ import annotations

import numpy as np


def mix64(x):
    """sfmi_mix64 (csrc/sfmi_ragged.h) on uint64 arrays"""
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def plane_hypotheses(sizes, H, seed=0):
    """(B,H,3) int32: index = mix64((seed << 40) + 4 h + slot) mod n_b, written as loops over python ints"""
    sizes = [int(n) for n in np.asarray(sizes).reshape(-1)]
    out = np.zeros((len(sizes), H, 3), np.int32)
    for h in range(H):
        for slot in range(3):
            r = int(mix64(np.array([((int(seed) << 40) + 4 * h + slot) & 0xFFFFFFFFFFFFFFFF], np.uint64))[0])
            for b, n in enumerate(sizes):
                out[b, h, slot] = r % n if n > 0 else 0
    return out


def triple_plane(p, t):
    """p (n,3) f32, t three local indices -> (n (3,) f64, d, nn, valid): every product and sum rounded on its own, in the written order"""
    n_pts = p.shape[0]
    i0, i1, i2 = (int(v) for v in t)
    if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= n_pts or i0 == i1 or i0 == i2 or i1 == i2:
        return np.zeros(3), 0.0, 0.0, False
    with np.errstate(all="ignore"):
        p0, p1, p2 = (p[i].astype(np.float64) for i in (i0, i1, i2))
        u, v = p1 - p0, p2 - p0
        n = np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
        nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
        d = (n[0] * p0[0] + n[1] * p0[1]) + n[2] * p0[2]
    return n, d, nn, bool(nn > 0)


def seed_inliers(p, n, d, nn, thr):
    x = p.astype(np.float64)
    with np.errstate(all="ignore"):
        s = ((n[0] * x[:, 0] + n[1] * x[:, 1]) + n[2] * x[:, 2]) - d
        return s * s <= (np.float64(thr) * np.float64(thr)) * nn


def plane_score_set(p, triples, thr):
    """one set: p (n,3) f32, triples (H,3) -> count (H,) int32, best, status"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    H = triples.shape[0]
    count = np.full(H, -1, np.int32)
    if not np.isfinite(p).all():
        return count, -1, 2
    for h in range(H):
        n, d, nn, ok = triple_plane(p, triples[h])
        if ok:
            count[h] = int(seed_inliers(p, n, d, nn, thr).sum())
    if (count < 0).all():
        return count, -1, 1
    return count, int(np.argmax(count)), 0            # argmax: the first (lowest h) among equal counts


def plane_score(points, off, triples, thr):
    B = len(off) - 1
    res = [plane_score_set(points[off[b]:off[b + 1]], triples[b], thr) for b in range(B)]
    return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], np.int32))


def plane_refit_set(p, triple, thr, up=None):
    """one set, seeded by a triple -> plane (4,) f64, mask (n,) bool, n_in, signed distances (n,) f64 to the refit plane, eigen-gap
    (l1 - l0) / l2"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    n, d, nn, ok = triple_plane(p, triple)
    return plane_refit_seed(p, n, d, nn, thr, up, ok)


def plane_refit_seed(p, n, d, nn, thr, up=None, ok=True):
    """the refit from the seed plane n . x = d with nn = |n|^2 (a (n, dd) plane has d = -dd)"""
    p = np.asarray(p, np.float32).reshape(-1, 3)
    fail = (np.full(4, np.nan), np.zeros(len(p), bool), 0, np.full(len(p), np.nan), np.nan)
    if not ok or not nn > 0 or not np.isfinite([nn, d]).all() or not np.isfinite(p).all():
        return fail
    m = seed_inliers(p, n, d, nn, thr)
    if m.sum() < 3:
        return fail
    x = p[m].astype(np.float64)
    c = x.mean(0)
    y = x - c
    lam, vec = np.linalg.eigh(y.T @ y / len(x))
    e = vec[:, 0]
    e = e / np.linalg.norm(e)
    if up is not None:
        flip = e @ np.asarray(up, np.float64) < 0
    else:
        flip = e[int(np.argmax(np.abs(e)))] < 0
    e = -e if flip else e
    dd = -(e @ c)
    dist = p.astype(np.float64) @ e + dd
    mask = np.abs(dist) <= thr
    return np.concatenate([e, [dd]]), mask, int(mask.sum()), dist, (lam[1] - lam[0]) / lam[2]


def _fmaf(a, b, c):
    """fmaf on f32 arrays: the product is exact in f64, one f64 add, one rounding to f32 (as tests/downsample_ref.py)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def d2_matrix_rows(p, i0, i1):
    """(i1 - i0, n) f32: fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with f32 differences, points i0..i1 against every point"""
    with np.errstate(all="ignore"):
        d = p[i0:i1, None, :] - p[None, :, :]
        return _fmaf(d[..., 2], d[..., 2], _fmaf(d[..., 1], d[..., 1], d[..., 0] * d[..., 0]))


def cluster_roots(p, radius):
    """one set -> root (n,) int32: the lowest index of each point's connected component of the graph d2 <= f32(radius^2)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    p = np.asarray(p, np.float32).reshape(-1, 3)
    n = len(p)
    if n == 0:
        return np.zeros(0, np.int32)
    r2 = np.float32(float(radius) ** 2)
    rows, cols = [], []
    for i0 in range(0, n, 1024):                      # row blocks: the full matrix of 4100 points would be 200 MB of temporaries
        d2 = d2_matrix_rows(p, i0, min(i0 + 1024, n))
        with np.errstate(invalid="ignore"):
            i, j = np.nonzero(d2 <= r2)
        rows.append(i + i0)
        cols.append(j)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    _, lab = connected_components(csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n, n)), directed=False)
    first = np.full(lab.max() + 1, n, np.int64)
    np.minimum.at(first, lab, np.arange(n))
    return first[lab].astype(np.int32)


def cluster_labels(root, min_points=1):
    """one set: root (n,) -> label (n,) int32 rank under (size descending, root ascending), -1 below min_points; sizes of the kept"""
    roots, inv, cnt = np.unique(root, return_inverse=True, return_counts=True)
    order = np.lexsort((roots, -cnt))
    order = order[cnt[order] >= min_points]
    rank = np.full(len(roots), -1, np.int32)
    rank[order] = np.arange(len(order), dtype=np.int32)
    return rank[inv].astype(np.int32), cnt[order].astype(np.int32)


def upright_rotation(normal, up=(0, 1, 0)):
    """180 degrees about the bisector of the unit vectors (geoutil.rotation_v1tov2): R = 2 a a^T - I; one vector, (3,3) f64"""
    v = np.asarray(normal, np.float64)
    u = np.asarray(up, np.float64)
    v, u = v / np.linalg.norm(v), u / np.linalg.norm(u)
    a = v + u
    if np.linalg.norm(a) <= 1e-8:
        e = np.eye(3)[[k for k in range(3) if np.linalg.norm(np.cross(np.eye(3)[k], u)) > 1e-12][0]]
        a = e - (e @ u) * u
    a = a / np.linalg.norm(a)
    return 2.0 * np.outer(a, a) - np.eye(3)


def scene(seed, n_plane=3000, n_sphere=1000, n_out=100):
    """A jittered plane at y = -0.4, a sphere shell of radius 0.3 about the origin, uniform outliers; permuted, f32.
    -> points (n,3) f32, kind (n,) int8: 0 plane, 1 sphere, 2 outlier"""
    rng = np.random.default_rng(seed)
    pl = np.stack([rng.uniform(-0.8, 0.8, n_plane), -0.4 + rng.normal(0, 0.002, n_plane), rng.uniform(-0.8, 0.8, n_plane)], 1)
    s = rng.normal(size=(n_sphere, 3))
    sp = 0.3 * s / np.linalg.norm(s, axis=1, keepdims=True)
    out = rng.uniform(-0.9, 0.9, (n_out, 3))
    p = np.concatenate([pl, sp, out]).astype(np.float32)
    kind = np.concatenate([np.zeros(n_plane, np.int8), np.ones(n_sphere, np.int8), np.full(n_out, 2, np.int8)])
    perm = rng.permutation(len(p))
    return p[perm], kind[perm]
