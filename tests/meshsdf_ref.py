"""f64 restatement of mesh signed distance for the meshsdf tests: closest point on a triangle (Ericson, Real-Time Collision
Detection 5.1.5), van Oosterom-Strackee solid angle, and brute-force S, I, C, W over every (query, face) pair.  A face whose
area is zero (repeated vertex, collinear vertices) is the union of its three edges here: its closest point is the nearest of
their closest points."""
import numpy as np


def closest_on_segment(p, a, b):
    """p (..., 3), segment a -> b (..., 3) -> closest point (..., 3); a zero-length segment gives a."""
    ab = b - a
    den = (ab * ab).sum(-1)
    t = np.where(den > 0, ((p - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0)
    return a + np.clip(t, 0.0, 1.0)[..., None] * ab


def closest_on_triangle(p, a, b, c):
    """Ericson's region form, vectorised over broadcast (..., 3) arrays, in f64."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    dot = lambda x, y: (x * y).sum(-1)
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = p - b
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = p - c
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    sd = lambda x, y: x / np.where(y != 0, y, 1.0)
    den = va + vb + vc
    v, w = sd(vb, den), sd(vc, den)                                  # interior (lowest priority)
    for cond, vv, ww in [
            ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), 1 - sd(d4 - d3, (d4 - d3) + (d5 - d6)), sd(d4 - d3, (d4 - d3) + (d5 - d6))),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), 0.0, sd(d2, d2 - d6)),
            ((d6 >= 0) & (d5 <= d6), 0.0, 1.0),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), sd(d1, d1 - d3), 0.0),
            ((d3 >= 0) & (d4 <= d3), 1.0, 0.0),
            ((d1 <= 0) & (d2 <= 0), 0.0, 0.0)]:
        v, w = np.where(cond, vv, v), np.where(cond, ww, w)
    C = a + v[..., None] * ab + w[..., None] * ac
    cr = np.cross(ab, ac)
    degen = (cr * cr).sum(-1) == 0
    if degen.any():
        E = np.stack([closest_on_segment(p, a, b), closest_on_segment(p, b, c), closest_on_segment(p, c, a)])
        k = ((p[None] - E) ** 2).sum(-1).argmin(0)
        Ce = np.take_along_axis(E, k[None, ..., None], 0)[0]
        C = np.where(degen[..., None], Ce, C)
    return C


def solid_angle(p, a, b, c):
    """van Oosterom-Strackee: Omega = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), a, b, c relative to p."""
    a, b, c = (np.asarray(x, np.float64) - np.asarray(p, np.float64) for x in (a, b, c))
    la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (a, b, c))
    det = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return 2 * np.arctan2(det, den)


def brute(q, vert, face, chunk=256):
    """q (N,3), vert (V,3), face (T,3) -> dict S, I, C, W, d2 (closest), d2_second (second-closest face's distance), all f64."""
    q, vert = np.asarray(q, np.float64), np.asarray(vert, np.float64)
    A, B, Cc = (vert[face[:, k]] for k in range(3))
    out = {k: [] for k in ("S", "I", "C", "W", "d2", "d2_second")}
    for s in range(0, len(q), chunk):
        p = q[s:s + chunk, None, :]
        C = closest_on_triangle(p, A[None], B[None], Cc[None])             # (n, T, 3)
        d2 = ((p - C) ** 2).sum(-1)
        I = d2.argmin(1)
        srt = np.sort(d2, 1)
        W = solid_angle(p, A[None], B[None], Cc[None]).sum(1) / (4 * np.pi)
        best = srt[:, 0]
        out["I"].append(I)
        out["C"].append(C[np.arange(len(I)), I])
        out["d2"].append(best)
        out["d2_second"].append(srt[:, 1] if srt.shape[1] > 1 else np.full(len(I), np.inf))
        out["W"].append(W)
        out["S"].append(np.where(np.abs(W) > 0.5, -1.0, 1.0) * np.sqrt(best))
    return {k: np.concatenate(v) for k, v in out.items()}


def box_sdf(q, half=(1.0, 1.0, 1.0)):
    """geoutil.boxSDF (xgutils/geoutil.py:422-436) about the origin."""
    d = np.abs(np.asarray(q, np.float64)) - np.asarray(half, np.float64)[None]
    m = d.max(-1)
    return np.linalg.norm(d * (d > 0), axis=-1) + m * (m < 0)


# the reference's 12-triangle cube (xgutils/geoutil.py:493-498), consistently oriented
CUBE_V = np.array([[1, 1, 1], [-1, 1, 1], [-1, -1, 1], [1, -1, 1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, -1.0]])
CUBE_F = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 6], [0, 6, 1], [1, 6, 7], [1, 7, 2], [7, 4, 3], [7, 3, 2],
                   [4, 7, 6], [4, 6, 5]])


def icosphere(level=2, r=1.0):
    """Subdivided icosahedron on the sphere of radius r, outward-oriented faces."""
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1],
         [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = nf
    return np.array(v) * r, np.array(f)
