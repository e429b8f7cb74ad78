"""Consistent orientation of unoriented normals, the numpy statement of the contract of include/sfmi.h (csrc/tangent.hip, DESIGN.md
§5.21): the k-nearest-neighbour graph, its weights in f64, the strict total order (bits of w, lo, hi), the minimum spanning forest by
Kruskal over the sorted keys, parity by traversal of the forest, the integer vote.  A Boruvka restatement gives the same forest and
counts the rounds (informational).  Plain sequential code: no schedule to depend on.  The scene generators of the tests live here too.
"""
from __future__ import annotations

import numpy as np


# ---- the graph ------------------------------------------------------------------------------------------------------------------------

def alive_mask(normal):
    n = np.asarray(normal, np.float32)
    return np.isfinite(n).all(1) & (n != 0).any(1)


def dot64(a, b):
    """(ax bx + ay by) + az bz with the f32 components widened to f64 (the products are exact)"""
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def graph_edges(normal, idx):
    """One set: normal (n,3) f32, idx (n,k) int local -> lo, hi (E,) int64, bits (E,) uint64, flip (E,) bool, sorted ascending in
    (bits, lo, hi).  {i,j} is an edge when j is in row i or i in row j, both alive; entries < 0, >= n, == i are skipped; one edge per
    pair."""
    n = len(normal)
    idx = np.asarray(idx, np.int64).reshape(n, np.shape(idx)[-1])             # (0,k) for an empty set
    live = alive_mask(normal)
    i = np.repeat(np.arange(n, dtype=np.int64), idx.shape[1])
    j = idx.reshape(-1)
    ok = (j >= 0) & (j < n) & (j != i)
    i, j = i[ok], j[ok]
    ok = live[i] & live[j]
    i, j = i[ok], j[ok]
    key = np.unique(np.minimum(i, j) * max(n, 1) + np.maximum(i, j))
    lo, hi = key // max(n, 1), key % max(n, 1)
    d = dot64(normal[lo], normal[hi]) if len(lo) else np.zeros(0)
    w = np.maximum(0.0, 1.0 - np.abs(d))
    bits = np.ascontiguousarray(w).view(np.uint64)
    order = np.lexsort((hi, lo, bits))
    return lo[order], hi[order], bits[order], (d < 0)[order]


class _UF:
    def __init__(self, n):
        self.p = list(range(n))

    def find(self, v):
        p = self.p
        while p[v] != v:
            p[v] = p[p[v]]
            v = p[v]
        return v

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.p[max(a, b)] = min(a, b)                  # the root is the smallest index of its tree
        return True


def kruskal(n, lo, hi):
    """edges sorted by the total order -> bool (E,): the edges of the minimum spanning forest"""
    uf = _UF(n)
    take = np.zeros(len(lo), bool)
    for e in range(len(lo)):
        take[e] = uf.union(int(lo[e]), int(hi[e]))
    return take


def boruvka(n, lo, hi):
    """the same forest by Boruvka rounds (the rank of an edge in the sorted list is its key) -> (bool (E,), rounds that did work,
    the longest hook chain of any round)"""
    E = len(lo)
    label = np.arange(n)
    take = np.zeros(E, bool)
    rank = np.arange(E)
    rounds, longest = 0, 0
    while True:
        out = label[lo] != label[hi]
        if not out.any():
            return take, rounds, longest
        best = np.full(n, E)
        np.minimum.at(best, label[lo[out]], rank[out])
        np.minimum.at(best, label[hi[out]], rank[out])
        roots = np.nonzero(best < E)[0]
        take[best[roots]] = True
        parent = np.arange(n)
        for c in roots:                                # the hook rule of the kernel: a mutual pair keeps its smaller root
            e = best[c]
            a, b = label[lo[e]], label[hi[e]]
            o = b if a == c else a
            if not (best[o] == e and c < o):
                parent[c] = o
        new = np.arange(n)
        for c in np.nonzero(label == np.arange(n))[0]:
            r, steps = c, 0
            while parent[r] != r:
                r = parent[r]
                steps += 1
                assert steps <= n, "cycle among the hooks"
            new[c] = r
            longest = max(longest, steps)
        label = new[label]
        rounds += 1


def forest_outputs(n, lo, hi, flip, take):
    """-> component (n,) int32 (the smallest index of the vertex's tree), parity (n,) uint8 (XOR of flip along the tree path to it)"""
    adj = [[] for _ in range(n)]
    for e in np.nonzero(take)[0]:
        a, b, f = int(lo[e]), int(hi[e]), int(flip[e])
        adj[a].append((b, f))
        adj[b].append((a, f))
    component = np.full(n, -1, np.int32)
    parity = np.zeros(n, np.uint8)
    for s in range(n):                                 # ascending: the first vertex met of a tree is its smallest
        if component[s] >= 0:
            continue
        component[s] = s
        stack = [s]
        while stack:
            v = stack.pop()
            for u, f in adj[v]:
                if component[u] < 0:
                    component[u] = s
                    parity[u] = parity[v] ^ f
                    stack.append(u)
    return component, parity


def vote(points, normal, component, parity, anchor, ref):
    """One set.  anchor "outward": d = p - ref (the centroid); "viewpoint": d = ref - p.  -> votes (n,2) int32 at the component's row,
    negate (n,) bool per vertex (its tree's decision), margin = min |m . d| over the voters (inf without one)"""
    n = len(points)
    p = np.asarray(points, np.float32).astype(np.float64)
    m = np.asarray(normal, np.float32).astype(np.float64) * np.where(parity != 0, -1.0, 1.0)[:, None]
    d = p - ref[None] if anchor == "outward" else ref[None] - p
    with np.errstate(invalid="ignore"):
        t = (m[:, 0] * d[:, 0] + m[:, 1] * d[:, 1]) + m[:, 2] * d[:, 2]
        live = alive_mask(normal)
        pos, neg = live & (t > 0), live & (t < 0)
    votes = np.zeros((n, 2), np.int32)
    np.add.at(votes[:, 0], component[pos], 1)
    np.add.at(votes[:, 1], component[neg], 1)
    voters = pos | neg
    margin = float(np.abs(t[voters]).min()) if voters.any() else float("inf")
    return votes, (votes[:, 1] > votes[:, 0])[component], margin


def centroid(points):
    """the mean of the finite points in f64 (NaN without one).  The device sums in another fixed order: the callers assert a margin
    (|m . d| >= 1e-9) under which the last bits of the centroid cannot decide a vote"""
    p = np.asarray(points, np.float32).astype(np.float64)
    ok = np.isfinite(p).all(1)
    return p[ok].sum(0) / ok.sum() if ok.any() else np.full(3, np.nan)


def orient(points, normal, idx, off=None, anchor="outward", viewpoint=None, with_boruvka=False):
    """The whole contract for a ragged batch: points, normal (N,3), idx (N,k) local, off (B+1,).  -> dict: normal (N,3) f32, component
    (N,), parity (N,), tree: a list of B sets of (lo, hi), votes (N,2), n_components (B,), margin (the smallest |m . d| of any
    voter), and with_boruvka: rounds (B,), chain (B,) the longest hook chain, after asserting Boruvka == Kruskal."""
    points, normal = np.asarray(points, np.float32), np.asarray(normal, np.float32)
    N = len(points)
    off = np.array([0, N], np.int64) if off is None else np.asarray(off, np.int64)
    B = len(off) - 1
    idx = np.asarray(idx).reshape(N, -1)
    view = None if viewpoint is None else np.asarray(viewpoint, np.float64).reshape(B, 3)
    out = {"normal": normal.copy(), "component": np.zeros(N, np.int32), "parity": np.zeros(N, np.uint8), "tree": [],
           "votes": np.zeros((N, 2), np.int32), "n_components": np.zeros(B, np.int32), "margin": float("inf"),
           "rounds": np.zeros(B, np.int32), "chain": np.zeros(B, np.int32)}
    for b in range(B):
        s = slice(int(off[b]), int(off[b + 1]))
        n = s.stop - s.start
        lo, hi, bits, flip = graph_edges(normal[s], idx[s])
        take = kruskal(n, lo, hi)
        if with_boruvka:
            take_b, out["rounds"][b], out["chain"][b] = boruvka(n, lo, hi)
            assert np.array_equal(take, take_b), "Boruvka and Kruskal disagree"
        comp, par = forest_outputs(n, lo, hi, flip, take)
        out["tree"].append(set(zip(lo[take].tolist(), hi[take].tolist())))
        out["component"][s], out["parity"][s] = comp, par
        out["n_components"][b] = int((comp == np.arange(n)).sum())
        ref = centroid(points[s]) if anchor == "outward" else view[b]
        votes, negate, margin = vote(points[s], normal[s], comp, par, anchor, ref)
        out["votes"][s] = votes
        out["margin"] = min(out["margin"], margin)
        turn = (par != 0) != negate
        out["normal"][s] = np.where(turn[:, None], -normal[s], normal[s])
    return out


# ---- host kNN and PCA normals for the CPU tests (the GPU tests hand the device's own table and normals to `orient`) ------------------

def knn_table(points, k):
    """(n,k) int32: the k nearest points, the point itself included (scipy's order among ties)"""
    from scipy.spatial import cKDTree
    p = np.asarray(points, np.float64)
    return cKDTree(p).query(p, k=min(k, len(p)))[1].reshape(len(p), -1).astype(np.int32)


def pca_normals(points, idx):
    """the eigenvector of the smallest eigenvalue of each neighbourhood's covariance; the component of largest magnitude positive"""
    p = np.asarray(points, np.float64)
    q = p[idx]
    q = q - q.mean(1, keepdims=True)
    _, v = np.linalg.eigh(np.einsum("nki,nkj->nij", q, q))
    nrm = v[:, :, 0]
    big = np.take_along_axis(nrm, np.abs(nrm).argmax(1)[:, None], 1)
    return (nrm * np.where(big < 0, -1.0, 1.0)).astype(np.float32)


# ---- scenes: points f32 and, where there is one, the analytic outward normal ------------------------------------------------------------

def sphere(n, radius=0.5, centre=(0.0, 0.0, 0.0), seed=0):
    """a Fibonacci sphere with a little seeded jitter along the surface -> points (n,3) f32, outward (n,3) f64"""
    rng = np.random.default_rng(seed)
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    u = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    u = u + rng.normal(scale=0.2 / np.sqrt(n), size=u.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p = (np.asarray(centre, np.float64)[None] + radius * u).astype(np.float32)
    return p, u


def torus(n, R=0.5, r=0.2, seed=0):
    """a jittered (u, v) lattice on the torus around z -> points (n,3) f32, outward (n,3) f64"""
    rng = np.random.default_rng(seed)
    nv = max(3, int(round(np.sqrt(n * r / R))))
    nu = -(-n // nv)
    g = np.stack(np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij"), -1).reshape(-1, 2)[:n].astype(np.float64)
    g += rng.uniform(-0.3, 0.3, g.shape)
    u, v = 2 * np.pi * g[:, 0] / nu, 2 * np.pi * g[:, 1] / nv
    out = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], 1)
    p = np.stack([R * np.cos(u), R * np.sin(u), np.zeros_like(u)], 1) + r * out
    return p.astype(np.float32), out


def thin_box(n, half=(0.5, 0.3, 0.05), seed=0):
    """uniform random points on the surface of an axis-aligned box -> points (n,3) f32.  Its faces are planes of constant coordinate, so
    PCA normals there are exact axes and thousands of edges weigh exactly 0: the tie-break case"""
    rng = np.random.default_rng(seed)
    h = np.asarray(half, np.float64)
    area = np.array([h[1] * h[2], h[0] * h[2], h[0] * h[1]])
    axis = rng.choice(3, size=n, p=area / area.sum())
    p = rng.uniform(-1, 1, (n, 3)) * h[None]
    p[np.arange(n), axis] = np.where(rng.random(n) < 0.5, -1.0, 1.0) * h[axis]
    return p.astype(np.float32)


def lattice(m=32, seed=0):
    """an m x m planar lattice with normals (0,0,+-1) of random sign: every edge weighs exactly 0, so (lo, hi) alone orders them
    -> points (m m,3) f32, normals (m m,3) f32"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
    p = np.concatenate([g / float(m), np.zeros((m * m, 1))], 1).astype(np.float32)
    nrm = np.zeros((m * m, 3), np.float32)
    nrm[:, 2] = np.where(rng.random(m * m) < 0.5, -1.0, 1.0)
    return p, nrm


def chain(n=1000, seed=0):
    """a hand-made path graph: row i = (i - 1, i + 1) (-1 past the ends); normals (cos t_i, sin t_i, 0), t_i = sum_{j <= i} 0.001 (j + 1),
    times random signs, so the weights strictly increase along the chain (asserted): one Boruvka round hooks the whole chain
    -> points (n,3) f32, normals (n,3) f32, idx (n,2) int32, the signs (n,)"""
    rng = np.random.default_rng(seed)
    t = np.cumsum(0.001 * (np.arange(n) + 1.0))
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    nrm = (np.stack([np.cos(t), np.sin(t), np.zeros(n)], 1) * sign[:, None]).astype(np.float32)
    idx = np.stack([np.arange(n) - 1, np.arange(n) + 1], 1).astype(np.int32)
    idx[idx >= n] = -1
    w = np.maximum(0.0, 1.0 - np.abs(dot64(nrm[:-1], nrm[1:])))
    assert (np.diff(w) > 0).all(), "the chain's weights must strictly increase"
    p = np.stack([np.cos(t), np.sin(t), np.zeros(n)], 1).astype(np.float32)
    return p, nrm, idx, sign


def two_spheres(n0=1024, n1=512):
    """radii 0.25 and 0.2, centres (-0.5,0,0) and (0.5,0.1,0), one set -> points (n0 + n1,3) f32, outward (n0 + n1,3) f64"""
    p0, u0 = sphere(n0, 0.25, (-0.5, 0.0, 0.0), seed=1)
    p1, u1 = sphere(n1, 0.2, (0.5, 0.1, 0.0), seed=2)
    return np.concatenate([p0, p1]), np.concatenate([u0, u1])


def hemisphere(n, radius=0.5, viewpoint=(0.0, 0.0, 2.0), seed=0):
    """the side of sphere(n) that a camera at `viewpoint` sees: the points whose outward normal u has u . (v - p) > 0.05 (a cap a little
    short of the silhouette; behind it the outward normal points away from the camera) -> points f32, outward f64"""
    p, u = sphere(n, radius, seed=seed)
    keep = (u * (np.asarray(viewpoint, np.float64)[None] - p)).sum(1) > 0.05
    return p[keep], u[keep]
