"""Numpy statement of the mesh connected-components contract (include/sfmi.h): a plain sequential union-find, no
device.  One shape at a time; a batch is its shapes one after the other.

  status_of(verts, faces)                         0 ok, 1 no vertices, 2 a face index outside the shape, 3 a non-finite vertex
  labels(n_vert, faces)                           -> vlabel (V), flabel (T), C: numbered by the components' smallest vertex index
  face_terms(verts, faces)                        -> area terms, volume terms (T) f64, without fused multiply-adds
  stats(verts, faces, vlabel, flabel, C)          -> dict n_vert, n_face (int32), area, volume (f64), abs_area, abs_volume (sum |term|)
  select(stats, top, min_share, by)               -> kept (C) bool
  compact(verts, faces, vlabel, flabel, kept)     -> verts, faces
  components(verts, faces)                        -> vlabel, flabel, stats, status
  keep(verts, faces, top, min_share, by)          -> verts, faces, status, kept
  batch(fn, verts, faces, voff, toff, ...)        per-shape calls of fn over a ragged batch

The sums are plain f64 sums in face order; the device adds the same terms over a fixed tree, which the tolerance of
tests/test_components_gpu.py accounts for.
"""
import numpy as np


def status_of(verts, faces):
    v, f = np.asarray(verts).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    if len(v) == 0:
        return 1
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        return 2
    if not np.isfinite(v).all():
        return 3
    return 0


def _find(parent, v):
    while parent[v] != v:
        parent[v] = parent[parent[v]]
        v = parent[v]
    return v


def labels(n_vert, faces):
    """Two vertices are connected if one face names both (a degenerate face (a, a, b) still connects a and b); a vertex no face names
    gets -1.  Components are numbered in ascending order of their smallest vertex index; a face carries the label of its first index."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    parent = list(range(n_vert))
    ref = np.zeros(n_vert, bool)
    for a, b, c in f.tolist():
        ref[[a, b, c]] = True
        for u, w in ((a, b), (a, c)):
            ru, rw = _find(parent, u), _find(parent, w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)          # the smaller index stays the root
    root = np.array([_find(parent, v) for v in range(n_vert)], np.int64).reshape(-1)
    isroot = ref & (root == np.arange(n_vert))
    ids = np.cumsum(isroot) - 1                            # rank among the roots = rank of the component's smallest vertex
    vlabel = np.where(ref, ids[root] if n_vert else ids, -1).astype(np.int32)
    flabel = vlabel[f[:, 0]].astype(np.int32) if len(f) else np.zeros(0, np.int32)
    return vlabel, flabel, int(isroot.sum())


def face_terms(verts, faces):
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(b - a, c - a)
    area = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2]) * 0.5
    x = np.cross(b, c)
    vol = (a[:, 0] * x[:, 0] + a[:, 1] * x[:, 1] + a[:, 2] * x[:, 2]) / 6.0
    return area, vol


def stats(verts, faces, vlabel, flabel, C):
    area_t, vol_t = face_terms(verts, faces)
    out = dict(n_vert=np.bincount(vlabel[vlabel >= 0], minlength=C).astype(np.int32),
               n_face=np.bincount(flabel, minlength=C).astype(np.int32))
    for name, t in (("area", area_t), ("volume", vol_t)):
        out[name] = np.array([t[flabel == c].sum() for c in range(C)], np.float64)
        out["abs_" + name] = np.array([np.abs(t[flabel == c]).sum() for c in range(C)], np.float64)
    return out


def measure(st, by):
    return {"area": st["area"], "faces": st["n_face"].astype(np.float64), "volume": np.abs(st["volume"])}[by]


def select(st, top=None, min_share=0.0, by="area"):
    """Ranked by measure, descending, equal measures by ascending id; kept: rank < top (when top is not None) and measure >= min_share
    times the largest measure, in f64."""
    m = measure(st, by)
    C = len(m)
    if C == 0:
        return np.zeros(0, bool)
    order = sorted(range(C), key=lambda c: (-m[c], c))
    rank = np.empty(C, np.int64)
    rank[order] = np.arange(C)
    kept = m >= np.float64(min_share) * m.max()
    if top is not None:
        kept &= rank < top
    return kept


def compact(verts, faces, vlabel, flabel, kept):
    """the obvious mask-and-renumber: kept vertices and faces in input order, unreferenced vertices dropped"""
    v, f = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    vk = np.array([l >= 0 and kept[l] for l in vlabel], bool).reshape(-1)
    fk = np.array([kept[l] for l in flabel], bool).reshape(-1)
    new = np.cumsum(vk) - 1
    return v[vk], new[f[fk].astype(np.int64)].astype(np.int32).reshape(-1, 3)


def components(verts, faces):
    v, f = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    s = status_of(v, f)
    if s:
        return np.full(len(v), -1, np.int32), np.full(len(f), -1, np.int32), stats(v, f[:0], np.zeros(0, np.int32), np.zeros(0, np.int32), 0), s
    vl, fl, C = labels(len(v), f)
    return vl, fl, stats(v, f, vl, fl, C), 0


def keep(verts, faces, top=None, min_share=0.0, by="area"):
    v, f = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    vl, fl, st, s = components(v, f)
    if s:
        return v[:0], f[:0], s, np.zeros(0, bool)
    kept = select(st, top, min_share, by)
    return (*compact(v, f, vl, fl, kept), 0, kept)


def batch(fn, verts, faces, voff, toff, *a, **k):
    return [fn(verts[voff[b]:voff[b + 1]], faces[toff[b]:toff[b + 1]], *a, **k) for b in range(len(voff) - 1)]


# ---- fixtures shared by the CPU and the GPU tests (seeded; nothing is read from disk)

def small_meshes():
    """name -> (verts, faces, components): the five hand cases of the issue"""
    rng = np.random.default_rng(5)
    v = lambda n: rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    f = lambda *t: np.array(t, np.int32).reshape(-1, 3)
    return {"one": (v(3), f((0, 1, 2)), 1),
            "disjoint": (v(6), f((0, 1, 2), (3, 4, 5)), 2),
            "shared_vertex": (v(5), f((0, 1, 2), (2, 3, 4)), 1),
            "shared_edge": (v(4), f((0, 1, 2), (2, 1, 3)), 1),
            "repeated": (v(3), f((0, 1, 2), (0, 1, 2)), 1)}


def strip(n_tri, numbering, seed=0):
    """a strip of n_tri triangles in one component: triangle i on strip positions i, i+1, i+2; vertex indices ascending along the strip,
    descending or randomly permuted; face order shuffled"""
    rng = np.random.default_rng(seed)
    n = n_tri + 2
    pos = np.stack([np.arange(n) / n * 2 - 1, (np.arange(n) % 2) * 0.1, np.zeros(n)], 1).astype(np.float32)
    index = {"ascending": np.arange(n), "descending": np.arange(n)[::-1].copy(), "permuted": rng.permutation(n)}[numbering]
    verts = np.empty_like(pos)
    verts[index] = pos
    i = np.arange(n_tri)
    faces = np.stack([index[i], index[i + 1], index[i + 2]], 1).astype(np.int32)
    return verts, faces[rng.permutation(n_tri)]


def tetrahedra(n, seed=1):
    """n tetrahedra (0, s e0, s e1, s e2) + centre that share no vertex, oriented outward, sizes s distinct, vertices and faces randomly
    permuted -> verts, faces, tet of every vertex, volume of every tet from its placed corners, and s^3 / 6.  Every coordinate is a
    multiple of 2^-14 below 1, so the triple products of the face terms are exact in f64: each term is rounded once, by its division."""
    rng = np.random.default_rng(seed)
    assert n <= 1024
    s = ((16 + rng.permutation(n)) / 2.0 ** 14).astype(np.float32)         # distinct, in [0.001, 0.064)
    ctr = (rng.integers(-14000, 14000, (n, 3)) / 2.0 ** 14).astype(np.float32)
    corner = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    pos = (ctr[:, None, :] + s[:, None, None] * corner[None]).reshape(-1, 3).astype(np.float32)
    tri = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)  # outward
    faces = (4 * np.arange(n)[:, None, None] + tri[None]).reshape(-1, 3)
    perm = rng.permutation(4 * n)                                           # new index of old vertex i = perm[i]
    verts = np.empty_like(pos)
    verts[perm] = pos
    tet_of = np.empty(4 * n, np.int64)
    tet_of[perm] = np.repeat(np.arange(n), 4)
    faces = perm[faces][rng.permutation(4 * n)].astype(np.int32)
    # the exact volume of the f32 vertices as placed, in f64 (the corner products of the translated tetrahedron)
    p = verts.astype(np.float64)
    vol = np.empty(n)
    for t in range(n):
        q = pos[4 * t:4 * t + 4].astype(np.float64)
        vol[t] = np.dot(q[1] - q[0], np.cross(q[2] - q[0], q[3] - q[0])) / 6.0
    s64 = s.astype(np.float64)
    return verts, faces, tet_of, vol, s64 * s64 * s64 / 6.0


def sphere_field(Q=33):
    """the 33^3 lattice fields of the issue over [-1,1]^3: f_i = clip(0.5 + 8 (r_i - |x - c_i|), 0, 1) for a large sphere at the origin and
    two small ones whose supports (r_i + 1/16) are disjoint from it and from each other -> (f_0, max(f_0, f_1, f_2)) float32 (Q,Q,Q)"""
    g = np.linspace(-1.0, 1.0, Q)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1)
    spheres = [((0.0, 0.0, 0.0), 0.45), ((0.75, 0.7, 0.72), 0.08), ((-0.72, -0.7, 0.74), 0.08)]
    fs = [np.clip(0.5 + 8.0 * (r - np.linalg.norm(x - np.array(c), axis=-1)), 0.0, 1.0).astype(np.float32) for c, r in spheres]
    for i in range(3):
        for j in range(i + 1, 3):
            d = np.linalg.norm(np.array(spheres[i][0]) - np.array(spheres[j][0]))
            assert d > spheres[i][1] + spheres[j][1] + 2.0 / 16 + 2 * 2.0 / (Q - 1)      # supports disjoint, with a cell to spare
    return fs[0], np.maximum(np.maximum(fs[0], fs[1]), fs[2])
