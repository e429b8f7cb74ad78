"""Numpy statement of the mesh-decimation contract (include/sfmi.h): quadric vertex clustering on a G^3 grid over a
box, and the bisection of G to a face budget.  One shape at a time; a batch is its shapes one after the other.

  cell_keys(verts, G, bbox)            the f32 cell expression -> int64 keys (c0 G + c1) G + c2
  count(verts, faces, G, bbox)         -> (surviving faces, occupied cells): the counting pass
  cluster(verts, faces, G, bbox, reg)  -> verts (C,3) f32, faces (S,3) int32, status
  bisect(verts, faces, target, bbox)   -> G (0: the mesh is at or below the budget and stays as it is)
  decimate(verts, faces, target, ...)  -> verts, faces, status, G

The cell expression has no place where a fused multiply-add could form, so numpy f32 gives the device's bits.  Quadrics are summed
in f64 in corner order (face-major), relative to the cell centre; the device sums the same terms in another order, which the
position tolerance of tests/test_simplify_gpu.py accounts for.
"""
import numpy as np

UNIT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def cell_coords(verts, G, bbox=UNIT_BOX):
    """t = (v - lo) / (hi - lo) in f32, c = clamp(floor(t * G), 0, G-1) per axis -> (V,3) int64"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    lo, hi = np.asarray(bbox[0], np.float64).astype(np.float32), np.asarray(bbox[1], np.float64).astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (v - lo) / (hi - lo)
        c = np.floor(t * np.float32(G))
    assert c.dtype == np.float32
    return np.clip(c, 0, G - 1).astype(np.int64)      # clamped as a float first: the same values, and no overflowing cast


def cell_keys(verts, G, bbox=UNIT_BOX):
    c = cell_coords(verts, G, bbox)
    return (c[:, 0] * G + c[:, 1]) * G + c[:, 2]


def status_of(verts, faces):
    """0 ok, 1 no vertices, 2 a face index outside [0, V), 3 a non-finite vertex (the lowest code that applies)"""
    v, f = np.asarray(verts).reshape(-1, 3), np.asarray(faces).reshape(-1, 3)
    if len(v) == 0:
        return 1
    if len(f) and (f.min() < 0 or f.max() >= len(v)):
        return 2
    if not np.isfinite(v).all():
        return 3
    return 0


def _structure(verts, faces, G, bbox):
    """-> (ascending occupied keys, slot of every vertex, survive flag of every face)"""
    keys = cell_keys(verts, G, bbox)
    cells, slot = np.unique(keys, return_inverse=True)
    s = slot.reshape(-1)[np.asarray(faces, np.int64).reshape(-1, 3)]
    surv = (s[:, 0] != s[:, 1]) & (s[:, 1] != s[:, 2]) & (s[:, 0] != s[:, 2])
    return cells, slot.reshape(-1), surv


def count(verts, faces, G, bbox=UNIT_BOX):
    """the counting pass: (surviving faces, occupied cells); (0, 0) for a shape whose status is not 0"""
    if status_of(verts, faces):
        return 0, 0
    cells, _, surv = _structure(verts, faces, G, bbox)
    return int(surv.sum()), len(cells)


def cluster(verts, faces, G, bbox=UNIT_BOX, reg=1e-3):
    verts, faces = np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3)
    st = status_of(verts, faces)
    if st:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), st
    cells, slot, surv = _structure(verts, faces, G, bbox)
    C = len(cells)
    lo, hi = np.asarray(bbox[0], np.float64), np.asarray(bbox[1], np.float64)
    h = (hi - lo) / G
    cc = np.stack([cells // (G * G), (cells // G) % G, cells % G], 1)
    ctr = lo + (cc + 0.5) * h                                         # (C,3) f64
    P = verts.astype(np.float64)
    # mean of the cell's vertices, relative to the centre
    rel = P - ctr[slot]
    msum, cnt = np.zeros((C, 3)), np.bincount(slot, minlength=C)
    np.add.at(msum, slot, rel)
    m = msum / cnt[:, None]
    # quadrics: every corner (f, k) adds the plane of face f to the cell of its vertex
    F = faces.astype(np.int64)
    p0, p1, p2 = P[F[:, 0]], P[F[:, 1]], P[F[:, 2]]
    n = np.cross(p1 - p0, p2 - p0)                                    # not normalised: the weight is the squared area
    A, b = np.zeros((C, 3, 3)), np.zeros((C, 3))
    for k in range(3):
        s = slot[F[:, k]]
        d = -np.einsum("ij,ij->i", n, p0 - ctr[s])
        np.add.at(A, s, n[:, :, None] * n[:, None, :])
        np.add.at(b, s, d[:, None] * n)
    tr = np.trace(A, axis1=1, axis2=2)
    x = m.copy()
    pos = tr > 0
    if pos.any():
        lam = reg * tr[pos]
        M = A[pos] + lam[:, None, None] * np.eye(3)
        x[pos] = np.linalg.solve(M, (-b[pos] + lam[:, None] * m[pos])[..., None])[..., 0]
    x = np.clip(x, -h / 2, h / 2)
    out_f = slot[F[surv]].astype(np.int32).reshape(-1, 3)
    return (ctr + x).astype(np.float32), out_f, 0


def bisect(verts, faces, target, bbox=UNIT_BOX, gmax=512):
    """the G of the face budget; 0 where the mesh has at most `target` faces (it is returned unchanged)"""
    faces = np.asarray(faces).reshape(-1, 3)
    if len(faces) <= target:
        return 0
    if count(verts, faces, gmax, bbox)[0] <= target:
        return gmax
    lo, hi = 1, gmax
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if count(verts, faces, mid, bbox)[0] <= target:
            lo = mid
        else:
            hi = mid
    return lo


def decimate(verts, faces, target=4096, bbox=UNIT_BOX, reg=1e-3):
    G = bisect(verts, faces, target, bbox)
    if G == 0:
        v = np.asarray(verts, np.float32).reshape(-1, 3)           # unchanged and not inspected: status 0, or 1 without vertices
        return v, np.asarray(faces, np.int32).reshape(-1, 3), int(len(v) == 0), 0
    return cluster(verts, faces, G, bbox, reg) + (G,)


def cube_mesh(n=16, half=0.5):
    """Tessellated cube [-half, half]^3: n x n quads per side, each side with its own (n+1)^2 vertices (6 (n+1)^2 vertices, 12 n^2
    faces), outward normals."""
    u = np.linspace(-half, half, n + 1)
    V, F = [], []
    for axis in range(3):
        for side in (-1, 1):
            a, b = np.meshgrid(u, u, indexing="ij")
            p = np.zeros((n + 1, n + 1, 3))
            p[..., axis] = side * half
            p[..., (axis + 1) % 3], p[..., (axis + 2) % 3] = a, b
            base = sum(len(v) for v in V)
            V.append(p.reshape(-1, 3))
            i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
            q00, q10, q01, q11 = (base + (i + di) * (n + 1) + j + dj for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)))
            t = np.stack([np.stack([q00, q10, q11], -1), np.stack([q00, q11, q01], -1)], 2).reshape(-1, 3)
            F.append(t if side > 0 else t[:, ::-1])
    return np.concatenate(V).astype(np.float32), np.concatenate(F).astype(np.int32)


def mc_fields(Q):
    """sphere r = 0.6, torus R = 0.55 r = 0.22, two spheres: the fields of tests/iso_sparse_ref.py, f32"""
    import iso_sparse_ref as R
    return {n: R.field(n, Q) for n in ("sphere", "torus", "two")}
