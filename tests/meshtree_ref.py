"""numpy statement of the mesh tree of csrc/meshtree.hip (contract: include/sfmi.h): Morton keys in f32, the face order, the implicit
8-ary topology over leaves of 64 faces, the node table (aabb, f64 sums in the device's order, area-weighted centroid, dipole, second
and third moments, radius rounded up) and the tree-code winding number with its decisions in f32 and its values in f64.  Fixtures of the meshtree tests."""
import numpy as np

import meshsdf_ref as R

LEAF = 64
F32 = np.float32


# ---- order ------------------------------------------------------------------------------------------------------------------------------

def spread10(u):
    u = u.astype(np.int64)
    u = (u | (u << 16)) & 0x030000FF
    u = (u | (u << 8)) & 0x0300F00F
    u = (u | (u << 4)) & 0x030C30C3
    return (u | (u << 2)) & 0x09249249


def morton_keys(vert, face):
    """vert (V,3) f32, face (T,3) -> (T,) int64 30-bit keys; every operation in f32, rounded on its own"""
    v = np.asarray(vert, F32)
    lo, hi = v.min(0), v.max(0)
    a, b, c = (v[face[:, k]] for k in range(3))
    cen = ((a + b) + c) / F32(3)
    w = hi - lo
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(w > 0, (cen - lo) / np.where(w > 0, w, F32(1)), F32(0)).astype(F32)
    u = np.clip(np.floor(t * F32(1024)), 0, 1023).astype(np.int64)
    return (spread10(u[:, 0]) << 2) | (spread10(u[:, 1]) << 1) | spread10(u[:, 2])


def face_order(vert, face):
    """sorted position -> original face index: by (key, face index)"""
    return np.argsort(morton_keys(vert, face), kind="stable")


def level_nodes(T):
    """node count of every level, leaves first"""
    if T <= 0:
        return []
    out = [(T + LEAF - 1) // LEAF]
    while out[-1] > 1:
        out.append((out[-1] + 7) // 8)
    return out


def leaf_range(l, j, L0):
    """the leaves node j of level l covers"""
    return j * 8 ** l, min((j + 1) * 8 ** l, L0)


def level_base(levels, l):
    return int(sum(levels[:l]))


# ---- the node table ---------------------------------------------------------------------------------------------------------------------

def degenerate(p):
    """meshsdf's rule in f64: width |ab x ac| / longest edge <= 2^-22 longest edge.  p (T,3,3) f32"""
    p = p.astype(np.float64)
    e = [p[:, (k + 1) % 3] - p[:, k] for k in range(3)]
    l2 = np.stack([(x * x).sum(1) for x in e], 1)
    u = np.cross(e[0], -e[2])
    return (u * u).sum(1) <= 2.0 ** -44 * l2.max(1) ** 2


def round_up_f32(x):
    f = np.asarray(x, np.float64).astype(F32)
    return np.where(f.astype(np.float64) >= x, f, np.nextafter(f, F32(np.inf))).astype(F32)


NS = 34                                          # f64 sums per node; the sliver flag follows them
SI, SJ = (0, 1, 2, 0, 0, 1), (0, 1, 2, 1, 2, 2)  # the symmetric index pairs xx yy zz xy xz yz
SYM = ((0, 3, 4), (3, 1, 5), (4, 5, 2))


def coefficients(mom, p):
    """the sums about the origin shifted to the stored centre p (f32) in f64, in the device's order of operations, then what the
    expansion reads, rounded to f32: (NN,20) = tr Q, Qxx Qyy Qzz Qxy+Qyx Qxz+Qzx Qyz+Qzy, g (3), K xxx yyy zzz xxy xxz yyx yyz zzx zzy xyz"""
    P, D = p.astype(np.float64), mom[:, 4:7]
    R2 = lambda i, k: mom[:, 7 + 3 * i + k]
    Q = [[R2(i, k) - P[:, i] * D[:, k] for k in range(3)] for i in range(3)]
    M = [[((mom[:, 16 + 3 * q + k] - R2(SI[q], k) * P[:, SJ[q]]) - P[:, SI[q]] * R2(SJ[q], k)) + (P[:, SI[q]] * P[:, SJ[q]]) * D[:, k]
          for k in range(3)] for q in range(6)]
    g = [-6.0 * ((M[SYM[0][j]][0] + M[SYM[1][j]][1]) + M[SYM[2][j]][2]) - 3.0 * ((M[0][j] + M[1][j]) + M[2][j]) for j in range(3)]
    out = [(Q[0][0] + Q[1][1]) + Q[2][2], Q[0][0], Q[1][1], Q[2][2], Q[0][1] + Q[1][0], Q[0][2] + Q[2][0], Q[1][2] + Q[2][1], g[0], g[1], g[2],
           M[0][0], M[1][1], M[2][2], M[0][1] + 2.0 * M[3][0], M[0][2] + 2.0 * M[4][0], M[1][0] + 2.0 * M[3][1], M[1][2] + 2.0 * M[5][1],
           M[2][0] + 2.0 * M[4][2], M[2][1] + 2.0 * M[5][2], 2.0 * ((M[3][2] + M[4][1]) + M[5][0])]
    return np.stack(out, 1).astype(F32)


def expansion(r, dip, c):
    """the half solid angle of a node seen at r = p - q (N,3) f64 from its f32 dipole (3,) and coefficients c (20,), in f64:
    ((D . r + tr Q) / |r|^3 + (g . r / 2 - 3 r^T Q r) / |r|^5 + 7.5 K(r, r, r) / |r|^7) / 2"""
    c, D = c.astype(np.float64), dip.astype(np.float64)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    d2 = (r * r).sum(1)
    qf = c[1] * x * x + c[2] * y * y + c[3] * z * z + c[4] * x * y + c[5] * x * z + c[6] * y * z
    gr = c[7] * x + c[8] * y + c[9] * z
    cf = (c[10] * x ** 3 + c[11] * y ** 3 + c[12] * z ** 3 + c[13] * x * x * y + c[14] * x * x * z + c[15] * y * y * x + c[16] * y * y * z
          + c[17] * z * z * x + c[18] * z * z * y + c[19] * x * y * z)
    return 0.5 * ((r @ D + c[0]) / d2 ** 1.5 + (0.5 * gr - 3.0 * qf) / d2 ** 2.5 + 7.5 * cf / d2 ** 3.5)


def build(vert, face):
    """-> dict: order (T,), levels, lo / hi (NN,3) f32, mom (NN,36) f64 (area, a c, dipole, R2 = sum c (x) a n, R3 = sum S (x) a n about
    the origin, sliver flag, pad), p (NN,3) f32, dip (NN,3) f32, coef (NN,20) f32 (tr Q, Q's symmetric part (6), g (3), K (10): what
    the expansion reads, about the stored p), r (NN,) f32, r64 (NN,) f64 the radius before rounding, noprune (NN,) bool; nodes level
    by level, leaves first"""
    v = np.asarray(vert, F32)
    T = len(face)
    order = face_order(v, face)
    P = v[face[order]]                                                   # (T,3,3) sorted
    levels = level_nodes(T)
    L0, NN = levels[0], sum(levels)
    wt = ~degenerate(P)
    Pd = P.astype(np.float64)
    e1, e2, e3 = Pd[:, 1] - Pd[:, 0], Pd[:, 2] - Pd[:, 0], Pd[:, 2] - Pd[:, 1]
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    cr2 = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    sq = lambda x: (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
    lm = np.maximum(sq(e1), np.maximum(sq(e2), sq(e3)))
    sliver = wt & (cr2 <= 2.0 ** -16 * lm * lm)
    at = 0.5 * np.sqrt(cr2)
    cen = ((Pd[:, 0] + Pd[:, 1]) + Pd[:, 2]) / 3.0
    an = 0.5 * n
    dv = [Pd[:, k] - cen for k in range(3)]
    r2 = np.stack([cen[:, i] * an[:, k] for i in range(3) for k in range(3)], 1)
    s0 = [cen[:, i] * cen[:, j] + ((dv[0][:, i] * dv[0][:, j] + dv[1][:, i] * dv[1][:, j]) + dv[2][:, i] * dv[2][:, j]) / 12.0
          for i, j in zip(SI, SJ)]
    r3 = np.stack([s0[q] * an[:, k] for q in range(6) for k in range(3)], 1)
    term = np.concatenate([at[:, None], at[:, None] * cen, an, r2, r3], 1) * wt[:, None]      # (T,34)
    lo, hi = np.empty((NN, 3), F32), np.empty((NN, 3), F32)
    mom = np.zeros((NN, 36))
    pad = L0 * LEAF - T
    tp = np.concatenate([term, np.zeros((pad, NS))]).reshape(L0, LEAF, NS)
    for k in range(LEAF):                                                # a leaf's faces in order
        mom[:L0, :NS] += tp[:, k]
    for j in range(L0):
        s = slice(j * LEAF, min((j + 1) * LEAF, T))
        lo[j], hi[j] = P[s].reshape(-1, 3).min(0), P[s].reshape(-1, 3).max(0)
        mom[j, NS] = sliver[s].any()
    for l in range(1, len(levels)):
        cb, b = level_base(levels, l - 1), level_base(levels, l)
        for j in range(levels[l]):
            c0, c1 = 8 * j, min(8 * j + 8, levels[l - 1])
            acc = np.zeros(NS)
            for c in range(c0, c1):                                      # a node's children in order
                acc = acc + mom[cb + c, :NS]
            mom[b + j, :NS] = acc
            mom[b + j, NS] = mom[cb + c0:cb + c1, NS].max()
            lo[b + j], hi[b + j] = lo[cb + c0:cb + c1].min(0), hi[cb + c0:cb + c1].max(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(mom[:, :1] > 0, mom[:, 1:4] / mom[:, :1], (lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(F32)
    r64 = np.empty(NN)
    for l in range(len(levels)):
        b = level_base(levels, l)
        for j in range(levels[l]):
            a0, a1 = leaf_range(l, j, L0)
            d = Pd[a0 * LEAF:min(a1 * LEAF, T)].reshape(-1, 3) - p[b + j].astype(np.float64)
            r64[b + j] = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).max())
    return dict(order=order, levels=levels, lo=lo, hi=hi, mom=mom, p=p, dip=mom[:, 4:7].astype(F32), coef=coefficients(mom, p),
                r=round_up_f32(r64), r64=r64, noprune=mom[:, NS] != 0, P=P, wt=wt)


# ---- the tree-code winding number -------------------------------------------------------------------------------------------------------

def _d2_f32(q, p):
    """|q - p|^2 in f32, direct form fmaf(dz, dz, fmaf(dy, dy, dx * dx)) (the products are exact in f64)"""
    d = (p[None].astype(F32) - q).astype(F32)
    s = (d[:, 0] * d[:, 0]).astype(F32)
    s = (d[:, 1].astype(np.float64) ** 2 + s).astype(F32)
    return (d[:, 2].astype(np.float64) ** 2 + s).astype(F32)


def winding(q, P, wt, levels, p, r, dip, coef, beta, count=None):
    """W_tree of queries q (N,3) f32 over the sorted faces P (T,3,3) f32 with weights wt and the node table (p, r, dip, coef f32): the
    far test in f32 as the device takes it, every value in f64.  count: a dict that gains 'faces' and 'approx' per query."""
    q = np.asarray(q, F32)
    N, T, L0 = len(q), len(P), levels[0]
    half = np.zeros(N)                                                   # sum of half solid angles
    faces, approx = np.zeros(N, np.int64), np.zeros(N, np.int64)
    beta = F32(beta)
    Pd = P.astype(np.float64)

    def visit(l, j, idx):
        n = level_base(levels, l) + j
        br = F32(beta * r[n])
        far = _d2_f32(q[idx], p[n]) > F32(br * br)
        fi = idx[far]
        if len(fi):
            d = p[n].astype(np.float64)[None] - q[fi].astype(np.float64)
            half[fi] += expansion(d, dip[n], coef[n])
            approx[fi] += 1
        ni = idx[~far]
        if not len(ni):
            return
        if l == 0:
            s = slice(j * LEAF, min((j + 1) * LEAF, T))
            om = R.solid_angle(q[ni].astype(np.float64)[:, None], Pd[None, s, 0], Pd[None, s, 1], Pd[None, s, 2])
            half[ni] += (0.5 * om * wt[None, s]).sum(1)
            faces[ni] += s.stop - s.start
            return
        for c in range(8 * j, min(8 * j + 8, levels[l - 1])):
            visit(l - 1, c, ni)

    visit(len(levels) - 1, 0, np.arange(N))
    if count is not None:
        count["faces"], count["approx"] = faces, approx
    return half / (2 * np.pi)


def brute_winding(q, vert, face, chunk=128):
    """the exact generalized winding number in f64 (degenerate faces add nothing: their solid angle is 0)"""
    v = np.asarray(vert, np.float64)
    A, B, C = (v[face[:, k]] for k in range(3))
    q = np.asarray(q, np.float64)
    return np.concatenate([R.solid_angle(q[s:s + chunk, None], A[None], B[None], C[None]).sum(1) for s in range(0, len(q), chunk)]) / (4 * np.pi)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------

def uv_sphere(nu=96, nv=48, r=0.8, z_top=None):
    """nu x nv quads of a latitude-longitude sphere, two triangles each (2 nu nv faces, outward; a pole's quads have one zero-area
    triangle).  z_top: the polar angle starts where z = z_top instead of at the north pole: an open bowl"""
    th0 = 0.0 if z_top is None else np.arccos(z_top / r)
    th = th0 + (np.pi - th0) * np.arange(nv + 1) / nv
    ph = 2 * np.pi * np.arange(nu) / nu
    v = np.stack([r * np.sin(th)[:, None] * np.cos(ph)[None], r * np.sin(th)[:, None] * np.sin(ph)[None],
                  r * np.cos(th)[:, None] * np.ones(nu)[None]], -1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij")
    a, b, c, d = i * nu + j, (i + 1) * nu + j, (i + 1) * nu + (j + 1) % nu, i * nu + (j + 1) % nu
    f = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return v.astype(F32), f.astype(np.int32)


def sphere():
    return uv_sphere(96, 48, 0.8)


def bowl():
    return uv_sphere(96, 40, 0.8, z_top=0.0371)


def lattice(G=17, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, G)
    return np.stack(np.meshgrid(x, x, x, indexing="ij"), -1).reshape(-1, 3).astype(F32)


def strip_mesh(T):
    """T triangles of a zigzag strip along x in the plane z = 0, hand-checkable: face t has its centroid at x = (t + 1) / 2 and at
    y = 1/3 (even t) or 2/3 (odd t), one orientation"""
    n = T + 2
    v = np.stack([np.arange(n) * 0.5, (np.arange(n) % 2) * 1.0, np.zeros(n)], 1).astype(F32)
    f = np.stack([np.arange(T), np.arange(T) + 1, np.arange(T) + 2], 1)
    f[1::2] = f[1::2][:, [1, 0, 2]]                                      # one orientation
    return v, f.astype(np.int32)

