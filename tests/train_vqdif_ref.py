"""Float64 references of the VQDIF training kernels (csrc/train_vqdif.hip and the forward sfmi_maxpool2_cl_f32 / sfmi_upcat_cl_f32 /
sfmi_affine_cl_f32 of csrc/conv3d.hip), f32 mirrors of their index arithmetic and of the host rules that choose a launch form, and the
per-element error bounds their tests assert.  numpy only: no GPU, no torch, no reference tree.  The references restate each operation on
the f32 inputs the kernel sees; nothing here reuses a kernel's tiling or summation order.

Error bounds
  U = 2^-24, gamma(n) = n U / (1 - n U) (train_ref.py): a sum whose terms pass through at most n roundings is off by at most
  gamma(n) sum |term|.  A product, a sum and a division round once.  The library is built with -ffp-contract=on, so a * x + b * y may or
  may not be fused: a fused multiply-add rounds once where the separate form rounds twice, so counting the product and the sum separately
  is the worst case and every bound below holds for both.  Every bound is per output element.

  lincomb_kernel      a x + b y: two products, one sum: the sum's rounding is relative to |out| <= |a x| + |b y|              [LIN]
                      |err| <= 2 U (|a x| + |b y|);  y == NULL: a x + 0: U |a x|
  affine2_kernel      A u + B v + C: products U |A u|, U |B v|; first sum U (|A u| + |B v|); second sum U (|A u| + |B v| + |C|)
                      |err| <= 3 U (|A u| + |B v| + |C|)                                                                         [AFF2]
  affine_cl_kernel    x s + t:  |err| <= 2 U (|x s| + |t|)                                                                       [AFF]
  chan_dot_stats      float64 accumulators (U64 = 2^-53).  The product of two f32 is exact in f64.  A voxel lane adds ceil(len / rpp) terms
                      one after the other, lane 0 then adds the rpp - 1 other lanes serially: n = ceil(len / rpp) + rpp roundings.
                      |err| <= gamma64(n) sum |term|; an empty slice is exactly zero.                                              [CDS]
  sumpool2 / upsample2 / upcat / the two max-pools: data on a 2^-3 grid, so the eight-term sums are exact and every result is bit-exact.
  cells_kernel        p / 2 is exact; (p / 2) / 1.101f, + 0.5f and * G round once each and are mirrored in f32 (numpy's f32 operations are
                      correctly rounded, as __fdiv_rn and the f32 add / multiply are); no a * b + c occurs, so contraction changes nothing.
                      Bit-exact.
  fixed point  [FIX]  (embedding gradients): an accumulator is sum_i rint(v_i 2^32) as an integer, exactly and in any order;
                      (float)((double) acc 2^-32) rounds once (|acc| < 2^53 here).  Each term is off by at most 2^-33, so against the
                      float64 sum  |err| <= count 2^-33 + U |sum|.
  cell_mean_kernel    (double) acc 2^-32 / n rounds in f64 (negligible: 2^-53), the conversion to f32 rounds once:
                      |err| <= count 2^-33 / n + U (1 + 2^-20) |mean|
  cell_mean_bwd       one f32 division: |err| <= U |dgrid / count|
  trilinear  [TRI]    tri_axis is mirrored in f32 up to ix (the clamped lattice coordinate): x / 2 exact, the division, + 0.5, 2 u - 1 (2 u is
                      exact, so the fused and the separate form agree bit for bit), v + 1, / 2 exact, * (G - 1).  w1 = ix - floor(ix) is exact;
                      w0 = (floor(ix) + 1) - ix rounds once when floor(ix) == 0 (exact otherwise, Sterbenz); the corner weight (wx wy) wz
                      rounds twice more: every f32 weight is within 3 U (relative, gamma(3)) of the float64 weight formed from the same ix.
                      Forward: eight fmaf, one rounding each:  |err| <= gamma(3 + 8) sum_corners |w grid|.
                      Backward: w * d rounds once more (a lone product: nothing to contract), then [FIX]:
                      |err| <= count 2^-33 + gamma(4) sum |w d| + U |sum|     (count: point-corner pairs that land on the element)
  bce_logits_kernel   expf and log1pf are the OCML library functions, whose documented accuracy (OpenCL C full profile: exp <= 3 ulp,
                      log1p <= 2 ulp; 1 ulp <= 2 U relative) is used: E_EXPF = 6 U, E_LOG1P = 4 U.  e = expf(-|x|);  l = log1pf(e):
                      d l <= E_EXPF e (the slope of log1p is <= 1) + E_LOG1P l.  a = max(x, 0) - x y: U |x y| + U |a| (fused: less).
                      |d loss| <= U |x y| + U |a| + E_EXPF e + E_LOG1P l + U |loss| + TINY                                          [BCE]
                      s = 1 / (1 + expf(-x)): E_EXPF e' / (1 + e') + 2 U relative (the sum, the division) <= (E_EXPF + 2) U s, and
                      0 / denormal where expf overflows or the quotient leaves the normal range (TINY = 2^-120 covers both).
                      |d dlogit| <= |scale| ((E_EXPF + 2) U s + U |s - y|) + U |dlogit| + TINY
  vq_ema_kernel       N' = N g + (1 - g) c ((1 - g) is exact for g in [0.5, 1], Sterbenz): |d N'| <= 2 U (|N g| + |(1 - g) c|) [LIN]; z' alike.
                      n = sum N': a thread adds ceil(K / 1024) terms, then a 10-level tree over the 1024 threads:                     [EMA]
                      |d n| <= sum |d N'| + gamma(ceil(K / 1024) + 10) sum |N'|
                      w = (N' + eps) / (n + K eps) n:  a = N' + eps: d a <= d N' + U a;  b = n + K eps: d b <= d n + U K eps + U b;
                      relative  e_w = d a / a + d b / b + d n / n + 2 U (the division, the product)
                      emb = z' / w:  |d emb| <= d z' / w + |emb| (e_w + U)
  conv_wgrad_kernel   a slice accumulates min(rows, rows_per_split) products along one chain of 16x16x4 f32 MFMAs (four sequential fused
                      multiply-adds each, train_ref.py [ATTN]); sfmi_colsum_f32 over the nsplit slices adds colsum_depth('plain', nsplit):
                      |err| <= gamma(min(rows, rows_per_split) + colsum_depth) sum_r |dy x|                                          [WG]
"""
from __future__ import annotations

import itertools
import math

import numpy as np

from train_ref import U, TINY, FIX, gamma, f64, ratio, colsum_depth   # noqa: F401  (re-exported for the tests)

F32 = np.float32
U64 = 2.0 ** -53
E_EXPF, E_LOG1P = 6.0, 4.0                      # module docstring [BCE], in units of U
NORM_DIV, NORM_HI = F32(1.101), F32(0.999)      # sfmi_common.h: SFMI_NORM_DIV, SFMI_NORM_HI
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def gamma64(n):
    n = np.asarray(n, np.float64)
    return n * U64 / (1.0 - n * U64)


# ---------------------------------------------------------------------------------------------------- mirrors of the launch rules
def gn_splits(V):
    """sfmi_gn_splits (csrc/conv3d.hip)."""
    return 64 if V >= 32768 else 16 if V >= 4096 else 4 if V >= 512 else 1


def stats_slice(V, s, S):
    """v0, v1 of slice s of S in chan_dot_stats_kernel."""
    return V * s // S, V * (s + 1) // S


def chan_rpp(C):
    """(cg, rpp, idle threads) of chan_dot_stats_kernel: 256 threads = rpp voxel lanes x cg float4 channel groups."""
    cg = C // 4
    rpp = 256 // cg
    return cg, rpp, 256 - cg * rpp


def rows_per_split(rows, nsplit):
    """sfmi_conv3d_wgrad_f32: rows of a slice, a multiple of the 16-row stage."""
    return ((rows + nsplit - 1) // nsplit + 15) // 16 * 16


def wgrad_rows(B, Di, Hi, Wi, KS, stride, pad):
    o = lambda n: (n + 2 * pad - KS) // stride + 1
    return B * o(Di) * o(Hi) * o(Wi)


def wgrad_nsplit(rows, Cin, Cout, KS):
    """VQDIFTrainer._wgrad_into: enough (tile, tap, slice) blocks to fill the chip, at least 256 rows per slice."""
    tiles = -(-Cout // 64) * -(-Cin // 64) * KS ** 3
    return max(1, min(512, -(-1024 // tiles), rows // 256))


def wgrad_empty_slices(rows, nsplit):
    rps = rows_per_split(rows, nsplit)
    return sum(1 for s in range(nsplit) if s * rps >= rows)


def wgrad_empty_nsplit(rows):
    """the smallest nsplit whose last slices hold no row"""
    return next(ns for ns in itertools.count(2) if wgrad_empty_slices(rows, ns))


# ---------------------------------------------------------------------------------------------------- elementwise, statistics
def relu_bwd_ref(dy, y):
    return np.where(np.asarray(y, F32) > 0, np.asarray(dy, F32), F32(0))


def lincomb_ref(a, x, b, y):
    """-> (value, bound) [LIN]; a, b are the f32 scalars the kernel receives."""
    a, b = float(F32(a)), float(F32(b))
    t0 = a * f64(x)
    t1 = b * f64(y) if y is not None else np.zeros_like(t0)
    k = 2.0 if y is not None else 1.0
    return t0 + t1, k * U * (np.abs(t0) + np.abs(t1)) + TINY


def affine2_ref(u, v, A, Bc, Cc):
    """u, v (B,V,C); A, Bc, Cc (B,C) -> (value, bound) [AFF2]."""
    a, b, c = (f64(t)[:, None, :] for t in (A, Bc, Cc))
    t0, t1 = a * f64(u), b * f64(v)
    return t0 + t1 + c, 3 * U * (np.abs(t0) + np.abs(t1) + np.abs(c)) + TINY


def affine_ref(x, scale, shift):
    t0, t1 = f64(x) * f64(scale)[:, None, :], np.broadcast_to(f64(shift)[:, None, :], np.shape(x))
    return t0 + t1, 2 * U * (np.abs(t0) + np.abs(t1)) + TINY


def chan_dot_stats_ref(dy, x, S):
    """dy, x (B,V,C) -> partial (B,S,C,2) in extended precision, and its bound [CDS]."""
    dy, x = np.asarray(dy, np.longdouble), np.asarray(x, np.longdouble)
    B, V, C = dy.shape
    _, rpp, _ = chan_rpp(C)
    out, bnd = np.zeros((B, S, C, 2), np.longdouble), np.zeros((B, S, C, 2))
    for s in range(S):
        v0, v1 = stats_slice(V, s, S)
        if v1 <= v0:
            continue
        d, p = dy[:, v0:v1], dy[:, v0:v1] * x[:, v0:v1]
        out[:, s, :, 0], out[:, s, :, 1] = d.sum(1), p.sum(1)
        g = float(gamma64(-(-(v1 - v0) // rpp) + rpp))
        bnd[:, s, :, 0], bnd[:, s, :, 1] = g * np.abs(d).sum(1), g * np.abs(p).sum(1)
    return out, bnd


# ---------------------------------------------------------------------------------------------------- pooling / resampling
def _windows(x):
    """(B,2D,2H,2W,C) -> (B,D,H,W,C,8), window element t = 4 dz + 2 dy + dx (the kernels' z-major order)."""
    B, D2, H2, W2, C = x.shape
    return x.reshape(B, D2 // 2, 2, H2 // 2, 2, W2 // 2, 2, C).transpose(0, 1, 3, 5, 7, 2, 4, 6).reshape(B, D2 // 2, H2 // 2, W2 // 2, C, 8)


def _unwindows(w):
    B, D, H, W, C, _ = w.shape
    return w.reshape(B, D, H, W, C, 2, 2, 2).transpose(0, 1, 5, 2, 6, 3, 7, 4).reshape(B, 2 * D, 2 * H, 2 * W, C)


def upsample2_ref(x):
    return np.repeat(np.repeat(np.repeat(x, 2, 1), 2, 2), 2, 3)


def upcat_ref(skip, low):
    return np.concatenate([skip, upsample2_ref(low)], -1)


def sumpool2_ref(dy, c0, Cs):
    """float64 sum of the eight children of every voxel on the channel slice [c0, c0 + Cs)"""
    return _windows(f64(dy)[..., c0:c0 + Cs]).sum(-1)


def maxpool2_ref(x):
    return _windows(np.asarray(x, F32)).max(-1)


def maxpool2_bwd_ref(x, y, dy):
    """the gradient goes to the FIRST child, in z-major order, that equals the pooled value (ATen's rule); -0 == +0"""
    w = _windows(np.asarray(x, F32))
    hit = w == np.asarray(y, F32)[..., None]
    first = hit & (np.cumsum(hit, -1) == 1)
    return _unwindows(np.where(first, np.asarray(dy, F32)[..., None], F32(0)))


def pool_patterns():
    """-> (names, (P, 8) f32): every tie pattern of a 2^3 window on a 2^-3 grid.  'uniqueT': the only maximum at element T; 'pairST': a
    two-way tie at S < T (S wins); 'equal*': all eight equal; 'zeros-+' / 'zeros+-': -0 before / after +0 above negatives; 'neg*': all
    negative, with a unique maximum, a tie, and all equal."""
    names, rows = [], []
    lo = np.array([-1.0, -0.5, 0.125, -2.0, 0.25, -0.125, 0.375, -3.0], F32)
    for t in range(8):
        w = lo.copy(); w[t] = 1.5
        names.append(f"unique{t}"); rows.append(w)
    for s, t in itertools.combinations(range(8), 2):
        w = lo.copy(); w[s] = w[t] = 0.75
        names.append(f"pair{s}{t}"); rows.append(w)
    names += ["equal+", "equal0", "equal-0"]
    rows += [np.full(8, 0.5, F32), np.zeros(8, F32), np.full(8, -0.0, F32)]
    neg = -np.abs(lo) - F32(0.25)
    w = neg.copy(); w[2], w[5] = -0.0, 0.0
    names.append("zeros-+"); rows.append(w)
    w = neg.copy(); w[1], w[6] = 0.0, -0.0
    names.append("zeros+-"); rows.append(w)
    w = neg.copy(); w[4] = -0.125
    names.append("neg_unique"); rows.append(w)
    w = neg.copy(); w[3] = w[7] = -0.125
    names.append("neg_pair"); rows.append(w)
    names.append("neg_equal"); rows.append(np.full(8, -2.5, F32))
    return names, np.stack(rows).astype(F32)


def pool_input(B, Do, Ho, Wo, C, shift):
    """(B,2Do,2Ho,2Wo,C) f32 whose window j (linear, channel fastest) holds pattern (j + shift) % P; -> (x, pattern index per window)"""
    _, pat = pool_patterns()
    n = B * Do * Ho * Wo * C
    idx = (np.arange(n) + shift) % len(pat)
    return _unwindows(pat[idx].reshape(B, Do, Ho, Wo, C, 8)), idx


# ---------------------------------------------------------------------------------------------------- encoder pooling
def normalize_f32(p):
    """sfmi_normalize on f32 (p already halved)"""
    u = (np.asarray(p, F32) / NORM_DIV).astype(F32) + F32(0.5)
    u = np.where(u >= F32(1), NORM_HI, u)
    return np.where(u < F32(0), F32(0), u).astype(F32)


def cells_ref(cloud, G):
    """cells_kernel: -> (cell int32 (...,), p_half f32 (...,3)), bit-exact"""
    h = (np.asarray(cloud, F32) * F32(0.5)).astype(F32)
    i = (normalize_f32(h) * F32(G)).astype(F32).astype(np.int32)
    return (i[..., 0] + G * (i[..., 1] + G * i[..., 2])).astype(np.int32), h


def cell_boundary_coords(G):
    """every f32 cloud coordinate at which the rounding can turn the cell index: for each cell boundary the last float of the lower cell and
    the first of the upper one (found by bisection on the mirror, which is monotone) with one more float either side, +-1, the clamps of
    sfmi_normalize (|x| / 2 / 1.101 = 0.5) and beyond them, +-0"""
    cx = lambda x: int(cells_ref(np.array([[x, 0, 0]], F32), G)[0][0]) % G
    v = []
    for k in range(1, G):
        lo, hi = (int(f2key(F32(x))[0]) for x in (-2.5, 2.5))          # cx(lo) < k <= cx(hi); keys are ordered as the floats are
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if cx(key2f(np.int32(mid))) < k else (lo, mid)
        v += [key2f(np.int32(q)) for q in (lo - 1, lo, hi, hi + 1)]
    for x in (1.0, 1.1, 1.101, 1.102, 1.2, 2.5, 0.0):
        v += [F32(x), F32(-x), np.nextafter(F32(x), F32(np.inf)), np.nextafter(F32(-x), F32(-np.inf))]
    return np.array(v, F32).reshape(-1)


def f2key(x):
    """the kernels' monotone f32 -> int32 key (signed integer order == float order, -0 < +0)"""
    i = np.ascontiguousarray(x, F32).view(np.int32)
    return np.where(i >= 0, i, i ^ np.int32(0x7FFFFFFF)).astype(np.int32)


def key2f(k):
    k = np.asarray(k, np.int32)
    return np.where(k >= 0, k, k ^ np.int32(0x7FFFFFFF)).astype(np.int32).view(F32)


def cell_max_ref(net, cell, ncell):
    """net (B,T,C) f32, cell (B,T) -> (keys (B,ncell,C) int32 with INT_MIN in empty cells, pooled (B,T,C) f32), exact"""
    B, T, C = net.shape
    keys = np.full((B, ncell, C), INT_MIN, np.int32)
    k = f2key(net)
    for b in range(B):
        np.maximum.at(keys[b], cell[b], k[b])
    return keys, np.stack([key2f(keys[b][cell[b]]) for b in range(B)])


def to_fix(v):
    """__double2ll_rn((double) v * 2^32)"""
    return np.rint(f64(v) * FIX).astype(np.int64)


def fix_to_float(acc):
    return (np.asarray(acc, np.int64).astype(np.float64) / FIX).astype(F32)


def cell_scatter_ref(src, cell, ncell):
    """src (B,T,C) -> (acc int64 (B,ncell,C) exact, count int32 (B,ncell), float64 sum, float64 sum of |.|)"""
    B, T, C = src.shape
    acc, cnt = np.zeros((B, ncell, C), np.int64), np.zeros((B, ncell), np.int32)
    s, sa = np.zeros((B, ncell, C)), np.zeros((B, ncell, C))
    fx = to_fix(src)
    for b in range(B):
        np.add.at(acc[b], cell[b], fx[b])
        np.add.at(cnt[b], cell[b], 1)
        np.add.at(s[b], cell[b], f64(src[b]))
        np.add.at(sa[b], cell[b], np.abs(f64(src[b])))
    return acc, cnt, s, sa


def fix_bound(count, s):
    """[FIX]"""
    return f64(count) * 2.0 ** -33 + U * np.abs(s)


def cell_mean_ref(s, cnt):
    """float64 mean and bound from the float64 sums of cell_scatter_ref"""
    n = np.maximum(cnt, 1)[..., None].astype(np.float64)
    m = s / n
    return m, f64(cnt)[..., None] * 2.0 ** -33 / n + U * (1 + 2.0 ** -20) * np.abs(m)


def cell_mean_bwd_ref(dgrid, cnt, cell):
    """dgrid (B,ncell,C), cell (B,T) -> (value (B,T,C), bound)"""
    v = np.stack([f64(dgrid[b])[cell[b]] / f64(cnt[b])[cell[b]][:, None] for b in range(len(cell))])
    return v, U * np.abs(v) + TINY


def cell_winner(net, keys, cell):
    """the tie contract: win[b,cell,c] = the lowest point index t whose key equals the cell's maximum (INT_MAX in empty cells)"""
    B, T, C = net.shape
    win = np.full(keys.shape, INT_MAX, np.int64)
    k = f2key(net)
    for b in range(B):
        att = k[b] == keys[b][cell[b]]
        t = np.where(att, np.arange(T)[:, None], INT_MAX)
        np.minimum.at(win[b], cell[b], t)
    return win


def cell_max_bwd_ref(net, keys, acc, cell, prev=None):
    """dnet (B,T,C): the converted cell gradient at the winner, zero (prev when accumulating) elsewhere - exact in f32"""
    B, T, C = net.shape
    win = cell_winner(net, keys, cell)
    g = fix_to_float(acc)
    out = np.zeros((B, T, C), F32)
    for b in range(B):
        out[b] = np.where(win[b][cell[b]] == np.arange(T)[:, None], g[b][cell[b]], F32(0))
    return out if prev is None else (np.asarray(prev, F32) + out).astype(F32)


def cell_max_bwd_old_rule(net, keys, acc, cell):
    """what the kernel did before the tie contract: EVERY point whose value equals the maximum received the whole gradient"""
    g = fix_to_float(acc)
    k = f2key(net)
    return np.stack([np.where(k[b] == keys[b][cell[b]], g[b][cell[b]], F32(0)) for b in range(len(cell))])


# ---------------------------------------------------------------------------------------------------- trilinear sampling
def tri_axis(x, G):
    """tri_axis in f32: -> (i0, i1 int, w0, w1 f32 as the kernel forms them, ix f32)"""
    u = normalize_f32((np.asarray(x, F32) * F32(0.5)).astype(F32))
    v = (F32(2) * u - F32(1)).astype(F32)
    ix = (((v + F32(1)).astype(F32) / F32(2)).astype(F32) * F32(G - 1)).astype(F32)
    ix = np.minimum(F32(G - 1), np.maximum(ix, F32(0))).astype(F32)
    f0 = np.floor(ix).astype(F32)
    i0 = f0.astype(np.int64)
    return i0, np.minimum(i0 + 1, G - 1), ((f0 + F32(1)).astype(F32) - ix).astype(F32), (ix - f0).astype(F32), ix


def tri_corners(xyz, G):
    """xyz (B,N,3) -> (flat corner index (B,N,8) into G^3, float64 weights (B,N,8) formed from the f32 lattice coordinate)"""
    ax = [tri_axis(xyz[..., a], G) for a in range(3)]
    idx, w = [], []
    for corner in range(8):
        sel = (corner & 1, (corner >> 1) & 1, corner >> 2)          # dx, dy, dz
        ii, ww = [], []
        for a in range(3):
            i0, i1, _, _, ix = ax[a]
            w1 = f64(ix) - np.floor(f64(ix))
            ii.append(i1 if sel[a] else i0)
            ww.append(w1 if sel[a] else 1.0 - w1)
        idx.append((ii[2] * G + ii[1]) * G + ii[0])
        w.append(ww[0] * ww[1] * ww[2])
    return np.stack(idx, -1), np.stack(w, -1)


def trilinear_ref(xyz, grid, G):
    """grid (B,G^3,C) -> (out (B,N,C), bound) [TRI]"""
    idx, w = tri_corners(xyz, G)
    g = np.asarray(grid, F32)
    out, sa = np.zeros(idx.shape[:2] + (g.shape[-1],)), np.zeros(idx.shape[:2] + (g.shape[-1],))
    for b in range(idx.shape[0]):
        for k in range(8):
            t = w[b, :, k, None] * f64(g[b][idx[b, :, k]])
            out[b] += t
            sa[b] += np.abs(t)
    return out, gamma(11) * sa + TINY


def trilinear_bwd_ref(xyz, dout, G):
    """dout (B,N,C) -> (dgrid float64 (B,G^3,C), bound against acc 2^-32, bound against the converted f32) [TRI]"""
    idx, w = tri_corners(xyz, G)
    d = f64(dout)
    B, N, C = d.shape
    s, sa, cnt = np.zeros((B, G ** 3, C)), np.zeros((B, G ** 3, C)), np.zeros((B, G ** 3, 1))
    for b in range(B):
        for k in range(8):
            t = w[b, :, k, None] * d[b]
            np.add.at(s[b], idx[b, :, k], t)
            np.add.at(sa[b], idx[b, :, k], np.abs(t))
            np.add.at(cnt[b], idx[b, :, k], 1.0)
    b_acc = cnt * 2.0 ** -33 + gamma(4) * sa
    return s, b_acc, b_acc + U * np.abs(s)


# ---------------------------------------------------------------------------------------------------- loss, quantizer
def bce_ref(x, y, scale):
    """-> (loss, loss bound, dlogits, dlogits bound) [BCE]"""
    x, y, scale = f64(x), f64(y), float(F32(scale))
    e = np.exp(-np.abs(x))
    l = np.log1p(e)
    a = np.maximum(x, 0) - x * y
    loss = a + l
    bl = U * (np.abs(x * y) + np.abs(a) + E_EXPF * e + E_LOG1P * l + np.abs(loss)) + TINY
    with np.errstate(over="ignore"):
        s = 1.0 / (1.0 + np.exp(-x))
    d = (s - y) * scale
    return loss, bl, d, abs(scale) * U * ((E_EXPF + 2) * s + np.abs(s - y)) + U * np.abs(d) + TINY


def vq_stats_ref(x, idx, K):
    """x (rows,D), idx (rows,) -> (sums int64 (K,D) exact, counts int32 (K,))"""
    sums, cnt = np.zeros((K, x.shape[1]), np.int64), np.zeros(K, np.int32)
    np.add.at(sums, idx, to_fix(x))
    np.add.at(cnt, idx, 1)
    return sums, cnt


def vq_ema_ref(N, z, counts, sums, gamma_, eps):
    """-> dict(N, z, emb) of (value, bound) [EMA]"""
    g, eps = float(F32(gamma_)), float(F32(eps))
    og = float(F32(1) - F32(gamma_))
    N, z, c, s = f64(N), f64(z), f64(counts), f64(sums)
    K = N.shape[0]
    N1, dN = N * g + og * c, 2 * U * (np.abs(N * g) + np.abs(og * c))
    z1, dz = z * g + og * s, 2 * U * (np.abs(z * g) + np.abs(og * s)) + TINY
    n = N1.sum()
    dn = dN.sum() + float(gamma(-(-K // 1024) + 10)) * np.abs(N1).sum()
    a, b = N1 + eps, n + K * eps
    da, db = dN + U * np.abs(a), dn + U * K * eps + U * abs(b)
    w = a / b * n
    ew = da / np.abs(a) + db / abs(b) + dn / abs(n) + 2 * U
    emb = z1 / w[:, None]
    return dict(N=(N1, dN + TINY), z=(z1, dz), emb=(emb, dz / np.abs(w)[:, None] + np.abs(emb) * (ew[:, None] + U) + TINY))


# ---------------------------------------------------------------------------------------------------- conv weight gradient
def wgrad_ref(dy, x, B, Di, Hi, Wi, Cin, Cout, KS, stride, pad):
    """dy (rows, >= Cout), x (B*Di*Hi*Wi, >= Cin) channels-last rows -> (dW (KS^3, Cout, Cin) float64, sum of |terms|)"""
    o = lambda n: (n + 2 * pad - KS) // stride + 1
    Do, Ho, Wo = o(Di), o(Hi), o(Wi)
    d = f64(dy)[:, :Cout].reshape(B, Do, Ho, Wo, Cout)
    xp = np.zeros((B, Di + 2 * pad, Hi + 2 * pad, Wi + 2 * pad, Cin))
    xp[:, pad:pad + Di, pad:pad + Hi, pad:pad + Wi] = f64(x)[:, :Cin].reshape(B, Di, Hi, Wi, Cin)
    dW, sa = np.zeros((KS ** 3, Cout, Cin)), np.zeros((KS ** 3, Cout, Cin))
    d2, da = d.reshape(-1, Cout), np.abs(d).reshape(-1, Cout)
    for tap in range(KS ** 3):
        tz, ty, tx = tap // (KS * KS), (tap // KS) % KS, tap % KS
        xs = xp[:, tz:tz + stride * (Do - 1) + 1:stride, ty:ty + stride * (Ho - 1) + 1:stride, tx:tx + stride * (Wo - 1) + 1:stride].reshape(-1, Cin)
        dW[tap], sa[tap] = d2.T @ xs, da.T @ np.abs(xs)
    return dW, sa


def wgrad_bound(sa, rows, nsplit):
    """[WG]"""
    return gamma(min(rows, rows_per_split(rows, nsplit)) + colsum_depth("plain", nsplit)) * sa + TINY


# ---------------------------------------------------------------------------------------------------- test clouds
def cell_pool_case(C, seed):
    """One batch of points for the local max pool over ncell = 8 cells, every tie pattern present: -> dict(net (B,T,C) f32, cell (B,T) int32,
    ncell).  Per sample, before a seeded shuffle of the point order:
      cell 0  empty (sample 1: cell 7 instead)          cell 1  a single point                  cell 2  only negative values
      cell 3  three exact copies of one row that holds the maximum of every channel, among distinct rows
      cell 4  two DISTINCT rows that tie for the maximum in channel 1 only      cell 5  three distinct rows that tie in channel 0, one of them
      also present as an exact copy                     cell 6  -0 and +0 above negatives (+0 wins: key order)       cell 7  random rows"""
    rs = np.random.RandomState(seed)
    nets, cells = [], []
    for b in range(2):
        rows, cl = [], []
        def put(c, r):
            rows.append(np.asarray(r, F32)); cl.append(c)
        put(1, rs.randn(C))
        for _ in range(4):
            put(2, -np.abs(rs.randn(C)) - 0.25)
        top = np.abs(rs.randn(C)) + 4.0
        for _ in range(3):
            put(3, top)
        for _ in range(4):
            put(3, rs.randn(C))
        a, c2 = rs.randn(C), rs.randn(C)
        a[1] = c2[1] = 5.5
        put(4, a); put(4, c2)
        for _ in range(3):
            put(4, rs.randn(C))
        trio = [rs.randn(C) for _ in range(3)]
        for r in trio:
            r[0] = 6.25
            put(5, r)
        put(5, trio[1])
        put(5, rs.randn(C))
        z = -np.abs(rs.randn(4, C)) - 0.5
        z[1], z[2] = -0.0, 0.0
        for r in z:
            put(6, r)
        last = 7 if b == 0 else 0
        for _ in range(8):
            put(last, rs.randn(C))
        p = rs.permutation(len(rows))
        nets.append(np.stack(rows)[p]); cells.append(np.array(cl, np.int32)[p])
    return dict(net=np.stack(nets).astype(F32), cell=np.stack(cells), ncell=8)


def tri_points(G, N, seed):
    """(2,N,3) f32 query points in the API range: the first rows cycle through the special coordinates of tri_special(G) on every axis,
    the rest are uniform in [-1.2, 1.2]"""
    sp = tri_special(G)
    rs = np.random.RandomState(seed)
    xyz = (rs.rand(2, N, 3) * 2.4 - 1.2).astype(F32)
    n = min(N, 3 * len(sp))
    for b in range(2):
        for i in range(n):
            for a in range(3):
                xyz[b, i, a] = sp[(i + (5 * a + 3 * b + seed) * (a + 1)) % len(sp)]
    return xyz


def tri_special(G):
    """special coordinates: the borders +-1, outside them (clamped), 0, the pre-images of lattice nodes (kept where the f32 lattice coordinate
    is an integer) and one ulp either side of them (one ulp inside a cell face)"""
    v = [F32(1), F32(-1), F32(1.15), F32(-1.15), F32(2.5), F32(-2.5), F32(0), F32(-1.101), F32(1.101), F32(-1.1009), F32(1.1)]
    for k in range(G):
        x = F32(2.0 * 1.101 * (k / (G - 1) - 0.5))
        for c in (x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))):
            v.append(c)
    return np.array(v, F32)
