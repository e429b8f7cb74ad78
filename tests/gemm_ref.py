"""Float64 reference of the two f32 MFMA GEMMs (csrc/sgemm.hip, csrc/sgemm_sk.hip), the per-element error bound their tests assert,
mirrors of the host rules and of the device-side work split, and f32 emulations of deliberate mistakes (the mutants that prove the
bound has teeth).  Nothing here reuses a kernel's tiling or summation order for the VALUES; the mirrors restate the index arithmetic
of the work split only, so that a CPU test can say which launch forms a case reaches.

Operation (both entries; act 3, C2 and aux exist in the stream-K entry only)
    v = op(A) op(B)                                  MFMA chains, f32
    v = v + C[m, n]          when accumulate
    v = v + bias[n]          when bias
    pre = v                                          (C2[m, n] = pre when act == 2 and C2 is given)
    v = max(v, 0) | GELU(v) | v * GELU'(aux[m, n])   act 1 | 2 | 3
    v = v * dropout_mul(seed, m * N + n, p)          when p > 0  (train_ref.dropout_mul: 0, or 1 / (1 - p) formed in f32)
    v = v + resid[m, n]      when resid
    C[m, n] = v
C, C2, aux and resid are addressed with the row stride ldc; the dropout counter is m * N + n whatever ldc is.

Error bound (U = 2^-24, gamma(n) = n U / (1 - n U): train_ref.py)
  Product.  Every term a[m, k] b[k, n] is rounded when it is formed (not at all when the MFMA fuses it) and once per addition it
  takes part in afterwards.  Whatever the order - one chain, chunks of 32, a split of K into S slices whose partial sums are added by
  a second launch, stream-K slices added in workgroup order - a term takes part in at most K - 1 additions inside its slice and in at
  most c additions of slices, c = the number of slices (sgemm.hip: S) or of contributors of the tile (sgemm_sk.hip: at most
  ceil(K / 32)); the addition to the zeroed accumulator is exact.  So (Higham 3.1-3.3)
      |d P[m, n]| <= gamma(K + c) (|A| |B|)[m, n]                                                                          [PROD]
  for any summation order: split-K, stream-K and every grid share it.  The bound assumes only that the matrix core's
  v_mfma_f32_32x32x2_f32 rounds each of its two multiply-adds like an IEEE fused or unfused multiply-add.  No measured constant
  enters: the measured error / bound on an MI355X reaches 0.50 where the bound is tightest (K = 4: five roundings) and never exceeds 1
  (tests/test_gemm_kernels_gpu.py records it per family), so the assumption needed no correction.  The bound is a worst case: it
  grows with K^2 where the error of random operands grows with K, so at K = 2052 a correct product sits at 1e-3 of it - and a single
  dropped k index still lands at 15 x (tests/test_gemm_ref_cpu.py).
  Additions (accumulate, bias, residual): fl(x + y) for an x that carries the error b:  b' = b (1 + U) + U |x + y|.         [ADD]
  ReLU is exact and 1-Lipschitz: b' = b.
  GELU: |GELU'| <= 1.13 everywhere (maximum 1.1289 at x = sqrt 2, minimum -0.1289), so the pre-activation's error arrives as at most
  1.13 b; erff and the products add train_ref.gelu_ref's own bound g(x).  g is evaluated at the float64 pre-activation instead of the
  f32 one the kernel holds: g is a sum of terms U x (smooth function of x) with slopes <= 4 U, hence + 4 U b.
      b' = 1.13 b + g(pre) + 4 U b                                                                                          [GELU]
  GELU' multiply (act 3): fl(v * gp_f) with gp_f = sk_gelu_grad(aux) (== csrc/train.hip's gelu_grad: train_ref.gelu_bwd_ref gives
  |v| |d gp| + U |v gp| + TINY for an exact v):  b' = 1.13 b + gelu_bwd_ref(v, aux).bound + 4 U b.                           [GBWD]
  Dropout: one product with the f32 multiplier mul in {0, inv_keep(p)}:  b' = b mul + U |v mul|.                            [DROP]
  The pre-activation side output C2 carries the bound before the activation.
  The tests assert error / bound <= 1 per element (train_ref.ratio)."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import train_ref as T
from train_ref import U, f64, gamma, ratio, dropout_mul, inv_keep, gelu_ref, gelu_bwd_ref   # noqa: F401  (re-exported)

KC = 32                       # k per chunk, both files
SG_BM, SG_GM = 128, 8         # csrc/sgemm.hip: workgroup tile, M-tiles per panel
SK_GM = 8                     # csrc/sgemm_sk.hip: M-tiles per panel
SG_SLOTS = 512                # 256 CUs x 2 resident workgroups
SK_GRIDS = (256, 512, 768, 1024)
SK_GRID_DEFAULT = 512
GELU_SLOPE = 1.13
FORMS = ((0, 1), (0, 0), (1, 0), (1, 1))      # (transA, transB): y = x W^T, dX = dY W, dW = dY^T X, and the fourth


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- host rules
def mfma_splits(M, N, K):
    """sfmi_sgemm_mfma_splits"""
    blocks, nch, S = cdiv(M, SG_BM) * cdiv(N, SG_BM), cdiv(K, KC), 1
    while S < 8 and blocks * S * 2 <= SG_SLOTS and nch // (S * 2) >= 8:
        S *= 2
    return S


def mfma_launch_splits(M, N, K, ws_floats):
    """the S sfmi_sgemm_mfma_f32 launches with: ws_floats None = ws NULL; a scratch too small halves S until it fits"""
    S = 1 if ws_floats is None else mfma_splits(M, N, K)
    while S > 1 and S * M * N > ws_floats:
        S //= 2
    return S


def sk_tile(M, N, K, knob=0):
    """sfmi_sgemm_sk_tile (knob: the `sk_tile` setting)"""
    if knob:
        return knob
    return 2 if cdiv(M, 128) * cdiv(N, 128) * cdiv(K, KC) >= 12 * 512 else 1


def sk_cnt_ints(M, N):
    return 4 * cdiv(M, 64) * cdiv(N, 64)


def sk_slab_floats():
    return 1024 * 2 * 128 * 128


def _shape_ok(tA, tB, M, N, K, lda, ldb, ldc):
    if M <= 0 or N <= 0 or K <= 0 or N % 4 or lda % 4 or ldb % 4 or ldc % 4 or N < 4:
        return False
    if (not tA and K % 4) or (tB and K % 4) or (tA and (M % 4 or M < 4)):
        return False
    return lda >= (M if tA else K) and ldb >= (K if tB else N) and ldc >= N


def mfma_accepts(tA, tB, M, N, K, lda, ldb, ldc, act=0, ws_floats=0, drop_p=0.0, A=True, B=True, C=True):
    """True where sfmi_sgemm_mfma_f32 launches, False where it returns SFMI_EINVAL (include/sfmi.h)"""
    return bool(A and B and C and _shape_ok(tA, tB, M, N, K, lda, ldb, ldc) and 0 <= act <= 2 and ws_floats >= 0 and 0.0 <= drop_p < 1.0)


def sk_accepts(tA, tB, M, N, K, lda, ldb, ldc, act=0, aux=False, drop_p=0.0, slab_floats=None, cnt_ints=None, tile=0, grid=SK_GRID_DEFAULT,
               A=True, B=True, C=True, slab=True, cnt=True):
    """the same for sfmi_sgemm_sk_f32 / _sd_f32 (slab_floats / cnt_ints None: exactly what the launch needs)"""
    if not (A and B and C and slab and cnt and _shape_ok(tA, tB, M, N, K, lda, ldb, ldc)):
        return False
    if not (0 <= act <= 3) or (act == 3 and not aux) or not (0.0 <= drop_p < 1.0):
        return False
    p = sk_geometry(M, N, K, sk_tile(M, N, K, tile), grid)
    return (cnt_ints is None or cnt_ints >= 4 * p.tiles) and (slab_floats is None or slab_floats >= p.slab)


# ---------------------------------------------------------------------------------------------------- device-side work split
def xcd_remap(b, nb):
    """block b of nb runs on XCD b % 8; the remap gives every XCD one contiguous range of logical ids (both files)"""
    q, r, xcd, k = nb // 8, nb % 8, b % 8, b // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + k


def panel_tile(lid, nbm, nbn, gm=SG_GM):
    """logical tile id -> (M-tile, N-tile): panels of gm M-tiles, inside a panel the M-tiles of one N-tile are consecutive"""
    per_panel = gm * nbn
    panel = lid // per_panel
    rows = min(gm, nbm - panel * gm)
    r = lid - panel * per_panel
    return panel * gm + r % rows, r // rows


def sg_cuts(K, S):
    """[(c_lo, c_hi)] of the S slices of sgemm_mfma_kernel"""
    nch = cdiv(K, KC)
    return [(nch * s // S, nch * (s + 1) // S) for s in range(S)]


def sg_blocks(M, N):
    """[(M-tile, N-tile)] by blockIdx.x"""
    nbm, nbn = cdiv(M, SG_BM), cdiv(N, SG_BM)
    return [panel_tile(xcd_remap(b, nbm * nbn), nbm, nbn) for b in range(nbm * nbn)]


def sk_first_unit(v, U_, G):
    return v * U_ // G


def sk_owner(u, U_, G):
    return ((u + 1) * G - 1) // U_


Seg = namedtuple("Seg", "tile c_lo c_hi whole slot")
SkPlan = namedtuple("SkPlan", "TM BM nbm nbn C tiles units G slab wgs contributors")


def sk_geometry(M, N, K, TM, grid):
    BM = 64 * TM
    nbm, nbn, C = cdiv(M, BM), cdiv(N, BM), cdiv(K, KC)
    tiles = nbm * nbn
    G = min(grid, tiles * C)
    return SkPlan(TM, BM, nbm, nbn, C, tiles, tiles * C, G, G * 2 * BM * BM, None, None)


def sk_plan(M, N, K, TM, grid):
    """The launch as sgemm_sk_kernel walks it: wgs[v] = the segments of logical workgroup v (block b is v = xcd_remap(b, G));
    contributors[tile] = how many workgroups hold a slice of the tile (1: the direct epilogue)."""
    g = sk_geometry(M, N, K, TM, grid)
    C, U_, G = g.C, g.units, g.G
    wgs = []
    for v in range(G):
        lo, hi = sk_first_unit(v, U_, G), sk_first_unit(v + 1, U_, G)
        tile_lo, u, segs = lo // C, lo, []
        while u < hi:
            t = u // C
            c_lo = u - t * C
            c_hi = min(C, c_lo + (hi - u))
            whole = c_hi - c_lo == C
            segs.append(Seg(t, c_lo, c_hi, whole, None if whole else (0 if t == tile_lo else 1)))
            u += c_hi - c_lo
        wgs.append(segs)
    contrib = [sk_owner(t * C + C - 1, U_, G) - sk_owner(t * C, U_, G) + 1 for t in range(g.tiles)]
    return g._replace(wgs=wgs, contributors=contrib)


def wg_form(segs):
    """'w', 'p', 'pw', 'wp', 'pwp', 'pp': partial and whole segments in order, runs of whole tiles collapsed"""
    s = "".join("w" if x.whole else "p" for x in segs)
    while "ww" in s:
        s = s.replace("ww", "w")
    return s


def sk_reaches(M, N, K, TM, grid):
    """the set of work-split forms one stream-K launch reaches (names: SK_FORMS)"""
    p = sk_plan(M, N, K, TM, grid)
    out = set()
    for segs in p.wgs:
        out.add("wg:" + wg_form(segs))
        for s in segs:
            if not s.whole:
                n = s.c_hi - s.c_lo
                out.add(f"slot{s.slot}")
                out.add("partial:1" if n == 1 else "partial:odd" if n & 1 else "partial:even")
    for c in p.contributors:
        out.add("contrib:1" if c == 1 else "contrib:2" if c == 2 else "contrib:3-4" if c <= 4 else "contrib:5+")
    if p.G < grid:
        out.add("G<grid")
    if p.G % 8:
        out.add("G%8")
    if p.nbm % SK_GM:
        out.add("short-panel")
    if p.G == grid:
        out.add(f"grid:{grid}")
    if K % KC:
        out.add("ktail")
    if K % 4:
        out.add("K%4")
    return {f"t{TM}:{x}" for x in out}


SK_FORMS = tuple(f"t{t}:{x}" for t, xs in (
    (1, ("wg:w", "wg:p", "wg:pw", "wg:wp", "wg:pwp", "wg:pp", "slot0", "slot1", "partial:1", "partial:odd", "partial:even", "contrib:1", "contrib:2",
         "contrib:3-4", "contrib:5+", "G<grid", "G%8", "short-panel", "ktail", "K%4", "grid:256", "grid:512", "grid:768", "grid:1024")),
    (2, ("wg:w", "wg:p", "wg:pw", "wg:wp", "wg:pwp", "slot0", "slot1", "partial:1", "partial:odd", "partial:even", "contrib:1", "contrib:2", "contrib:3-4",
         "G<grid", "G%8", "short-panel", "ktail", "grid:256"))) for x in xs)


def sg_reaches(M, N, K, S):
    """the same for one sgemm.hip launch with S slices"""
    out = {f"S{S}"}
    nch = cdiv(K, KC)
    cuts = sg_cuts(K, S)
    if len({hi - lo for lo, hi in cuts}) > 1:
        out.add("uneven-cut")
    for lo, hi in cuts:
        out.add(f"chunks:{hi - lo}" if hi - lo <= 4 else "chunks:5+")
    if K % KC:
        out.add("ktail")
    if K % 4:
        out.add("K%4")
    nbm, nbn = cdiv(M, SG_BM), cdiv(N, SG_BM)
    if nbm % SG_GM:
        out.add("short-panel")
    if nbm > SG_GM and nbm % SG_GM:
        out.add("short-last-panel")
    if (nbm * nbn) % 8:
        out.add("blocks%8")
    out.add(f"Mrem:{M % SG_BM}/{nbm}")
    out.add(f"Nrem:{N % SG_BM}/{nbn}")
    out.add(f"Krem:{K % KC}/{min(nch, 5)}")
    return out


SG_FORMS = ("S1", "S2", "S4", "S8", "uneven-cut", "chunks:1", "chunks:2", "chunks:3", "chunks:4", "chunks:5+", "ktail", "K%4", "short-panel",
            "short-last-panel", "blocks%8")


# ---------------------------------------------------------------------------------------------------- operands
def operands(M, N, K, seed, epilogue=True):
    """Logical f32 A (M, K), B (K, N) whose rows / columns carry scales spread over 2^-10 .. 2^10 (per-element bounds then differ by
    orders of magnitude inside one tile), and C0, bias, resid of the product's magnitude; aux of the product's magnitude clipped to
    2^-6 .. 4, the range in which GELU' is not a constant.  epilogue=False: A and B only."""
    rs = np.random.RandomState(seed)
    ra, cb = 2.0 ** rs.uniform(-10, 10, (M, 1)), 2.0 ** rs.uniform(-10, 10, (1, N))
    A = (rs.randn(M, K) * ra).astype(np.float32)
    B = (rs.randn(K, N) * cb).astype(np.float32)
    if not epilogue:
        return dict(A=A, B=B)
    mag = ra * cb * math.sqrt(K)
    C0 = (rs.randn(M, N) * mag).astype(np.float32)
    bias = (rs.randn(N) * cb[0] * math.sqrt(K)).astype(np.float32)
    resid = (rs.randn(M, N) * mag).astype(np.float32)
    aux = (rs.randn(M, N) * np.clip(mag, 2.0 ** -6, 4.0)).astype(np.float32)
    return dict(A=A, B=B, C0=C0, bias=bias, resid=resid, aux=aux)


def stored(X, trans, ld=None, fill=np.nan):
    """the (rows, ld) array an entry reads for a logical operand: X^T when `trans`, padding columns filled"""
    S = np.ascontiguousarray(X.T if trans else X)
    ld = S.shape[1] if ld is None else ld
    out = np.full((S.shape[0], ld), fill, np.float32)
    out[:, :S.shape[1]] = S
    return out


# ---------------------------------------------------------------------------------------------------- reference and bound
def product_ref(A, B, c):
    """(P, bound) of [PROD] for logical A (M, K), B (K, N) and c slice / contributor additions"""
    A, B = f64(A), f64(B)
    return A @ B, gamma(A.shape[1] + c) * (np.abs(A) @ np.abs(B))


def abs_product(A, B):
    """(|A| |B|)[m, n] in float64: [PROD] is gamma(K + c) times this"""
    return np.abs(f64(A)) @ np.abs(f64(B))


def _add(v, b, y):
    v = v + y
    return v, b * (1 + U) + U * np.abs(v)


def epilogue_ref(P, bP, C0=None, bias=None, act=0, aux=None, resid=None, p=0.0, seed=0):
    """The epilogue in the kernel's order on the float64 product and its bound -> dict(y, b, pre, b_pre, keep (M, N) bool)."""
    M, N = P.shape
    v, b = P, bP
    if C0 is not None:
        v, b = _add(v, b, f64(C0))
    if bias is not None:
        v, b = _add(v, b, f64(bias)[None, :])
    pre, b_pre = v, b
    if act == 1:
        v = np.maximum(v, 0.0)
    elif act == 2:
        v, g = gelu_ref(pre)
        b = GELU_SLOPE * b + g + 4 * U * b
    elif act == 3:
        v, g = gelu_bwd_ref(pre, aux)
        b = GELU_SLOPE * b + g + 4 * U * b
    keep = np.ones((M, N), bool)
    if p > 0:
        mul = f64(dropout_mul(seed, np.arange(M * N, dtype=np.int64).reshape(M, N), p))
        keep = mul != 0
        v = v * mul
        b = b * mul + U * np.abs(v)
    if resid is not None:
        v, b = _add(v, b, f64(resid))
    return dict(y=v, b=b, pre=pre, b_pre=b_pre, keep=keep)


# ---------------------------------------------------------------------------------------------------- f32 emulations (mutants)
def product_f32(A, B, order="chunks", cuts=None):
    """A correct f32 product in one of several summation orders: 'blas' (numpy's sgemm), 'chunks' (32-deep chunks added in order),
    'reverse' (the chunks from the last to the first), 'slices' (cuts: [(c_lo, c_hi)] partial sums added in order)."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    K = A.shape[1]
    if order == "blas":
        return A @ B
    nch = cdiv(K, KC)
    part = lambda lo, hi: A[:, lo * KC:hi * KC] @ B[lo * KC:hi * KC]
    if order == "slices":
        parts = []
        for lo, hi in cuts:
            acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
            for c in range(lo, hi):
                acc = acc + part(c, c + 1)
            parts.append(acc)
    else:
        parts = [part(c, c + 1) for c in (range(nch) if order == "chunks" else reversed(range(nch)))]
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for x in parts:
        acc = acc + x
    return acc


def _tile(P, mt, nt, BM):
    return slice(mt * BM, min((mt + 1) * BM, P.shape[0])), slice(nt * BM, min((nt + 1) * BM, P.shape[1]))


def mut_drop_k(P32, A, B, mt, nt, BM, k):
    """one k index dropped in one tile"""
    r, c = _tile(P32, mt, nt, BM)
    out = P32.copy()
    out[r, c] -= np.outer(A[r, k], B[k, c]).astype(np.float32)
    return out


def mut_slice(P32, A, B, mt, nt, BM, c_lo, c_hi, times):
    """one contributor's slice [c_lo, c_hi) of one tile skipped (times = 0) or added twice (times = 2)"""
    r, c = _tile(P32, mt, nt, BM)
    out = P32.copy()
    out[r, c] += np.float32(times - 1) * (A[r, c_lo * KC:c_hi * KC] @ B[c_lo * KC:c_hi * KC, c])
    return out


def mut_swap(P32, band, pair, axis):
    """rows (axis 0) or columns (axis 1) 2 pair and 2 pair + 1 of one 64-wide band swapped: the interleaved order of the
    row-contiguous forms undone the wrong way"""
    i = 64 * band + 2 * pair
    out = P32.copy()
    if axis == 0:
        out[[i, i + 1]] = P32[[i + 1, i]]
    else:
        out[:, [i, i + 1]] = P32[:, [i + 1, i]]
    return out


EPILOGUE_MUTANTS = ("resid_ld", "aux_ld", "c2_ld", "drop_ld", "bias_after")


def _wrong_stride(buf, M, N):
    """element (m, n) of an (M, ldc) buffer read at m * N + n instead of m * ldc + n"""
    return buf.reshape(-1)[:M * N].reshape(M, N)


def epilogue_f32(P32, ldc, C0=None, bias=None, act=0, aux=None, resid=None, p=0.0, seed=0, mutant=None):
    """The epilogue in f32 on an f32 product, with the operands in (M, ldc) buffers as the kernel sees them (padding: zero) ->
    (C, C2) as (M, ldc) buffers, NaN where nothing was stored.  mutant: one of EPILOGUE_MUTANTS."""
    f = np.float32
    M, N = P32.shape
    pad = lambda x: None if x is None else stored(np.asarray(x, f), False, ldc, 0.0)
    rd = lambda buf, wrong: _wrong_stride(buf, M, N) if wrong else buf[:, :N]
    v = P32.astype(f)
    if C0 is not None:
        v = v + pad(C0)[:, :N]
    if bias is not None and mutant != "bias_after":
        v = v + np.asarray(bias, f)[None, :]
    pre = v
    e32 = lambda x: T._erf(x.astype(np.float64) * math.sqrt(0.5))
    if act == 1:
        v = np.maximum(v, f(0))
    elif act == 2:
        v = (0.5 * pre.astype(np.float64) * (1.0 + e32(pre))).astype(f)
    elif act == 3:
        h = rd(pad(aux), mutant == "aux_ld").astype(np.float64)
        gp = (0.5 * (1.0 + T._erf(h * math.sqrt(0.5))) + h * T.K_PDF * np.exp(-0.5 * h * h)).astype(f)
        v = v * gp
    if bias is not None and mutant == "bias_after":
        v = v + np.asarray(bias, f)[None, :]
    if p > 0:
        m, n = np.arange(M, dtype=np.int64)[:, None], np.arange(N, dtype=np.int64)[None, :]
        v = v * dropout_mul(seed, m * (ldc if mutant == "drop_ld" else N) + n, p)
    if resid is not None:
        v = v + rd(pad(resid), mutant == "resid_ld")
    C = np.full((M, ldc), np.nan, f)
    C[:, :N] = v
    C2 = np.full((M, ldc), np.nan, f)
    if act == 2:
        if mutant == "c2_ld":
            C2.reshape(-1)[:M * N] = pre.reshape(-1)
        else:
            C2[:, :N] = pre
    return C, C2
