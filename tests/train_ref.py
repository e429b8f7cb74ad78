"""Float64 references of the training-step kernels of csrc/train.hip, the per-element error bounds their tests assert, and mirrors of the
host rules that choose a launch form.

Kernels: transpose_kernel, colsum_kernel, colsum_part / colsum_finish, col_reduce_kernel (kinds 0 and 1), gelu_fwd / gelu_bwd,
ln_bwd_rows_kernel (block per row) and ln_bwd_rows_wave_kernel<NE> (wave per row), ln_bwd_params_part / _finish, ce_fwd_bwd_kernel,
embed_scatter_kernel + fixed_to_float_kernel, dropout_kernel, add_kernel, adamw_kernel / adamw_multi_kernel / unflatten_multi_kernel,
attn_train_fwd_kernel / attn_prefill_mfma_kernel (csrc/gpt.hip) with the row log-sum-exps, attn_delta_kernel / attn_stats_mfma_kernel and
attn_bwd_fused_kernel<RW, NG>.  The references restate each operation in float64 (numpy) on the f32 inputs the kernel sees; nothing
here reuses a kernel's tiling or summation order.

Error bounds
  U = 2^-24, gamma(n) = n U / (1 - n U) (decode_ref.py; Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., 3.1-3.3): a sum
  in which every term passes through at most n roundings is off by at most gamma(n) sum |term|.  A product, a sum, a division and sqrtf
  round once (all four are correctly rounded on gfx950: measured 1.0000 U below); a fused multiply-add rounds once, so counting the
  product and the add separately is the worst case whatever the compiler contracts.  Every bound is per output element.

  Intrinsics that are NOT correctly rounded.  Measured alone on one MI355X (ROCm 7.2, 2^22 arguments per range, against float64 libm),
  in units of U, relative to the exact result unless said otherwise:
      erff      [-29, 29] 1.94   [-4, 4] 1.97   [1e-31, 1] (log-spaced) 2.00         (absolute: 1.40)
      __expf    [-1, 0] 1.83   [-10, 0] 8.68   [-20, 1] 16.4   [-87, 1] 64.0; divided by (1 + |x|): 1.01 / 1.13 / 1.28 / 1.30 - the
                argument's scaling by log2 e rounds relative to |x|; [-800, -87]: the result is flushed to 0 (exact value < 2^-125)
      __logf    [1, 8192] (log-spaced) 2.97   [1, 1.01] 2.92   [1, 2] 2.93
      rsqrtf    [1e-5, 1e4] (log-spaced) 1.57
  The constants below are the measured maxima times two (compiler-version drift):
      E_ERF = 4.0    |d erff(z)| <= E_ERF U |erf z|
      E_EXP = 2.6    |d __expf(x)| <= E_EXP (1 + |x|) U exp(x) + TINY         x in [-800, 1]
      E_LOG = 6.0    |d __logf(x)| <= E_LOG U |log x|                         x in [1, 8192]
      E_RSQRT = 3.2  |d rsqrtf(x)| <= E_RSQRT U / sqrt(x)                     x in [1e-5, 1e4]
  TINY = 2^-120 covers results and intermediate products flushed below the normal range.

  Column sums.  [COL]
      colsum_kernel        a row lane adds ceil(M / 4) rows one after the other, a 2-level tree joins the 4 lanes, `accumulate` adds once:
                           n = ceil(M / 4) + 2 + 1
      colsum_part / finish rows_per = ceil(M / RS) rows per slice: n = ceil(rows_per / 4) + 2, then the RS slices serially, + 1: + RS + 1
      col_reduce_kernel    16 row lanes: ceil(rows_per / 16), the 16 lanes added serially (16), RS slices serially, + 1
      |err| <= gamma(n) sum_m |term|.  The LayerNorm-parameter term dy (x - mean) rstd (kind 1, ln_bwd_params_part) takes the row
      statistics as f32 INPUTS (the reference reads the same (M, 2) array) and rounds three more times: n + 3.

  GELU.  z = x * f32(1 / sqrt 2): the constant and the product round, and erf' (z) z = (2 / sqrt pi) z exp(-z^2) <= 0.484, so
      e1 = |d (1 + erff z)| <= 0.97 U + E_ERF U |erf z| + U |1 + erf z|,   |d gelu| <= 0.5 |x| e1 (1 + U) + U |gelu| + TINY          [GELU]
  (0.5 x is exact).  GELU' = 0.5 (1 + erf z) + x k exp(-x^2 / 2): a = -0.5 x x rounds once (U |a| absolute in the exponent), x k twice,
  the product with the exponential once:
      |d B| <= |B| (3 U + U |a| + E_EXP (1 + |a|) U),   |d gelu'| <= 0.5 e1 + |d B| + U |gelu'|,   |d dx| <= |dy| |d gelu'| + U |dx| + TINY

  LayerNorm backward, row part.  A row sum has depth ns = NE + 6 (wave form: NE = D / 64 elements per lane, a 6-level butterfly) or
  ns = ceil(D / 256) + 8 (block form: + the 2-level tree over the 4 waves).  With E|.| the row mean of absolute values:                 [LN]
      |d mean| = dm <= gamma(ns + 1) E|x|
      var_f = mean (x - mean_f)^2 = var + (mean_f - mean)^2 exactly; each difference rounds once, each square once more:
      |d var| <= dm^2 + gamma(ns + 4) (var + dm^2);   e = |d var| / (var + eps);   e_r = e / (2 (1 - e)^1.5) + (1 + E_RSQRT) U   (relative, rstd)
      |d xhat| = dxh <= rstd (1 + e_r) (dm + U |x - mean|) + |xhat| (e_r + U)      - a constant row has xhat = 0 and |d xhat| <= rstd dm
      g = dy gamma: U |g|;  |d ma| <= gamma(ns + 2) E|g|;  |d mb| = dmb <= E(|g| dxh) + gamma(ns + 3) E|g xhat|
      t = g - ma - xhat mb:  dt <= U |g| + dma + |xhat| dmb + |mb| dxh + dxh dmb + U |xhat mb| + U (|g| + |ma|) + U (|g| + |ma| + |xhat mb|)
      dx = rstd t (+ dres):  |d dx| <= rstd (1 + e_r) dt + |rstd t| (e_r + U) + U |dx|
  x = 100 + randn loses 7 bits in x - mean: dm ~ 1e-5 is the dominant term, as it is in the kernel.

  Cross entropy.  x_v = logit_v - max (one rounding: U |x_v| in the exponent), p_v = __expf(x_v):  r_v = U |x_v| + E_EXP (1 + |x_v|) U.   [CE]
      tot = sum_v p_v over ceil(V / 256) + 6 + 2 levels:  e_t = sum_v p_v r_v / tot + gamma(ceil(V / 256) + 8) (+ V TINY), relative
      loss = max + __logf(tot) - logit_tg:  |d loss| <= e_t + E_LOG U log tot + U |max + log tot| + U |loss|
      dlogit_v = (p_v / tot - [v = tg]) scale:  <= |scale| (p_v / tot (r_v + e_t + U) + U |p_v / tot - onehot|) + U |dlogit_v| + TINY

  Embedding scatter: sum_m rint(dx 2^32) in int64 is exact and order-free; (float)(acc 2^-32) rounds once.  Each term is off by at most
  2^-33, so against the float64 sum  |err| <= count 2^-33 + U |sum| (+ U |out + sum| when it accumulates).                               [FIX]

  AdamW.  The bias corrections are f32 INPUTS (sfmi_adamw_bias_corrections forms them on the host; its own test compares them with
  float64: glibc's powf is within 1 ulp, so |d bc| <= 2 U beta^t + U bc).  Per element, with s = sqrt(v') / sqrt(bc2):                   [ADAM]
      m' = b1 m + (1 - b1) g:   dm <= U |b1 m| + 2 U |(1 - b1) g| + U |m'|
      v' = b2 v + (1 - b2) g g: dv <= U |b2 v| + 3 U |(1 - b2) g g| + U |v'| <= 4 U v'
      denom = s + eps:  dden <= s (dv / (2 v') + 3 U) + U denom   (sqrtf, sqrtf(bc2), the division, the add)
      upd = (lr / bc1) m' / denom:  dupd <= (lr / bc1) dm / denom + |upd| (dden / denom + 3 U)
      p' = p (1 - lr wd) - upd:  <= |p (1 - lr wd)| 3 U + dupd + U |p'|

  Attention.  Scores s = (q / 8) . k along an MFMA chain of 64 products (a 16x16x4 MFMA counts as four sequential fused multiply-adds;
  q / 8 is exact):  ds <= gamma(64) sum |q k| / 8.  Online softmax over nb = ceil(keys / 64) blocks; with x = s - m, m the row maximum
  and R = m - min s (every running maximum lies between):                                                                           [ATTN]
      eps_p = max_k (ds_k + U |x_k| + E_EXP (1 + |x_k|) U) + (nb + 1) (E_EXP (1 + R) + 2) U      (each block's rescale, the group merge)
      l = sum p: 4 + 4 levels per block, two roundings per block:  e_l = expm1(eps_p) + gamma(10 + 2 nb)
      lse = m + __logf(l):  |d lse| <= e_l + E_LOG U log l + U |lse|
      y = sum_k p_k mask_k v_k / l along a chain over the keys (+ one rescale per block, the mask product, 1 / l and the final product):
      |d y| <= (expm1(eps_p) + gamma(keys + nb + 4)) sum_k p_k mask_k |v_k| / l + |y| (e_l + 2 U)
      delta = sum_d dO O (O = the f32 y the backward pass reads): n = max(H + 6, 18) + 1
  Backward (recompute form): P = __expf(s - lse) with the f32 lse:  rP = ds + d lse + U |x| + E_EXP (1 + |x|) U, x = s - lse;
      dP = dO . v (gamma(64) sum |dO v|);  t = dP mask - delta:  dt <= mask ddP + U |dP mask| + d delta + U |t|
      dS = P t:  ddS <= P dt + |dS| (rP + U);   dQ = sum_k dS k / 8, dK = sum_q dS q / 8, dV = sum_q P mask dO along chains of
      n = rows + 3 (the group exchange adds once, the final scale is exact):
      |d dQ| <= (sum_k ddS |k| + gamma(n) sum_k |dS k|) / 8, dK alike;  |d dV| <= sum_q P mask |dO| (rP + U) + gamma(n) sum_q P mask |dO|
"""
from __future__ import annotations

import math

import numpy as np

from decode_ref import U, LN_EPS

E_ERF, E_EXP, E_LOG, E_RSQRT = 4.0, 2.6, 6.0, 3.2        # module docstring: measured maxima x 2, in units of U
TINY = 2.0 ** -120
FIX = 2.0 ** 32                                           # embedding gradients: 2^-32 fixed point
LN_WAVE_WIDTHS = (128, 256, 512, 1024)                    # sfmi_layernorm_bwd_rows_drop_sd_f32: D with a wave-per-row instance


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


# ---------------------------------------------------------------------------------------------------- launch-form mirrors
COLSUM_TARGET_BLOCKS, COLSUM_MAX_SLICES, COLSUM_MIN_ROWS = 2048, 128, 16       # sfmi_colsum_slices
CR_DIRECT_ROWS, CR_ROWS_PER_SLICE, CR_MAX_SLICES = 1024, 512, 16               # sfmi_col_reduce_slices
ATTN_BWD_SMALL_WG, ATTN_FWD_SMALL_WG = 256, 128                                # attn_bwd_fused_launch, sfmi_attn_train_fwd_small_sd_f32


def colsum_slices(M, N):
    """sfmi_colsum_slices: enough (64-column block, slice) pairs to fill the chip, at most 128 slices, at least 16 rows each."""
    cb = (N + 63) // 64
    rs = min((COLSUM_TARGET_BLOCKS + cb - 1) // cb, COLSUM_MAX_SLICES, M // COLSUM_MIN_ROWS)
    return max(rs, 1)


def col_reduce_slices(M):
    """sfmi_col_reduce_slices."""
    return 1 if M <= CR_DIRECT_ROWS else min((M + CR_ROWS_PER_SLICE - 1) // CR_ROWS_PER_SLICE, CR_MAX_SLICES)


def ln_rows_form(D):
    """'wave' (ln_bwd_rows_wave_kernel<D / 64>) or 'block' (ln_bwd_rows_kernel, dropout as its own launch)."""
    return "wave" if D in LN_WAVE_WIDTHS else "block"


def attn_bwd_form(B, L, H):
    """(RW, NG) of the attn_bwd_fused_kernel instance attn_bwd_fused_launch picks."""
    nqb = (L + 63) // 64
    return (2, 2) if B * H * 2 * nqb <= ATTN_BWD_SMALL_WG and nqb > 1 else (4, 1)


def attn_fwd_small(B, L, H):
    """True where sfmi_attn_train_fwd_small_f32 accepts the launch (else SFMI_EINVAL: use sfmi_gpt_attn_prefill_lse_f32)."""
    return B * H * ((L + 63) // 64) <= ATTN_FWD_SMALL_WG


def colsum_depth(kind, M, N=0):
    """n of [COL] for kind in 'plain', 'ws', 'col_reduce' (without the + 3 of a LayerNorm-parameter term)."""
    if kind == "plain":
        return -(-M // 4) + 2 + 1
    if kind == "ws":
        RS = colsum_slices(M, N)
        return -(-(-(-M // RS)) // 4) + 2 + RS + 1
    RS = col_reduce_slices(M)
    return -(-(-(-M // RS)) // 16) + 16 + RS + 1


def ln_sum_depth(D):
    return D // 64 + 6 if ln_rows_form(D) == "wave" else -(-D // 256) + 8


# ---------------------------------------------------------------------------------------------------- transpose / column sums
def transpose_ref(x, Rpad):
    """out (C, Rpad) = x^T, columns R .. Rpad - 1 zero."""
    x = np.asarray(x)
    out = np.zeros((x.shape[1], Rpad), x.dtype)
    out[:, :x.shape[0]] = x.T
    return out


def colsum_ref(a, n, prev=None):
    """(sum_m a, bound) for a (M, N) f32 terms-as-given; prev: the values `accumulate` adds to."""
    a = f64(a)
    s, sa = a.sum(0), np.abs(a).sum(0)
    if prev is not None:
        s, sa = s + f64(prev), sa + np.abs(f64(prev))
    return s, gamma(n) * sa


def ln_param_terms(dy, x, stats):
    """float64 dy (x - mean) rstd with the f32 row statistics (M, 2) the kernel reads."""
    st = f64(stats)
    return f64(dy) * (f64(x) - st[:, :1]) * st[:, 1:2]


# ---------------------------------------------------------------------------------------------------- GELU
_erf = np.vectorize(math.erf, otypes=[np.float64])
K_PDF = 0.3989422804014327


def _e1(x):
    er = _erf(x * math.sqrt(0.5))
    return er, 0.97 * U + E_ERF * U * np.abs(er) + U * np.abs(1.0 + er)


def gelu_ref(x):
    x = f64(x)
    er, e1 = _e1(x)
    y = 0.5 * x * (1.0 + er)
    return y, 0.5 * np.abs(x) * e1 * (1 + U) + U * np.abs(y) + TINY


def gelu_bwd_ref(dy, x):
    dy, x = f64(dy), f64(x)
    er, e1 = _e1(x)
    a = -0.5 * x * x
    Bt = x * K_PDF * np.exp(a)
    gp = 0.5 * (1.0 + er) + Bt
    dB = np.abs(Bt) * (3 * U + U * np.abs(a) + E_EXP * (1 + np.abs(a)) * U)
    dgp = 0.5 * e1 + dB + U * np.abs(gp)
    dx = dy * gp
    return dx, np.abs(dy) * dgp + U * np.abs(dx) + TINY


# ---------------------------------------------------------------------------------------------------- LayerNorm backward
def ln_bwd_rows_ref(dy, x, gam, dres, ns, eps=LN_EPS):
    """dict(dx, stats (M, 2), b_dx, b_stats) of [LN] for row-sum depth ns (ln_sum_depth(D))."""
    dy, x, gam = f64(dy), f64(x), f64(gam)
    E = lambda a: a.mean(1, keepdims=True)
    mean = E(x)
    var = E((x - mean) ** 2)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (x - mean) * rstd
    g = dy * gam
    ma, mb = E(g), E(g * xh)
    t = g - ma - xh * mb
    v0 = rstd * t
    dx = v0 if dres is None else v0 + f64(dres)
    dm = gamma(ns + 1) * E(np.abs(x))
    dvar = dm ** 2 + gamma(ns + 4) * (var + dm ** 2)
    e = dvar / (var + eps)
    assert float(e.max()) < 0.5
    e_r = e / (2 * (1 - e) ** 1.5) + (1 + E_RSQRT) * U
    dxh = rstd * (1 + e_r) * (dm + U * np.abs(x - mean)) + np.abs(xh) * (e_r + U)
    dma = gamma(ns + 2) * E(np.abs(g))
    dmb = E(np.abs(g) * dxh) + gamma(ns + 3) * E(np.abs(g * xh))
    xm = np.abs(xh * mb)
    dt = (U * np.abs(g) + dma + np.abs(xh) * dmb + np.abs(mb) * dxh + dxh * dmb + U * xm + U * (np.abs(g) + np.abs(ma))
          + U * (np.abs(g) + np.abs(ma) + xm))
    b = rstd * (1 + e_r) * dt + np.abs(v0) * (e_r + U) + U * np.abs(dx)
    return dict(dx=dx, stats=np.concatenate([mean, rstd], 1), b_dx=b, b_stats=np.concatenate([dm, rstd * e_r], 1))


# ---------------------------------------------------------------------------------------------------- cross entropy
def ce_ref(logits, target, V, L, t0, scale):
    """logits (M, ld): dict(loss (M,), dlogits (M, ld), b_loss, b_dl, active (M,) bool) of [CE]."""
    z = f64(logits)
    scale = float(np.float32(scale))                              # the f32 value the entry receives
    M, ld = z.shape
    tg = np.asarray(target).astype(np.int64)
    act = (np.arange(M) % L) >= t0
    zz = z[:, :V]
    mx = zz.max(1, keepdims=True)
    x = zz - mx
    p = np.exp(x)
    tot = p.sum(1, keepdims=True)
    r = U * np.abs(x) + E_EXP * (1 + np.abs(x)) * U
    e_t = (p * r).sum(1, keepdims=True) / tot + gamma(-(-V // 256) + 8) + V * TINY
    lt = np.log(tot)
    loss = (mx + lt)[:, 0] - zz[np.arange(M), tg]
    b_loss = (e_t + E_LOG * U * lt + U * np.abs(mx + lt))[:, 0] + U * np.abs(loss)
    oh = np.zeros_like(zz)
    oh[np.arange(M), tg] = 1.0
    sm = p / tot
    dl = np.zeros((M, ld))
    bd = np.zeros((M, ld))
    dl[:, :V] = (sm - oh) * scale
    bd[:, :V] = abs(scale) * (sm * (r + e_t + U) + U * np.abs(sm - oh)) + U * np.abs(dl[:, :V]) + TINY
    dl[~act], bd[~act], loss[~act], b_loss[~act] = 0.0, 0.0, 0.0, 0.0
    return dict(loss=loss, dlogits=dl, b_loss=b_loss, b_dl=bd, active=act)


# ---------------------------------------------------------------------------------------------------- embedding scatter
def scatter_fixed_ref(dx, idx, rows, prev=None, trunc=False):
    """The exact fixed-point result, bit for bit: (float)(sum_m rint(dx 2^32) 2^-32) (+ prev in f32).  trunc: a MUTANT (truncation)."""
    dx = np.asarray(dx, np.float32)
    q = dx.astype(np.float64) * FIX
    q = (np.trunc(q) if trunc else np.rint(q)).astype(np.int64)
    acc = np.zeros((rows, dx.shape[1]), np.int64)
    np.add.at(acc, np.asarray(idx).astype(np.int64), q)
    v = (acc.astype(np.float64) * (1.0 / FIX)).astype(np.float32)
    return v if prev is None else (np.asarray(prev, np.float32) + v).astype(np.float32)


def scatter_ref(dx, idx, rows, prev=None):
    """(float64 sum, [FIX] bound)."""
    dx = f64(dx)
    idx = np.asarray(idx).astype(np.int64)
    s = np.zeros((rows, dx.shape[1]))
    np.add.at(s, idx, dx)
    cnt = np.bincount(idx, minlength=rows).astype(np.float64)[:, None]
    b = cnt * 2.0 ** -33 + U * np.abs(s)
    if prev is not None:
        s = s + f64(prev)
        b = b + U * np.abs(s)
    return s, b


# ---------------------------------------------------------------------------------------------------- dropout
def hash_unit_idx(seed, idx):
    """weights.hash_unit's arithmetic for an integer seed at the flat indices idx (any shape): f32 in [0, 1)."""
    with np.errstate(over="ignore"):
        h = np.asarray(idx).astype(np.uint32) * np.uint32(0x9E3779B1) + np.uint32(seed & 0xFFFFFFFF)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / (1 << 24))


def inv_keep(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def dropout_mul(seed, idx, p):
    """f32 multiplier of sfmi_dropout_mul: 0 where hash < p, else 1 / (1 - p) formed in f32."""
    return np.where(hash_unit_idx(seed, idx) < np.float32(p), np.float32(0), inv_keep(p)).astype(np.float32)


def attn_mask(seed, B, H, L, p, swap=False):
    """(B, H, L, L) multiplier of element (b, h, query, key): flat index ((b H + h) L + q) L + key.  swap: a MUTANT (query and key swapped)."""
    i = np.arange(B * H * L * L, dtype=np.int64).reshape(B, H, L, L)
    m = dropout_mul(seed, i, p) if p > 0 else np.ones((B, H, L, L), np.float32)
    return m.transpose(0, 1, 3, 2).copy() if swap else m


# ---------------------------------------------------------------------------------------------------- AdamW
def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2):
    """torch.optim.AdamW semantics in float64 on f32 inputs (lr, betas, eps, wd, bc1, bc2 as the f32 values the kernel receives).
    Returns dict(p, m, v, b_p, b_m, b_v) of [ADAM]."""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    lr, b1, b2, eps, wd, bc1, bc2 = (float(np.float32(a)) for a in (lr, b1, b2, eps, wd, bc1, bc2))
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * g * g
    s = np.sqrt(v1) / math.sqrt(bc2)
    den = s + eps
    step = lr / bc1
    upd = step * m1 / den
    pd = p * (1 - lr * wd)
    p1 = pd - upd
    dm = U * np.abs(b1 * m) + 2 * U * np.abs((1 - b1) * g) + U * np.abs(m1)
    dv = U * np.abs(b2 * v) + 3 * U * np.abs((1 - b2) * g * g) + U * np.abs(v1)
    dden = s * (4 * U / 2 + 3 * U) + U * den
    dupd = step * dm / den + np.abs(upd) * (dden / den + 3 * U)
    return dict(p=p1, m=m1, v=v1, b_p=np.abs(pd) * 3 * U + dupd + U * np.abs(p1) + TINY, b_m=dm + TINY, b_v=dv + TINY)


def bias_corrections_ref(b1, b2, step):
    """(bc (2,), bound (2,)) for the f32 betas."""
    b = np.array([float(np.float32(b1)), float(np.float32(b2))])
    bt = b ** step
    return 1 - bt, 2 * U * bt + U * (1 - bt)


# ---------------------------------------------------------------------------------------------------- attention
def _heads(a, B, L, H):
    return a.reshape(B, L, H, 64).transpose(0, 2, 1, 3)           # (B, H, L, 64)


def _unheads(a):
    B, H, L, _ = a.shape
    return a.transpose(0, 2, 1, 3).reshape(B * L, H * 64)


def _qk(a, b):
    """(.., q, d) x (.., k, d) -> (.., q, k)"""
    return a @ np.swapaxes(b, -1, -2)


def _pv(a, b):
    """(.., q, k) x (.., k, d) -> (.., q, d)"""
    return a @ b


def _tq(a, b):
    """(.., q, k) x (.., q, d) -> (.., k, d)"""
    return np.swapaxes(a, -1, -2) @ b


def attn_fwd_ref(qkv, B, L, H, mask=None):
    """Causal attention of qkv (B L, 3 D) with the explicit dropout multiplier mask (B, H, L, L) applied to P after the row sum.
    dict(y (B L, D), lse (B, H, L), b_y, b_lse, + internals for attn_bwd_ref)."""
    D = 64 * H
    x = f64(qkv)
    q, k, v = (_heads(x[:, i * D:(i + 1) * D], B, L, H) for i in range(3))
    s = _qk(q, k) / 8.0
    sabs = _qk(np.abs(q), np.abs(k)) / 8.0
    live = np.tril(np.ones((L, L), bool))
    mk = np.ones((B, H, L, L)) if mask is None else f64(mask)
    sm = np.where(live, s, -np.inf)
    mx = sm.max(-1, keepdims=True)
    xx = np.where(live, s - mx, 0.0)
    p = np.where(live, np.exp(xx), 0.0)
    l = p.sum(-1, keepdims=True)
    lse = (mx + np.log(l))[..., 0]
    P = p / l
    y = _pv(P * mk, v)
    keys = np.arange(1, L + 1, dtype=np.float64).reshape(1, 1, L, 1)
    nb = np.ceil(keys / 64)
    ds = gamma(64) * sabs
    R = mx - np.where(live, s, np.inf).min(-1, keepdims=True)
    eps_k = np.where(live, ds + U * np.abs(xx) + E_EXP * (1 + np.abs(xx)) * U, 0.0)
    eps_p = eps_k.max(-1, keepdims=True) + (nb + 1) * (E_EXP * (1 + R) + 2) * U
    e_l = np.expm1(eps_p) + gamma(10 + 2 * nb)
    b_lse = (e_l + E_LOG * U * np.log(l))[..., 0] + U * np.abs(lse)
    ya = _pv(P * mk, np.abs(v))
    b_y = (np.expm1(eps_p) + gamma(keys + nb + 4)) * ya + np.abs(y) * (e_l + 2 * U)
    return dict(y=_unheads(y), lse=lse, b_y=_unheads(b_y), b_lse=b_lse, q=q, k=k, v=v, s=s, ds=ds, P=P, mk=mk, live=live)


def delta_ref(y, dy, B, L, H):
    """delta (B, H, L) = sum_d dO O for the f32 y the backward pass reads, and its bound."""
    yy, dd = _heads(f64(y), B, L, H), _heads(f64(dy), B, L, H)
    n = max(H + 6, 18) + 1
    return (yy * dd).sum(-1), gamma(n) * np.abs(yy * dd).sum(-1)


def attn_bwd_ref(fw, dy, B, L, H):
    """dqkv (B L, 3 D) and its bound from attn_fwd_ref's dict fw (float64 throughout: lse and delta are the exact ones, their f32
    errors enter the bound)."""
    q, k, v, P, mk, live = fw["q"], fw["k"], fw["v"], fw["P"], fw["mk"], fw["live"]
    do = _heads(f64(dy), B, L, H)
    yh = _pv(P * mk, v)
    delta = (do * yh).sum(-1, keepdims=True)
    n_d = max(H + 6, 18) + 1
    # the f32 delta is formed from the f32 y: |d delta| <= sum_d |dO| |d y| + gamma(n_d) sum |dO y|
    b_yh = _heads(fw["b_y"], B, L, H)
    d_delta = (np.abs(do) * b_yh).sum(-1, keepdims=True) + gamma(n_d) * np.abs(do * yh).sum(-1, keepdims=True)
    dP = _qk(do, v)
    ddP = gamma(64) * _qk(np.abs(do), np.abs(v))
    x = np.where(live, fw["s"] - fw["lse"][..., None], 0.0)
    rP = fw["ds"] + fw["b_lse"][..., None] + U * np.abs(x) + E_EXP * (1 + np.abs(x)) * U
    t = dP * mk - delta
    dt = mk * ddP + U * np.abs(dP * mk) + d_delta + U * np.abs(t)
    dS = P * t
    ddS = P * dt + np.abs(dS) * (rP + U) + np.where(live, TINY, 0.0)
    n = L + 3
    dq = _pv(dS, k) / 8.0
    b_dq = (_pv(ddS, np.abs(k)) + gamma(n) * _pv(np.abs(dS), np.abs(k))) / 8.0
    dk = _tq(dS, q) / 8.0
    b_dk = (_tq(ddS, np.abs(q)) + gamma(n) * _tq(np.abs(dS), np.abs(q))) / 8.0
    Pm = P * mk
    dv = _tq(Pm, do)
    b_dv = _tq(Pm * (rP + U + gamma(n)), np.abs(do))
    cat = lambda a, b_, c: np.concatenate([_unheads(a), _unheads(b_), _unheads(c)], 1)
    return dict(dqkv=cat(dq, dk, dv), b_dqkv=cat(b_dq, b_dk, b_dv) + TINY, delta=delta[..., 0], b_delta=d_delta[..., 0])


def ratio(got, ref, bound):
    """max |got - ref| / bound; a non-finite value or an error at a zero bound gives inf."""
    got, ref, bound = f64(got), f64(ref), np.broadcast_to(f64(bound), np.shape(ref))
    if not np.isfinite(got).all():
        return math.inf
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    return float(r.max()) if r.size else 0.0


# ---------------------------------------------------------------------------------------------------- a whole step against the float64 oracle
def oracle_grads(sd, cfg, c, z, dropout, dtype):
    """(loss, {key: gradient}) of oracle.gpt_oracle.training_loss by CPU autograd with the state dict in `dtype` (float64: the reference;
    float32: the yardstick whose own error sets the gate)."""
    import torch
    from oracle import gpt_oracle as GO, tokens_oracle as TO
    sdt = {k: torch.from_numpy(np.asarray(v)).to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    extra = torch.from_numpy(TO.extra_indices_AR_N(c.numpy(), z.numpy(), 4096))
    loss = GO.training_loss(sdt, cfg, c, z, extra, dropout=dropout)
    loss.backward()
    return float(loss.item()), {k: v.grad for k, v in sdt.items()}


def oracle_pair(sd, cfg, c, z, dropout):
    """(float64 loss, float64 gradients, fp32 gradients) of the oracle: what step_ratios compares a trainer with."""
    import torch
    l64, g64 = oracle_grads(sd, cfg, c, z, dropout, torch.float64)
    return l64, g64, oracle_grads(sd, cfg, c, z, dropout, torch.float32)[1]


def step_ratios(sd, cfg, c, z, dropout, name_map, get, oracle=None):
    """Per trainer tensor (name_map: trainer name -> oracle keys; get(name) -> the trainer's gradient on the CPU): the max-normalised error
    of the trainer and of the oracle's own fp32 autograd against the float64 oracle, and their ratio with the fp32 error floored at U.
    oracle: a precomputed oracle_pair of the same arguments.  Returns (float64 loss, [(name, e_gpu, e_cpu, ratio)])."""
    import torch
    l64, g64, g32 = oracle if oracle is not None else oracle_pair(sd, cfg, c, z, dropout)
    cat = lambda g, keys: torch.cat([g[k].reshape(-1, g[k].shape[-1]) if g[k].dim() > 1 else g[k] for k in keys], 0).double()
    rows = []
    for name, keys in name_map.items():
        w64, w32 = cat(g64, keys), cat(g32, keys)
        scale = float(w64.abs().max()) + 1e-300
        e_cpu = float((w32 - w64).abs().max()) / scale
        e_gpu = float((get(name).double().reshape(w64.shape) - w64).abs().max()) / scale
        rows.append((name, e_gpu, e_cpu, e_gpu / max(e_cpu, U)))
    return l64, rows
