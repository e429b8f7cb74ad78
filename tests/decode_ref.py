"""Float64 references of the decode-step kernels of csrc/gpt.hip and the per-element error bounds their tests assert.

Kernels: dgemm_kernel (decode GEMM: LayerNorm fold, GELU, residual, split-K; launcher decode_gemm_launch), attn_decode_kernel (one new
position per row against the KV cache, optional shared prefix) and attn_prefill_mfma_kernel (causal attention over a prefix, fills the
cache).  The references restate the model (mingpt.py:73-111) in float64 on the f32 inputs the kernels see; nothing here reuses the
kernels' summation order, so a legitimate change of that order passes on numbers, not on bit patterns.

Layouts
  pack(a, rows)     (R, C) row-major -> fragment-packed [rows/16][C/16][64 lanes][4], lane = ((c >> 2) & 3) * 16 + (r & 15), j = c & 3
                    (gpt.hip pk_off).  The decode activations use it with (r, c) = (row, feature); the weight pack Wp16 of
                    sfmi_skinny16_pack_weight is the same map with (r, c) = (output n, input k), so one function serves both.
  unpack(p, R, C)   the inverse (rows >= R dropped).

Error bounds
  u = 2^-24 (f32, round to nearest), gamma(n) = n u / (1 - n u).  A sum evaluated along a tree in which every term passes through at
  most n roundings is off by at most gamma(n) * sum |term| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., 3.1-3.3);
  a product counts as one rounding.  Every bound is per output element and derived here; there is no blanket tolerance.

  Decode GEMM, out = act(x W^T + c2) + resid (ln = 0).  A wave keeps two accumulator chains of v_mfma_f32_16x16x4f32 per tile; every
  MFMA is counted as four sequential fused multiply-adds (the hardware's internal order is not documented: the worst case), so a chain
  accumulates 8 * steps k-values (steps = K / S / NW / 16 k16-steps per wave).  The two chains are then added (1), the NW waves'
  partial tiles summed in LDS (NW), the S slices of a split summed in slice order (S) and c2 added (1):
      n = 8 * steps + 1 + NW + S + 1,   |err| <= gamma(n) * (|x| |W|^T + |c2|)                                          [GEMM]
  (`dgemm_depth`).  GELU (0.5 r (1 + erff(r / sqrt 2))) multiplies an input error by at most max gelu' = 1.1289 and adds erff's 2 ulp
  (absolute: |erf| <= 1) times 0.5 |r| plus three roundings: <= 1.13 err + 6 u |r| + u.  The residual add rounds once: + u |out|.

  LayerNorm fold (ln = 1, weights from sfmi_ln_fold_pack_f32): out = (A - c1 mean) rstd + c2 with A = x W'^T, W' = f32(W diag(gamma)),
  c1 = sum_k W'_k and c2 = sum_k beta_k W_k + bias, each rounded once.  The row statistics are ONE pass (sum and sum of squares, f32):
      t1 = sum x: 2 levels per k16-step in a lane + steps, 2 shuffles, NW waves, S slices -> n1 = steps + 4 + NW + S;  t2: n1 + 1
      |d mean| <= gamma(n1 + 1) E|x|,   |d var| <= gamma(n1 + 3) (E[x^2] + mean^2) + 2 |mean| |d mean|
  With e = |d var| / (var + 1e-5), rsqrt(var + eps) is off by at most e / (2 (1 - e)^1.5) + 3 u relative (rsqrtf 1 ulp, the eps add,
  the division by K).  E[x^2] = var + mean^2: the variance term grows with (1 + mean^2 / var), so a row with a large mean loses digits
  in E[x^2] - mean^2 first.  The centring A - c1 mean cancels the same way; its error is
      gamma(n) |x| |W'|^T + |c1| |d mean| + 2 u |mean| |c1| + u |x - mean| |W'|^T   (the last: W' against the exact W gamma),
  times rstd (1 + its error); the result z = (x - mean) rstd (gamma W)^T carries the rstd error and two roundings (the subtraction
  and the product), c2 its own rounding and the add.

  Decode attention (one query per (row, head), t + 1 keys).  A score s_i = f32(q scale) . k_i: the scale 1/sqrtf(HD) (2 roundings),
  q times it (1), the products (1), two in-lane levels and a 16-lane DPP tree (4 levels) -> |d s_i| <= gamma(10) scale sum_d |q_d k_id|.
  p_i = __expf(s_i - max): the subtraction, __expf's scaling by log2 e and v_exp_f32 give a relative error <= 2 u |s_i - max| + 3 u;
  the common max cancels in the normalisation, so every p_i is off by at most eps_p = max_i (|d s_i| + 2 u |s_i - max|) + 3 u relative
  to a common factor.  y = sum p_i v_i / sum p_i: a lane accumulates ceil((t + 1) / (4 NWV)) keys (+ the product), then 2 shuffle
  levels and NWV waves: n_a = ceil((t + 1) / (4 NWV)) + NWV + 3, and
      |err| <= (exp(eps_p) - 1 + gamma(n_a)) (sum p |v| / sum p + |y|) + u |y|                                           [ATTN]
  (sum p |v| / sum p <= max |v|: the accumulation error over the t keys is scaled by the values' size).

  Prefill attention (MFMA, online softmax over 64-key blocks): scores through HD sequential fused multiply-adds (+ 3 for the scale),
  P V through one MFMA chain over the keys with one rescale per block (n_a = (t + 1) + 2 blocks + 8), and every block's rescale
  exp(m_old - m_new) adds 3 u + 2 u |s - max| to eps_p.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of f32
LN_EPS = 1e-5           # nn.LayerNorm default (mingpt.py:103-111)
GELU_SLOPE = 1.1289     # max_r d/dr [r Phi(r)] (at r = sqrt 2)


def gamma(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U / (1.0 - n * U)


def _t64(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    return a.detach().to("cpu", torch.float64)


# ---------------------------------------------------------------------------------------------------- fragment-packed layout
def pack(a, rows=None):
    """(R, C) -> flat fragment-packed [rows/16][C/16][64][4] (zero rows beyond R); C % 16 == 0 (the weight pack: C = K)."""
    a = torch.as_tensor(a)
    R, C = a.shape
    assert C % 16 == 0, C
    rows = (R + 15) // 16 * 16 if rows is None else rows
    assert rows % 16 == 0 and rows >= R
    if rows != R:
        a = torch.cat([a, a.new_zeros(rows - R, C)], 0)
    return a.reshape(rows // 16, 16, C // 16, 4, 4).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def unpack(p, R, C):
    """Inverse of pack: a flat fragment-packed buffer (at least ceil(R/16)*16*C elements) -> (R, C)."""
    p = torch.as_tensor(p)
    rows = (R + 15) // 16 * 16
    a = p[:rows * C].reshape(rows // 16, C // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(rows, C)
    return a[:R]


def unpack_weight(wp, N, K):
    """Wp16 = sfmi_skinny16_pack_weight(W (N, K)) -> W."""
    return unpack(wp, N, K)


def pk_off(m, n, N):
    """gpt.hip pk_off, vectorised over integer arrays."""
    m, n = np.asarray(m, np.int64), np.asarray(n, np.int64)
    return ((((m >> 4) * (N >> 4) + (n >> 4)) * 64 + ((n >> 2) & 3) * 16 + (m & 15)) << 2) + (n & 3)


# ---------------------------------------------------------------------------------------------------- decode GEMM
DGEMM_DEFAULT_KNOBS = {"dgemm_nw": 0, "dgemm_un": 0, "dgemm_nt2": 1}

# every dgemm_kernel<MT, NW, UN, NT> that decode_gemm_launch instantiates (its DG2 / DG / DGU8 / DGU4 / DGU2 macros), as (NT, MT, NW, UN)
DGEMM_INSTANCES = sorted(
    [(2, mt, 8, 2) for mt in (2, 3)]
    + [(1, 1, 16, u) for u in (8, 4, 2, 1)] + [(1, 2, 16, u) for u in (4, 2, 1)] + [(1, mt, 16, u) for mt in (3, 4) for u in (2, 1)]
    + [(1, 1, 4, 1), (1, 2, 4, 1)] + [(1, mt, 4, u) for mt in (3, 4) for u in (2, 1)]
    + [(1, 1, 1, 1)]
    + [(1, 1, 8, u) for u in (8, 4, 2, 1)] + [(1, 2, 8, u) for u in (4, 2, 1)] + [(1, mt, 8, u) for mt in (3, 4, 5) for u in (2, 1)]
    + [(1, 6, 8, 1)])

_MT_CAP = {16: 4, 8: 6, 4: 4, 1: 1}                           # row tiles per workgroup an NW has instances for
_UN_CAP = {16: {1: 8, 2: 4, 3: 2, 4: 2}, 8: {1: 8, 2: 4, 3: 2, 4: 2, 5: 2, 6: 1}, 4: {1: 1, 2: 1, 3: 2, 4: 2}, 1: {1: 1}}


def dgemm_form(M, K, S, knobs=None):
    """(NT, MT, NW, UN, groups) of the dgemm_kernel instance that decode_gemm_launch (csrc/gpt.hip) picks for an M-row launch of a
    K-deep GEMM split S ways under the tuning knobs `knobs` (defaults: DGEMM_DEFAULT_KNOBS).  Used only to prove which instances a
    test reaches.  It MIRRORS decode_gemm_launch and has to change with it.  Raises ValueError where the launcher returns SFMI_EINVAL."""
    kn = dict(DGEMM_DEFAULT_KNOBS, **(knobs or {}))
    if not (0 < M <= 192) or S <= 0 or K % S:
        raise ValueError("EINVAL")
    kslice = K // S
    tiles = (M + 15) // 16
    groups = (tiles + 5) // 6
    MT = -(-tiles // groups)
    NW = 16 if (kslice >= 2048 and MT <= 4) else 8
    knw = kn["dgemm_nw"]
    if knw in (4, 8, 16) and kslice % (16 * knw) == 0 and MT <= (6 if knw == 8 else 4):
        NW = knw
    if kslice % (16 * NW):
        NW = 4 if kslice % 64 == 0 else 1
    if kslice % (16 * NW):
        raise ValueError("EINVAL")
    if MT > _MT_CAP[NW]:
        groups = -(-tiles // _MT_CAP[NW])
        MT = -(-tiles // groups)
    nt2 = kn["dgemm_nt2"]
    if (nt2 == 2 or (nt2 == 1 and tiles % 3 == 0)) and NW == 8 and (kslice // 8 // 16) % 2 == 0 and tiles >= 3:
        g2 = (tiles + 2) // 3
        return (2, -(-tiles // g2), 8, 2, g2)
    steps = kslice // NW // 16
    un = 8 if MT == 1 else 4 if MT == 2 else 2 if MT <= 5 else 1
    if 0 < kn["dgemm_un"] < un:
        un = 1 << (kn["dgemm_un"].bit_length() - 1)
    while un > 1 and steps % un:
        un >>= 1
    return (1, MT, NW, min(un, _UN_CAP[NW][MT]), groups)


def dgemm_depth(K, S, NW):
    """n of the [GEMM] bound: the roundings a product passes on its way to the output (module docstring)."""
    steps = K // S // NW // 16
    return 8 * steps + 1 + NW + S + 1


def dgemm_stats_depth(K, S, NW):
    """n1 of the LayerNorm statistics (module docstring)."""
    steps = K // S // NW // 16
    return steps + 4 + NW + S


def _gelu(h):
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))


def ln_linear_ref(x, W, gamma_=None, beta=None, bias=None, act=0, resid=None):
    """mingpt.py:103-111 in float64: [LayerNorm (eps 1e-5, biased variance)] -> x W^T + bias -> [GELU (erf)] -> [+ resid].
    gamma_ None: no LayerNorm."""
    x, W = _t64(x), _t64(W)
    if gamma_ is not None:
        mean = x.mean(1, keepdim=True)
        var = ((x - mean) ** 2).mean(1, keepdim=True)
        x = (x - mean) / torch.sqrt(var + LN_EPS) * _t64(gamma_) + (_t64(beta) if beta is not None else 0.0)
    h = x @ W.T
    if bias is not None:
        h = h + _t64(bias)
    if act:
        h = _gelu(h)
    if resid is not None:
        h = h + _t64(resid)
    return h


def dgemm_plain_bound(x, W, c2, act, resid, n):
    """[GEMM] bound of out = act(x W^T + c2) + resid (ln = 0; c2 / resid may be None) for summation depth n."""
    x, W = _t64(x), _t64(W)
    P = x.abs() @ W.abs().T
    pre = x @ W.T
    if c2 is not None:
        c2 = _t64(c2)[:W.shape[0]]
        P, pre = P + c2.abs(), pre + c2
    return _epilogue_bound(gamma(n) * P, pre, act, resid)


def dgemm_ln_bound(x, W, gamma_, beta, bias, c1, act, resid, n, n1):
    """Bound of the LayerNorm-fold form against ln_linear_ref(x, W, gamma_, beta, bias, act, resid): c1 the folded row sums the kernel
    read (sfmi_ln_fold_pack_f32), n / n1 the summation depths of the GEMM and of the row statistics (module docstring)."""
    x, W, g = _t64(x), _t64(W), _t64(gamma_)
    K = x.shape[1]
    Wp = _t64(W.to(torch.float32) * g.to(torch.float32))            # the f32 products the fold stores
    c1 = _t64(c1)[:W.shape[0]]
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    ex2 = (x * x).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    d_mean = gamma(n1 + 1) * x.abs().mean(1, keepdim=True)
    d_var = gamma(n1 + 3) * (ex2 + mean * mean) + 2.0 * mean.abs() * d_mean
    e = d_var / (var + LN_EPS)
    assert float(e.max()) < 0.5, "the rstd linearisation needs |d var| < (var + eps) / 2"
    e_rstd = e / (2.0 * (1.0 - e) ** 1.5) + 3 * U
    z = ((x - mean) * rstd) @ (W * g).T                               # the LayerNorm'd linear without beta / bias
    centred = (gamma(n) * (x.abs() @ Wp.abs().T) + c1.abs() * d_mean + 2 * U * mean.abs() * c1.abs()
               + U * ((x - mean).abs() @ Wp.abs().T))
    err = centred * rstd * (1.0 + e_rstd) + z.abs() * (e_rstd + 2 * U)
    c2 = W @ (_t64(beta) if beta is not None else torch.zeros(K, dtype=torch.float64))
    if bias is not None:
        c2 = c2 + _t64(bias)
    pre = z + c2
    err = err + U * c2.abs() + U * pre.abs()
    return _epilogue_bound(err, pre, act, resid)


def _epilogue_bound(err, pre, act, resid):
    val = pre
    if act:
        err = GELU_SLOPE * err + 6 * U * pre.abs() + U
        val = _gelu(pre)
    if resid is not None:
        err = err + U * (val + _t64(resid)).abs()
    return err


# ---------------------------------------------------------------------------------------------------- attention
def decode_attn_ref(q, k_new, v_new, Kc, Vc, lens, shared_len=0, nwv=16):
    """One decode step (mingpt.py:73-91, one new query per row) in float64.
    q, k_new, v_new (B, H, HD): the step's projections; Kc / Vc (B, H, >= max len, HD): the caches as the kernel finds them (position
    len[b]-1 is the step's own and is taken from k_new / v_new); lens (B,) = len.  shared_len > 0: positions < shared_len of every
    row come from row 0's cache (csrc/gpt.hip attn_decode_item, SH).  Returns y (B, H, HD) and the [ATTN] bound for NWV waves."""
    q, k_new, v_new, Kc, Vc = (_t64(a) for a in (q, k_new, v_new, Kc, Vc))
    B, H, HD = q.shape
    scale = 1.0 / math.sqrt(HD)
    y = torch.empty(B, H, HD, dtype=torch.float64)
    bound = torch.empty(B, H, HD, dtype=torch.float64)
    for b in range(B):
        t = int(lens[b]) - 1
        K = Kc[b, :, :t + 1].clone()
        V = Vc[b, :, :t + 1].clone()
        ns = min(int(shared_len), t)
        if ns > 0:
            K[:, :ns], V[:, :ns] = Kc[0, :, :ns], Vc[0, :, :ns]
        K[:, t], V[:, t] = k_new[b], v_new[b]
        qs = q[b] * scale
        s = torch.einsum("hd,htd->ht", qs, K)
        smax = s.max(1, keepdim=True).values
        p = torch.exp(s - smax)
        l = p.sum(1, keepdim=True)
        yb = torch.einsum("ht,htd->hd", p, V) / l
        y[b] = yb
        ds = gamma(10) * torch.einsum("hd,htd->ht", qs.abs(), K.abs())
        eps_p = (ds + 2 * U * (s - smax).abs()).max(1, keepdim=True).values + 3 * U
        na = -(-(t + 1) // (4 * nwv)) + nwv + 3
        pv = torch.einsum("ht,htd->hd", p, V.abs()) / l
        bound[b] = (torch.expm1(eps_p) + gamma(na)) * (pv + yb.abs()) + U * yb.abs()
    return y, bound


def causal_attn_ref(q, k, v, nval):
    """Causal self-attention over a prefix (mingpt.py:73-91) in float64: q / k / v (B, H, P, HD), rows t < nval[b] valid.  Returns
    y (B, H, P, HD) (rows >= nval zero) and the prefill form of the [ATTN] bound."""
    q, k, v = _t64(q), _t64(k), _t64(v)
    B, H, P, HD = q.shape
    scale = 1.0 / math.sqrt(HD)
    y = torch.zeros(B, H, P, HD, dtype=torch.float64)
    bound = torch.zeros(B, H, P, HD, dtype=torch.float64)
    for b in range(B):
        n = int(nval[b])
        if n <= 0:
            continue
        qs = q[b, :, :n] * scale
        s = qs @ k[b, :, :n].transpose(1, 2)
        mask = torch.ones(n, n, dtype=torch.bool).tril()
        s = s.masked_fill(~mask, -math.inf)
        smax = s.max(2, keepdim=True).values
        p = torch.exp(s - smax)
        l = p.sum(2, keepdim=True)
        yb = p @ v[b, :, :n] / l
        y[b, :, :n] = yb
        tq = torch.arange(n, dtype=torch.float64).view(1, n, 1)
        blocks = torch.div(tq, 64, rounding_mode="floor") + 1
        ds = gamma(HD + 3) * (qs.abs() @ k[b, :, :n].abs().transpose(1, 2))
        spread = (s - smax).abs().masked_fill(~mask, 0)
        eps_p = ((ds + 2 * U * spread).masked_fill(~mask, 0).max(2, keepdim=True).values + 3 * U
                 + blocks * (3 * U + 2 * U * spread.max(2, keepdim=True).values))
        na = (tq + 1) + 2 * blocks + 8
        pv = p @ v[b, :, :n].abs() / l
        bound[b, :, :n] = (torch.expm1(eps_p) + gamma(na)) * (pv + yb.abs()) + U * yb.abs()
    return y, bound
