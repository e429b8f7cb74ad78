"""Float64 references of the implicit-GEMM convolution family of csrc/conv3d.hip and the per-element error bounds its tests assert.

Kernels: conv3d_igemm_kernel<CO_TILES, WM, WN, UPS, XR, J, ST> in the fourteen instances conv_dispatch launches (entries
sfmi_conv3d_cl[_stats]_f32, sfmi_conv3d_up2_cl[_stats]_f32, sfmi_gemm_f32), chan_stats_kernel and gn_coeffs_kernel
(sfmi_groupnorm_coeffs[_partial]_f32).  The references restate the model (updown.py:79-132, unet3d.py:79-144: GroupNorm apply ->
[nearest x2] -> zero padding -> Conv3d -> bias -> activation) in float64 on the f32 inputs the kernels see, tap by tap over a padded
copy of the input; nothing here reuses the kernels' tiling, chunking or summation order.  Every function keeps the device of its
inputs (float64 matmuls are exact enough on either), so the GPU tests can afford full-tensor references.

Layouts: x (B, D, H, W, Cin) channels last with separate extents, w (Cout, Cin, k, k, k) as torch stores it, scale / shift (B, Cin),
y (B, Do, Ho, Wo, Cout), Do = ((D << up) + 2 pad - k) / stride + 1.

Error bounds
  u = 2^-24 (f32, round to nearest), gamma(n) = n u / (1 - n u) (decode_ref.py; Higham, Accuracy and Stability of Numerical
  Algorithms, 2nd ed., 3.1-3.3): a sum in which every term passes through at most n roundings is off by at most gamma(n) sum |term|.
  Every bound is per output element and derived here; there is no blanket tolerance.

  Input affine.  The kernel forms xa = x * scale + shift in f32, fused or not (the compiler decides): at most two roundings,
      |d xa| <= e_aff = (2 u |x scale| + u |shift|) (1 + u).
  Padding voxels are exact zeros (a select, applied after the affine).  Through the convolution this is  E = |w| conv e_aff.        [AFF]

  Accumulation.  With A = |w| conv (|xa| + e_aff), the products of one output element are summed along one chain of
  v_mfma_f32_32x32x2f32; the hardware's internal order is not documented, so every MFMA counts as two sequential fused
  multiply-adds (a product is not rounded, each add is).  The chain depth n (`chain_depth`) is
      un-blocked forms     n = taps * Cin                     (27 Cin, 8 Cin for a sub-pixel parity and k2, Cin for k1 / the GEMM)
      ACC2 (128 x 64 x-reuse tile)   the running tile is folded into a second accumulator every FOLD = 8 chunks of KS * 16 products
                           (384 for k3): n = min(8 KS 16, K) + ceil(chunks / 8): one block's chain, then one add per fold - the last,
                           partial block is folded too and counts as one of them.
  The bias add is one more rounding of everything:      |err| <= gamma(n + 1) (A + |bias|) + E                                    [ACC]

  Sub-pixel form (sfmi_conv3d_up2_cl_f32) against the reference with the ORIGINAL 3^3 weights: sfmi_conv_pack_weight_subpixel sums up
  to eight f32 weights in f32, one after the other: |d w'| <= gamma(7) sum |w_t|.  Summed over the merged taps, sum |w_t| |xa| is
  exactly the A of the direct form, so the term is  gamma(7) A,  and the chain sees |w'| <= (1 + gamma(7)) sum |w_t|.             [SUB]

  Epilogue: ReLU is exact and 1-Lipschitz; GELU and the residual add as decode_ref._epilogue_bound (imported, not copied).

  Statistics epilogue (ST instances).  Per (tile, channel) a lane adds its J values (J roundings at most), 4 DPP levels and one
  shuffle make the half-wave's sum, the rest is f64.  The squares enter through fmaf(v, v, q): the product is not rounded.
      |d sum| <= gamma(J + 5) sum |y|,   |d sumsq| <= gamma(J + 5) sum y^2   (+ 8 * 2^-53 of the same for the f64 adds)           [ST]
  over the at most 512 values of a tile, against float64 sums of the y the same launch wrote.

  GroupNorm coefficients (chan_stats_kernel + gn_coeffs_kernel).  Sums and sums of squares are f64 throughout: with u64 = 2^-53 and
  n64 = ceil(V / S) + 256 + cpg S + 8 the depth of the longest f64 chain,
      |d mean| <= gamma64(n64) E|x|,  |d var| <= gamma64(n64 + 3) (E[x^2] + mean^2) + 2 |mean| |d mean|
  (the one-pass form E[x^2] - mean^2 loses (1 + mean^2 / var) digits: the large-mean case), e = |d var| / (var + eps),
  rstd = (float)(1 / sqrt(var + eps)) off by e / (2 (1 - e)^1.5) + 2 u64 + u relative, scale = gamma * rstd one more u:
      |d scale| <= |scale| (e_rstd + 2 u),   |d shift| <= |mean scale| (e_rstd + 4 u) + |scale| |d mean| + u |shift|                [GN]
  ((float) mean, the product and the subtraction round once each).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from decode_ref import U, gamma, _epilogue_bound, _gelu

U64 = 2.0 ** -53
FOLD = 8                   # conv3d.hip ACC2: chunks per fold block
KC = 16                    # input channels per chunk
SUBPIXEL_TERMS = 8         # weights sfmi_conv_pack_weight_subpixel sums at most


def t64(a):
    """float64 copy on the SAME device."""
    return torch.as_tensor(a).detach().to(torch.float64)


def gamma64(n):
    n = torch.as_tensor(n, dtype=torch.float64)
    return n * U64 / (1.0 - n * U64)


# ---------------------------------------------------------------------------------------------------- launcher mirror
# every conv3d_igemm_kernel<CO_TILES, WM, WN, UPS, XR, J, ST> that conv_dispatch instantiates (bools as 0 / 1)
CONV_INSTANCES = sorted([
    (2, 1, 4, 0, 1, 2, 1), (1, 1, 4, 0, 1, 4, 1),                                  # statistics epilogue: 64 / 32 channels
    (1, 2, 2, 0, 1, 2, 0), (1, 2, 2, 0, 0, 2, 0),                                  # 128 x 64 tile: ACC2 x reuse, per tap
    (2, 2, 2, 0, 1, 2, 0), (2, 2, 2, 1, 0, 2, 0), (2, 2, 2, 0, 0, 2, 0),           # 128 x 128 tile: x reuse, up-sampling, per tap
    (2, 1, 4, 0, 1, 2, 0), (2, 1, 4, 1, 0, 2, 0), (2, 1, 4, 0, 0, 2, 0),           # 64 channels x 256 voxels
    (1, 1, 4, 0, 1, 4, 0), (1, 1, 4, 0, 1, 2, 0), (1, 1, 4, 1, 0, 2, 0), (1, 1, 4, 0, 0, 2, 0),   # 32 channels x 512 / 256 voxels
])
ACC2_INSTANCE = (1, 2, 2, 0, 1, 2, 0)


class ConvForm:
    """What conv_form returns: instance (CO_TILES, WM, WN, UPS, XR, J, ST), tile sizes M_T (voxels) x N_T (channels), blocks (grid size),
    straddle (some tile holds voxels of two shapes), partial (the last voxel tile is partly empty), output extents, K, chain depth n."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "ConvForm(%s)" % ", ".join(f"{k}={v}" for k, v in self.__dict__.items())


def out_extent(d, ks, stride, pad, up):
    return ((d << up) + 2 * pad - ks) // stride + 1


def chain_depth(instance, Cin, KS):
    """n of the [ACC] bound without the bias add (module docstring)."""
    K = KS ** 3 * Cin
    if tuple(instance) == ACC2_INSTANCE:
        chunks = KS * KS * (Cin // KC)
        return min(FOLD * KS * KC, K) + -(-chunks // FOLD)
    return K


def conv_form(B, Di, Hi, Wi, Cin, Cout, KS, stride=1, pad=0, up=0, knob=2, stats=False, subpixel=False, has_scale=False, has_shift=None,
              resid=False, out_group=0):
    """The instance conv_dispatch (csrc/conv3d.hip) launches for these arguments under conv_xreuse = knob, assuming the device grants
    the raised dynamic-LDS limits (gfx950 does).  subpixel: ONE parity launch of sfmi_conv3d_up2_cl[_stats]_f32 on the low-resolution
    grid (KS, stride, pad, up are then 2, 1, 0, 0).  stats: the *_stats entry with a partial buffer.  It MIRRORS conv_stats_tile,
    conv_dispatch and the argument checks of the entries and has to change with them.  Raises ValueError where the entry returns
    SFMI_EINVAL."""
    if subpixel:
        KS, stride, pad, up = 2, 1, 0, 0
    has_shift = has_scale if has_shift is None else has_shift
    lim = 1 << 20
    if (B < 1 or Cin < KC or Cin % KC or Cout < 32 or Cout % 32 or KS not in (1, 2, 3) or bool(has_scale) != bool(has_shift) or stride < 1
            or pad < 0 or pad > lim or up not in (0, 1) or min(Di, Hi, Wi) < 1 or max(Di, Hi, Wi) > lim or knob not in (0, 1, 2, 3)):
        raise ValueError("EINVAL")
    if not subpixel and min((Di << up) + 2 * pad, (Hi << up) + 2 * pad, (Wi << up) + 2 * pad) < KS:      # an output extent < 1
        raise ValueError("EINVAL")
    Do, Ho, Wo = (Di, Hi, Wi) if subpixel else tuple(out_extent(d, KS, stride, pad, up) for d in (Di, Hi, Wi))
    vs = Do * Ho * Wo
    M = B * vs
    xr_geom = bool(knob) and stride == 1 and not up and KS in (2, 3) and (Do, Ho, Wo) == (Di, Hi, Wi) and (subpixel or 2 * pad == KS - 1)

    def lds(M_T, N_T, x):
        arows = (M_T // Wo) * (Wo + KS - 1) if x else M_T
        if x and (N_T == 128 or M_T == 512):
            return (2 * ((arows + 15) & ~15) + 2 * 3 * N_T) * 16 * 4
        return (2 * arows + 2 * (3 if x else 1) * N_T) * 20 * 4

    def stats_tile():
        if not (xr_geom and 256 % Wo == 0) or resid or out_group:
            return 0
        if Cout == 64 and vs % 256 == 0 and lds(256, 64, True) <= 96 * 1024:
            return 256
        if Cout == 32 and knob >= 2 and 512 % Wo == 0 and vs % 512 == 0 and M // 512 >= 1024 and lds(512, 32, True) <= 80 * 1024:
            return 512
        return 0

    xr = xr_geom and 256 % Wo == 0 and Cout % 128 != 0
    if stats:
        M_T = stats_tile()
        if not M_T:
            raise ValueError("EINVAL")
        inst, N_T = ((2, 1, 4, 0, 1, 2, 1), 64) if M_T == 256 else ((1, 1, 4, 0, 1, 4, 1), 32)
    elif Cout % 128 == 0:
        M_T = 128
        tiles = -(-M // 128) * (Cout // 128)
        xr128 = xr_geom and knob >= 2 and 128 % Wo == 0
        if (tiles < 512 or (xr128 and knob == 2)) and not up and knob >= 2:
            N_T = 64
            inst = (1, 2, 2, 0, 1, 2, 0) if xr128 and lds(128, 64, True) <= 80 * 1024 else (1, 2, 2, 0, 0, 2, 0)
        else:
            N_T = 128
            inst = ((2, 2, 2, 0, 1, 2, 0) if xr128 and lds(128, 128, True) <= 80 * 1024 else (2, 2, 2, 1, 0, 2, 0) if up else (2, 2, 2, 0, 0, 2, 0))
    elif Cout % 64 == 0:
        M_T, N_T = 256, 64
        inst = (2, 1, 4, 0, 1, 2, 0) if xr and lds(256, 64, True) <= 96 * 1024 else (2, 1, 4, 1, 0, 2, 0) if up else (2, 1, 4, 0, 0, 2, 0)
    else:
        M_T, N_T = 256, 32
        if (xr and knob >= 2 and 512 % Wo == 0 and lds(512, 32, True) <= 80 * 1024 and vs % 512 == 0 and (M // 512) * (Cout // 32) >= 1024):
            M_T, inst = 512, (1, 1, 4, 0, 1, 4, 0)
        else:
            inst = (1, 1, 4, 0, 1, 2, 0) if xr and lds(256, 32, True) <= 96 * 1024 else (1, 1, 4, 1, 0, 2, 0) if up else (1, 1, 4, 0, 0, 2, 0)
    vt = -(-M // M_T)
    return ConvForm(instance=inst, M_T=M_T, N_T=N_T, voxel_tiles=vt, blocks=vt * (Cout // N_T), straddle=B > 1 and vs % M_T != 0,
                    partial=M % M_T != 0, Do=Do, Ho=Ho, Wo=Wo, K=KS ** 3 * Cin, n=chain_depth(inst, Cin, KS))


def gemm_form(M, N, K, knob=2, out_group=0, out_group_stride=0):
    """sfmi_gemm_f32's launch: a 1 x 1 x 1 convolution over a (1, 1, 1, M) grid.  ValueError where it returns SFMI_EINVAL."""
    if M < 1 or M > 0x7FFFFFFF or out_group < 0 or (out_group > 0 and out_group_stride < out_group) or K < KC or K % KC or N < 32 or N % 32:
        raise ValueError("EINVAL")
    f = conv_form(1, 1, 1, min(M, 1 << 20), K, N, 1, knob=knob)        # (the entry does not limit M to the grid-extent range)
    if M > 1 << 20:
        vt = -(-M // f.M_T)
        f.voxel_tiles, f.blocks, f.partial, f.Wo = vt, vt * (N // f.N_T), M % f.M_T != 0, M
    return f


def gn_splits(V):
    return 64 if V >= 32768 else 16 if V >= 4096 else 4 if V >= 512 else 1


# ---------------------------------------------------------------------------------------------------- convolution
def affine_pad(x, scale, shift, pad, up, pad_first=False):
    """(xa, e_aff) zero-padded by `pad` voxels per side, both (B, Dp, Hp, Wp, C) float64: the affine'd [and nearest-x2 up-sampled] input
    and the [AFF] bound of its f32 evaluation.  pad_first (a MUTANT for the teeth tests): padding applied before the affine."""
    x = t64(x)
    B, C = x.shape[0], x.shape[-1]
    if scale is not None:
        sc, sh = t64(scale).view(B, 1, 1, 1, C), t64(shift).view(B, 1, 1, 1, C)
    p6 = (0, 0, pad, pad, pad, pad, pad, pad)

    def up2(a):
        for d in (1, 2, 3):
            a = a.repeat_interleave(2, dim=d) if up else a
        return a
    if scale is None:
        return F.pad(up2(x), p6), F.pad(torch.zeros_like(up2(x)), p6)
    e = (2 * U * (x * sc).abs() + U * sh.abs().expand_as(x)) * (1 + U)
    if pad_first:
        return F.pad(up2(x), p6) * sc + sh, F.pad(up2(e), p6)
    return F.pad(up2(x * sc + sh), p6), F.pad(up2(e), p6)


def correlate(xp, w, ks, stride, osz, hook=None):
    """sum over the ks^3 taps of (strided window of the padded input) @ w[:, :, tap]^T.  hook(dz, dy, dx, window, wt) -> (window, wt)
    lets a teeth test mutate single taps."""
    Do, Ho, Wo = osz
    out = xp.new_zeros(xp.shape[0], Do, Ho, Wo, w.shape[0])
    for dz in range(ks):
        for dy in range(ks):
            for dx in range(ks):
                sl = xp[:, dz:dz + stride * (Do - 1) + 1:stride, dy:dy + stride * (Ho - 1) + 1:stride, dx:dx + stride * (Wo - 1) + 1:stride]
                wt = w[:, :, dz, dy, dx]
                if hook is not None:
                    sl, wt = hook(dz, dy, dx, sl, wt)
                out += sl @ wt.T
    return out


def _act(pre, act):
    return pre if act == 0 else torch.relu(pre) if act == 1 else _gelu(pre)


def conv_ref(x, w, scale, shift, bias, ks, stride, pad, up, act, parts=False, hook=None, pad_first=False):
    """act(conv3d(zero_pad(nearest_x2^up(x * scale + shift)), w, stride) + bias) in float64; act 0 none / 1 ReLU / 2 erf-GELU.
    parts: also pre (before the activation), A = |w| conv (|xa| + e_aff) and E = |w| conv e_aff, as a dict."""
    w = t64(w)
    xp, ep = affine_pad(x, scale, shift, pad, up, pad_first)
    osz = tuple(out_extent(d, ks, stride, pad, up) for d in x.shape[1:4])
    pre = correlate(xp, w, ks, stride, osz, hook)
    if bias is not None:
        pre = pre + t64(bias)
    y = _act(pre, act)
    if not parts:
        return y
    return dict(y=y, pre=pre, A=correlate(xp.abs() + ep, w.abs(), ks, stride, osz), E=correlate(ep, w.abs(), ks, stride, osz))


def conv_bound(p, n, bias, act, subpixel=False):
    """[ACC] + [AFF] (+ [SUB]) + epilogue for the parts dict p of conv_ref and chain depth n."""
    A = p["A"]
    if subpixel:
        A = A * (1.0 + gamma(SUBPIXEL_TERMS - 1))
    err = gamma(n + 1) * (A + (t64(bias).abs() if bias is not None else 0.0)) + p["E"]
    if subpixel:
        err = err + gamma(SUBPIXEL_TERMS - 1) * p["A"]
    return _epilogue_bound(err, p["pre"], act == 2, None)


def pack_weight(w):
    """sfmi_conv_pack_weight: (Cout, Cin, k, k, k) -> [tap][Cout][Cin] (f32, contiguous)."""
    Cout, Cin = w.shape[:2]
    return w.reshape(Cout, Cin, -1).permute(2, 0, 1).contiguous()


def boundary_mask(Do, Ho, Wo, device=None):
    """(Do, Ho, Wo) bool: the outermost voxel layer (where a window reaches the padding)."""
    m = torch.zeros(Do, Ho, Wo, dtype=torch.bool, device=device)
    m[0], m[-1], m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True, True, True
    return m


# ---------------------------------------------------------------------------------------------------- GEMM
def remap_rows(M, out_group, out_group_stride, device=None):
    m = torch.arange(M, device=device)
    return m if not out_group else (m // out_group) * out_group_stride + m % out_group


def gemm_ref(x, W, bias, act, resid, out_group=0, out_group_stride=0, resid_unmapped=False):
    """y[remap(m)] = act(x W^T + bias) + resid[remap(m)] in float64.  Returns (rows = remap(0 .. M-1), y (M, N) in input row order,
    pre, P = |x| |W|^T + |bias|, r = the residual rows read), all on the CPU.  resid is the WHOLE remapped buffer (rows_out, N).  resid_unmapped (a MUTANT): resid read at row m."""
    x, W = t64(x).cpu(), t64(W).cpu()           # on the CPU: decode_ref._epilogue_bound works there, and a GEMM is small
    bias, resid = (None if a is None else t64(a).cpu() for a in (bias, resid))
    M = x.shape[0]
    rows = remap_rows(M, out_group, out_group_stride, x.device)
    pre, P = x @ W.T, x.abs() @ W.abs().T
    if bias is not None:
        pre, P = pre + t64(bias), P + t64(bias).abs()
    y = _act(pre, act)
    r = None
    if resid is not None:
        r = t64(resid)[torch.arange(M, device=x.device) if resid_unmapped else rows]
        y = y + r
    return rows, y, pre, P, r


def gemm_bound(pre, P, K, has_bias, act, r):
    """[ACC] with n = K (+ 1 for the bias add) and the epilogue of decode_ref."""
    err = gamma(K + 1) * P
    if act == 1:
        return _epilogue_bound(err, torch.relu(pre), 0, r)
    return _epilogue_bound(err, pre, act == 2, r)


# ---------------------------------------------------------------------------------------------------- statistics / GroupNorm
def tile_sums_ref(y, M_T, subpixel=False):
    """Per (shape, split, channel) float64 {sum, sum of squares, sum |.|} of y (B, Do, Ho, Wo, C) in the layout the ST instances write:
    split = tile of M_T consecutive voxels of a shape; subpixel: split = parity (4 pz + 2 py + px) * tiles + tile of the LOW-resolution
    lattice, whose voxel (z, y, x) stands for output voxel (2z + pz, 2y + py, 2x + px).  Returns (B, S, C, 3)."""
    y = t64(y)
    B, Do, Ho, Wo, C = y.shape
    if subpixel:
        y = y.view(B, Do // 2, 2, Ho // 2, 2, Wo // 2, 2, C).permute(0, 2, 4, 6, 1, 3, 5, 7)
    y = y.reshape(B, -1, M_T, C)
    return torch.stack([y.sum(2), (y * y).sum(2), y.abs().sum(2)], -1)


def tile_sums_bound(ref, J):
    """[ST]: (B, S, C, 2) bounds of {sum, sum of squares} for the (B, S, C, 3) reference of tile_sums_ref."""
    g = gamma(J + 5) + 8 * U64
    return torch.stack([g * ref[..., 2], g * ref[..., 1]], -1)


def groupnorm_coeffs_ref(x, gamma_, beta, groups, eps=1e-5, S=None):
    """nn.GroupNorm(groups, C, eps) of x (B, V, C) as per-(shape, channel) scale / shift with GN(x) == x * scale + shift, float64, and
    the [GN] bounds of the f32 coefficients.  Returns (scale, shift, d_scale, d_shift), each (B, C).  S: statistics splits (default:
    sfmi_gn_splits(V))."""
    x, g, b = t64(x), t64(gamma_), t64(beta)
    B, V, C = x.shape
    cpg = C // groups
    S = gn_splits(V) if S is None else S
    xg = x.view(B, V, groups, cpg)
    mean = xg.mean((1, 3))
    var = ((xg - mean.view(B, 1, groups, 1)) ** 2).mean((1, 3))
    ex2, eabs = (xg * xg).mean((1, 3)), xg.abs().mean((1, 3))
    n64 = -(-V // S) + 256 + cpg * S + 8
    d_mean = gamma64(n64) * eabs
    d_var = gamma64(n64 + 3) * (ex2 + mean * mean) + 2.0 * mean.abs() * d_mean
    e = d_var / (var + eps)
    assert float(e.max()) < 0.5, "the rstd linearisation needs |d var| < (var + eps) / 2"
    e_rstd = e / (2.0 * (1.0 - e) ** 1.5) + 2 * U64 + U
    rstd = 1.0 / torch.sqrt(var + eps)
    rep = lambda t: t.repeat_interleave(cpg, dim=1)          # (B, groups) -> (B, C)
    scale = g * rep(rstd)
    shift = b - rep(mean) * scale
    d_scale = scale.abs() * (rep(e_rstd) + 2 * U)
    d_shift = (rep(mean) * scale).abs() * (rep(e_rstd) + 4 * U) + scale.abs() * rep(d_mean) + U * shift.abs()
    return scale, shift, d_scale, d_shift


def chan_sums_ref(x):
    """float64 per-(shape, channel) sum and sum of squares of x (B, V, C): (B, C, 2)."""
    x = t64(x)
    return torch.stack([x.sum(1), (x * x).sum(1)], -1)


def rel_rms(y, y64, mask=None):
    d, r = t64(y) - y64, y64
    if mask is not None:
        d, r = d[mask], r[mask]
    return math.sqrt(float((d * d).mean()) / float((r * r).mean()))
