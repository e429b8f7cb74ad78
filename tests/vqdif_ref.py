"""Float64 references of the VQDIF point path - csrc/encoder.hip (enc_* kernels), csrc/vq_argmin.hip and the value forms of
csrc/sdf_query.hip - and the per-element error bounds their tests assert.

The references are the oracle's own pieces (oracle/vqdif_oracle.py: resblock, local_max_pool, grid_mean; its occupancy_mask and the
decoder of tests/sdf_grad_ref.py are what test_vqdif_ref_cpu.py checks the mirrors and the decoder written out here against) run in float64 on the f32 inputs the
kernels see.  The DISCRETE decisions - which cell a point falls in, which feature cell a query reads and with which weights - are
taken in float32 by numpy mirrors of the kernels' IEEE operation sequence (cells_f32, axis_f32): those must match bit for bit, and
sharing them removes the coordinate rounding (4.5e-5 on a logit at G = 64) from the value comparison, which is then left with the
arithmetic under test (1e-6).

Error bounds
  u = 2^-24, gamma(n) = n u / (1 - n u) (decode_ref.py; Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., 3.1-3.3).
  Nothing is fitted to a kernel's error.

  Local rounding of one layer, fan-in K (one chain of v_mfma_f32_32x32x2f32, every MFMA counted as two sequential fused multiply-adds,
  the bias as one more term, one spare):          eps = gamma(K + 2) (|W| |x| + |b|)                                          [LIN]
  A layer that accumulates ONTO a running value r (ResnetBlockFC's shortcut + fc_1 in one chain: K = 64 + 32; the decoder's
  net += fc_c(c), net += fc_1(relu(h))) counts r as one more term of the chain: gamma(K + 3) (|r| + |W| |x| + |b|); the decoder's host
  packer adds two biases in f32 (bc_i + b1_{i-1}): one more rounding of |b|, gamma(K + 4).                                      [ACC]

  Propagation.  Carrying a bound through the layers as  e_out = |W| e_in + eps  (the textbook rule; ReLU and max 1-Lipschitz, a pool
  taking the largest bound of its cell) is valid but useless here: with the test weights |W| has row sums of 8, a ResnetBlockFC
  multiplies the bound by 8 + 5.7 x 8 = 54 and five of them turn the 5e-5 of the first block into 8e2 on a quantity of size 2 - every
  seeded fault of test_vqdif_ref_cpu.py passed it.  The bound is therefore taken through the network's ACTUAL linearisation: with
  D the 0 / 1 ReLU masks and the arg-max points of every pool at the float64 reference, a block is  o = J x,  J = Wsc + W1 D_h W0 D_x,
  a pool copies the arg-max point's channel, and an output's error is, to first order in u,
      |d out| <= sum over every rounding site s  |d out / d s| eps_s                                                           [JAC]
  with the sensitivities d out / d s the entries of the product of those Jacobians - signs cancel inside the product, only the
  sites' contributions are added in absolute value.  The pools couple the points of a cell, so for the encoder the product is formed
  per cell over its n x 32 state (encoder_ref's backward sweep); the decoder is point-wise and its sensitivities are one
  torch.autograd pass (mlp_ref).  Second-order terms (u^2, and a ReLU or an arg-max that the error itself flips: such a unit lies
  within its own error of the kink and contributes no more than that error again) are not modelled.
  Cell mean: every c is converted to 2^-32 fixed point (|error| <= 2^-33), the integer sum is exact, sum / n is formed in f64 and
  rounded to f32 once:            e_mean = mean(e_c) + 2^-33 + u |mean|                                                        [MEAN]
  down0 (k2 s2, 32 -> 64, at most 8 x 32 fmaf in one chain): e = |W| e_mean + [LIN] with K = 256 (one layer: nothing to compound).
  VQ distance (|x|^2 - 2 x.w) + |w|^2: |x|^2 through D / 8 + 6 roundings, x.w through the D MFMA products, |w|^2 through D + 1 (host,
  sequential), two more adds:     e_d = gamma(D + 3) (|x|^2 + 2 |x|.|w| + |w|^2)                                                [VQ]
  Trilinear gather: w = (wx wy) wz (2 roundings), 8 fmaf: gamma(10) sum w |v|; the in-kernel GroupNorm affine is one fmaf: + u |c s + t|.
  Coordinate slack: a compiler may legally round ix once differently from the mirror (contraction); the value is continuous in ix
  (also across a feature-cell face), so 2 ulp(ix) per axis times the local slope - per channel the largest difference between the
  eight corner features - enter as an error of c and reach the logit through its sensitivity to c like any other site.           [IX]
  Sigmoid: y = 1 / (1 + E), E = __expf(-r).  train_ref.py bounds __expf by E_EXP (1 + |x|) u relative (twice the largest error measured by
  tools/ubench/intrinsic_error.hip: the argument's scaling by log2 e grows with |x|, v_exp_f32 adds its unit in the last place); d y / d E
  = -y^2, so that error reaches y as y (1 - y) E_EXP (1 + |r|) u.  The add rounds once and the reciprocal is good to one unit in the last
  place, 2 u: 3 u y.  Where E overflows (r < -88) or is flushed as a denormal (r > 87) the result is 0 or 1 and the truth within 2^-126
  of it.  The logit's own bound passes through max sigmoid' = 1 / 4:
                                  e_y = e_r / 4 + y (1 - y) E_EXP (1 + |r|) u + 3 u y + 2^-126                                 [SIG]
"""
from __future__ import annotations

import os
import re

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vqdif_oracle as O
from decode_ref import U, gamma
from train_ref import E_EXP

ENC_G = O.G
F32 = np.float32
NORM_DIV32 = F32(1.101)            # SFMI_NORM_DIV
NORM_HI32 = F32(0.999)             # SFMI_NORM_HI
NORM_DIV = 1.0 + O.PAD + 10e-4
IX_SLACK_ULP = 2.0                 # [IX]
HERE = os.path.dirname(os.path.abspath(__file__))
ENCODER_HIP = os.path.join(os.path.dirname(HERE), "shapeformer_amd", "csrc", "encoder.hip")


def t64(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(a)
    return torch.as_tensor(a).detach().to("cpu", torch.float64)


def sd64(sd, prefix):
    return {k: t64(v) for k, v in sd.items() if k.startswith(prefix)}


# ---------------------------------------------------------------------------------------------------- float32 mirrors
def normalize_f32(p_half):
    """sfmi_normalize (csrc/sfmi_common.h) on an f32 array: __fdiv_rn by 1.101f, + 0.5f, the two clamps."""
    p_half = np.asarray(p_half)
    assert p_half.dtype == F32
    u = p_half / NORM_DIV32 + F32(0.5)
    u = np.where(u >= F32(1.0), NORM_HI32, u)
    u = np.where(u < F32(0.0), F32(0.0), u)
    assert u.dtype == F32
    return u


def cells_f32(cloud, R):
    """enc_cells_kernel: cloud (B,T,3) f32 in the [-1,1] frame -> cell (B,T) int32 = cx + 64 (cy + 64 cz), mask (B,R,R,R) bool [z][y][x]."""
    cloud = np.asarray(cloud)
    assert cloud.dtype == F32 and cloud.ndim == 3
    u = normalize_f32(cloud * F32(0.5))
    c = (u * F32(ENC_G)).astype(np.int32)
    cell = c[..., 0] + ENC_G * (c[..., 1] + ENC_G * c[..., 2])
    m = (u * F32(R)).astype(np.int32)
    mask = np.zeros((cloud.shape[0], R, R, R), bool)
    b = np.broadcast_to(np.arange(cloud.shape[0])[:, None], m.shape[:2])
    mask[b, m[..., 2], m[..., 1], m[..., 0]] = True
    return cell.astype(np.int32), mask


def axis_f32(x, G, with_ix=False):
    """sdf_axis (csrc/sdf_query.hip) on an f32 array of [-1,1]-frame coordinates -> i0, i1 (int32), w0, w1 (f32)."""
    x = np.asarray(x)
    assert x.dtype == F32
    u = normalize_f32(x * F32(0.5))
    v = F32(2.0) * u - F32(1.0)
    ix = ((v + F32(1.0)) / F32(2.0)) * F32(G - 1)
    ix = np.minimum(F32(G - 1), np.maximum(ix, F32(0.0)))
    f0 = np.floor(ix)
    i0 = f0.astype(np.int32)
    i1 = np.minimum(i0 + 1, G - 1).astype(np.int32)
    w1 = ix - f0
    w0 = (f0 + F32(1.0)) - ix
    assert ix.dtype == F32 and w0.dtype == F32 and w1.dtype == F32
    return (i0, i1, w0, w1, ix) if with_ix else (i0, i1, w0, w1)


def ix_f64(x, G):
    """The same expression in float64 on the same f32 coordinates (the clamps of normalize_3d and of the border gather included)."""
    u = np.asarray(x, np.float64) * 0.5 / NORM_DIV + 0.5
    u = np.where(u >= 1.0, 1.0 - 10e-4, u)
    u = np.where(u < 0.0, 0.0, u)
    return np.clip(u * (G - 1), 0.0, G - 1)


def ix_ulp_bound(G):
    """|axis_f32's ix - ix_f64| <= this.  u = p / 1.101f + 0.5f in [0, 1): the constant 1.101f is 2^-24 relative from 1.101 (the clamp
    constant 0.999f likewise), the division and the add round once each (2^-24 relative, 2^-25 absolute below 1): 2.5 * 2^-24 in u,
    i.e. <= 3 * 2^-24.  v = 2 u - 1 in [-1, 1) and v + 1 in [0, 2) round to 2^-24 and 2^-24 absolute at most (the halvings are exact):
    2^-24 more in u's units.  Times (G - 1), and the product rounds once: 2^-24 (G - 1)."""
    return (3.0 + 1.0 + 1.0) * U * (G - 1)


# ---------------------------------------------------------------------------------------------------- layers with their bounds
def lin(x, e, W, b=None):
    """One layer [LIN]: (W x + b, |W| e + gamma(K + 2) (|W| |x| + |b|)); x, e (..., K)."""
    mag = F.linear(x.abs(), W.abs(), None if b is None else b.abs())
    return F.linear(x, W, b), F.linear(e, W.abs()) + gamma(W.shape[1] + 2) * mag


def block_parts(sd, prefix, x, e_x=None):
    """One ResnetBlockFC (layers.py:39-48) at x (T,64) with the kernels' chains - h = fc_0(relu x) + b0, then b1 + shortcut(x) +
    fc_1(relu h) in ONE chain of 96 - -> o (T,32) by the oracle's resblock, eps (T,32) its local rounding ([LIN] for h, taken through
    W1 D_h, + [LIN] with K = 96; e_x: a bound of x itself, taken through |J|), J (T,32,64) = d o / d x."""
    W0, b0, W1, b1, Wsc = (sd[prefix + k] for k in ("fc_0.weight", "fc_0.bias", "fc_1.weight", "fc_1.bias", "shortcut.weight"))
    h = F.linear(F.relu(x), W0, b0)
    eps_h = gamma(W0.shape[1] + 2) * F.linear(F.relu(x), W0.abs(), b0.abs())
    W1D = W1[None] * (h > 0)[:, None, :].double()
    eps = gamma(W0.shape[1] + W1.shape[1] + 2) * (F.linear(x.abs(), Wsc.abs()) + F.linear(F.relu(h), W1.abs(), b1.abs()))
    eps = eps + torch.einsum("tij,tj->ti", W1D.abs(), eps_h)
    J = Wsc[None] + (W1D @ W0[None]) * (x > 0)[:, None, :].double()
    if e_x is not None:
        eps = eps + torch.einsum("tij,tj->ti", J.abs(), e_x)
    return O.resblock(sd, prefix, x), eps, J


SWEEP_F32 = 1.0 + 2.0 ** -10     # the sweep's own arithmetic is float32 (it forms a bound, not a value): sums of <= 5 * 300 * 32 positive terms


def _sweep(Wout, K, A, P, am, eps, device=None, rows=4096):
    """[JAC] for C cells of n points each: the outputs are Wout X_K per point (Wout (32,32); None: X_K itself) -> (C,n,32)
    sum_k |d out / d X_k| eps_k, k = K .. 0.  A[k], P[k] (C,n,32,32): d X_k / d X_{k-1} through the point's own features and through the
    pooled ones; am[k] (C,32): the pool's arg-max point per channel; eps[k] (C,n,32).  The sensitivities live as g (C, point p, output
    row (q,i), channel j), a chunk of rows at a time, on `device` (the GPU tests pass theirs: cells of 300 points cost 1e11 flop)."""
    C, n = eps[0].shape[:2]
    Rn = 32 * n
    dev = torch.device("cpu") if device is None else device
    out = torch.zeros(C, Rn, dtype=torch.float64)
    A, P, eps = ([None if t is None else t.float().to(dev) for t in x] for x in (A, P, eps))
    am = [None if t is None else t.to(dev) for t in am]
    W = torch.eye(32) if Wout is None else Wout.float()
    for r0 in range(0, Rn, rows):
        r = torch.arange(r0, min(Rn, r0 + rows))
        g = torch.zeros(C, n, len(r), 32)
        g[:, r // 32, torch.arange(len(r))] = W[r % 32]
        g = g.to(dev)
        tot = (g.abs() * eps[K][:, :, None]).sum((1, 3))
        for k in range(K, 0, -1):
            gm = torch.matmul(g, P[k]).sum(1)                                       # (C,R,32): through the pooled features
            g = torch.matmul(g, A[k])
            g.scatter_add_(1, am[k][:, None, None, :].expand(C, 1, g.shape[2], 32), gm[:, None])
            tot = tot + (g.abs() * eps[k - 1][:, :, None]).sum((1, 3))
        out[:, r0:r0 + len(r)] = tot.double().cpu() * SWEEP_F32
    return out.reshape(C, n, 32)


# ---------------------------------------------------------------------------------------------------- encoder
class EncRef:
    """cell (B,T) int32, mask (B,R,R,R) bool, stages: the five (B,T,32) block outputs, e_stages: {0, 1, 4: bound (B,T,32)}, c / e_c
    (B,T,32), occ (P,2) int64 [shape, cell] of the occupied cells (ascending), mean / e_mean (P,32), count (P),
    par (Q,4) int64 [shape, zo, yo, xo] of the 32^3 parents with points, down / e_down (Q,64) after ReLU."""


def down0_weight(sd):
    """encoder.downsampler.blocks.0.conv.weight (64,32,2,2,2) -> (64, 8 taps (dz,dy,dx) x 32 cin)."""
    w = t64(sd["encoder.downsampler.blocks.0.conv.weight"])
    return w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1)


def encoder_ref(sd, cloud, R, count_fault=None, relu=True, device=None):
    """sd: state dict with the reference's key names (numpy or torch); cloud (B,T,3) f32 numpy in the [-1,1] frame.
    count_fault = (shape, cell, d): the SEEDED FAULT of the CPU tests - that cell's mean is formed with a count off by d.
    device: where the [JAC] sweeps run (the values are float64 on the CPU either way)."""
    cloud = np.ascontiguousarray(cloud, F32)
    B, T, _ = cloud.shape
    r = EncRef()
    r.cell, r.mask = cells_f32(cloud, R)
    cell = torch.from_numpy(r.cell.astype(np.int64))
    s = sd64(sd, "encoder.")
    p = t64(cloud) * 0.5                                        # exact in f32
    x, e_x = lin(p, torch.zeros_like(p), s["encoder.fc_pos.weight"], s["encoder.fc_pos.bias"])
    net, e0, _ = block_parts(s, "encoder.blocks.0.", x.reshape(B * T, 64), e_x.reshape(B * T, 64))
    X, eps, Js = [net.reshape(B, T, 32)], [e0], [None]          # X[k] (B,T,32); eps[k] (B T,32); Js[k] (B T,32,64)
    for i in range(1, 5):
        x = torch.cat([X[-1], O.local_max_pool(X[-1], cell)], 2)
        net, e, J = block_parts(s, f"encoder.blocks.{i}.", x.reshape(B * T, 64))
        X.append(net.reshape(B, T, 32))
        eps.append(e)
        Js.append(J)
    r.stages = X
    Wc = s["encoder.fc_c.weight"]
    r.c, eps_c = lin(X[4], torch.zeros_like(X[4]), Wc, s["encoder.fc_c.bias"])
    # [JAC] per cell: the points of every cell, cells grouped by size
    key = (torch.arange(B)[:, None] * ENC_G ** 3 + cell).reshape(-1)
    order = torch.argsort(key, stable=True)
    _, counts = torch.unique_consecutive(key[order], return_counts=True)
    first = torch.cumsum(counts, 0) - counts
    e1, e4, ec = (torch.zeros(B * T, 32, dtype=torch.float64) for _ in range(3))
    for n in torch.unique(counts).tolist():
        pts = order[(first[counts == n][:, None] + torch.arange(n)[None])]                  # (C,n) flat point indices
        C = pts.shape[0]
        A = [None] + [Js[k][pts][..., :32] for k in range(1, 5)]
        P = [None] + [Js[k][pts][..., 32:] for k in range(1, 5)]
        am = [None] + [X[k - 1].reshape(B * T, 32)[pts].argmax(1) for k in range(1, 5)]
        ep = [eps[k][pts] for k in range(5)]
        e1[pts] = _sweep(None, 1, A, P, am, ep, device)
        e4[pts] = _sweep(None, 4, A, P, am, ep, device)
        ec[pts] = _sweep(Wc, 4, A, P, am, ep, device)
    r.e_stages = {0: eps[0].reshape(B, T, 32), 1: e1.reshape(B, T, 32), 4: e4.reshape(B, T, 32)}
    r.e_c = ec.reshape(B, T, 32) + eps_c
    mean_down(sd, r, count_fault, relu)
    return r


def mean_down(sd, r, count_fault=None, relu=True):
    """r.c, r.e_c (B,T,32) and r.cell -> r.occ, r.count, r.mean, r.e_mean [MEAN], r.par, r.down, r.e_down (EncRef).  Also the ANCHORED form
    of the GPU tests: with r.c a kernel's own per-point c (exact in float64) and r.e_c = 0 the bounds are those of the mean and the
    convolution alone."""
    B = r.c.shape[0]
    cell = torch.from_numpy(np.asarray(r.cell).astype(np.int64))
    # per-cell mean (dense through the oracle's grid_mean, then the occupied cells only)
    dense = O.grid_mean(r.c, cell).reshape(B, 32, -1)                              # (B,32,G^3), [z][y][x] flattened = the cell id
    e_dense = O.grid_mean(r.e_c, cell).reshape(B, 32, -1)
    cnt = torch.zeros(B, ENC_G ** 3, dtype=torch.int64).scatter_add_(1, cell, torch.ones_like(cell))
    if count_fault is not None:
        fb, fc, d = count_fault
        dense[fb, :, fc] *= float(cnt[fb, fc]) / float(cnt[fb, fc] + d)
    r.occ = torch.nonzero(cnt)                                                     # ascending (shape, cell)
    r.count = cnt[r.occ[:, 0], r.occ[:, 1]]
    r.mean = dense[r.occ[:, 0], :, r.occ[:, 1]]
    r.e_mean = e_dense[r.occ[:, 0], :, r.occ[:, 1]] + 2.0 ** -33 + U * r.mean.abs()
    # first Downsampler convolution at the parents that hold points: children gathered as [tap (dz,dy,dx)][cin]
    H = ENC_G // 2
    e_dense[r.occ[:, 0], :, r.occ[:, 1]] = r.e_mean

    def children(d):
        d = d.reshape(B, 32, H, 2, H, 2, H, 2).permute(0, 2, 4, 6, 3, 5, 7, 1)      # (B,zo,yo,xo,dz,dy,dx,c)
        return d.reshape(B, H, H, H, 256)
    pocc = (cnt.reshape(B, H, 2, H, 2, H, 2).sum((2, 4, 6)) > 0)
    r.par = torch.nonzero(pocc)
    idx = tuple(r.par.T)
    y, ey = lin(children(dense)[idx], children(e_dense)[idx], down0_weight(sd))
    r.down, r.e_down = (F.relu(y), ey) if relu else (y, ey)
    return r


def anchored_ref(sd, cell, s4c):
    """The kernel's own taps as inputs (s4c (B,T,64) f32 = [block-4 output | c]): c = fc_c(its block-4 output) with [LIN]'s local bound
    alone, mean / down0 of its own c with [MEAN] / [LIN] alone - no error travels further than one layer, so these gates sit at the
    f32 noise itself (1e-6) where the from-scratch bounds of encoder_ref, five blocks deep, stand at 1e-3."""
    s = sd64(sd, "encoder.")
    r = EncRef()
    r.cell = cell
    net = t64(s4c[..., :32])
    r.c_from_net, r.e_c_from_net = lin(net, torch.zeros_like(net), s["encoder.fc_c.weight"], s["encoder.fc_c.bias"])
    r.c = t64(s4c[..., 32:])
    r.e_c = torch.zeros_like(r.c)
    return mean_down(sd, r)


# ---------------------------------------------------------------------------------------------------- fused kernel's ownership rule
def fused_constants():
    """EF_CAP, EF_LIMIT, EF_NOM as csrc/encoder.hip declares them (a changed declaration fails here, loudly)."""
    src = open(ENCODER_HIP).read()
    m = re.search(r"constexpr int EF_CAP = (\d+), EF_LIMIT = (\d+), EF_NOM = EF_CAP - EF_LIMIT,", src)
    assert m, "csrc/encoder.hip no longer declares EF_CAP / EF_LIMIT / EF_NOM in the form this mirror reads"
    cap, limit = int(m.group(1)), int(m.group(2))
    assert re.search(r"dim3\(\(T \+ EF_NOM - 1\) / EF_NOM, B\)", src), "enc_fused_kernel's grid rule changed"
    assert re.search(r"int p0 = blockIdx\.x \* EF_NOM, p1 = min\(T, p0 \+ EF_NOM\);", src), "enc_fused_kernel's ownership rule changed"
    return cap, limit, cap - limit


EF_CAP, EF_LIMIT, EF_NOM = fused_constants()


def runs_of(sorted_cells):
    """start[i], end[i]: the run (cell) of sorted position i as [start, end)."""
    sc = np.asarray(sorted_cells)
    T = len(sc)
    first = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
    length = np.diff(np.r_[first, T])
    return np.repeat(first, length), np.repeat(first + length, length)


def fused_declines(sorted_cells):
    """The scan kernel's flag: a cell of the shape holds more than EF_LIMIT points -> the staged kernels take the shape."""
    st, en = runs_of(sorted_cells)
    return bool((en - st).max() > EF_LIMIT)


def fused_ownership(sorted_cells, T):
    """enc_fused_kernel's [p0, p1) of every workgroup of one shape (sorted_cells: its T cell ids in ascending order): the runs that
    START in [w EF_NOM, (w + 1) EF_NOM) - the tail of a run begun before is skipped, the run that straddles the end is finished."""
    assert len(sorted_cells) == T
    st, en = runs_of(sorted_cells)
    out = []
    for w in range((T + EF_NOM - 1) // EF_NOM):
        p0 = w * EF_NOM
        p1 = min(T, p0 + EF_NOM)
        if 0 < p0 < T and st[p0] < p0:
            p0 = int(en[p0])
        if p1 < T and st[p1] < p1:
            p1 = int(en[p1])
        out.append((p0, max(p0, p1)))
    return out


# ---------------------------------------------------------------------------------------------------- cloud builders
def cell_xyz(c):
    c = np.asarray(c, np.int64)
    return np.stack([c % ENC_G, (c // ENC_G) % ENC_G, c // (ENC_G * ENC_G)], -1)


def build_cloud(cells, seed, shuffle_seed=None):
    """cells: [(cell id, point count), ...] -> (T,3) f32: every point at 2 * 1.101 * ((c + f) / 64 - 0.5), f in [0.2, 0.8] per axis
    (the mirror asserts it fell in its cell), then shuffled by a seeded permutation (shuffle_seed: another order of the SAME points)."""
    g = np.random.default_rng(seed)
    ids = np.repeat([c for c, _ in cells], [n for _, n in cells])
    f = 0.2 + 0.6 * g.random((len(ids), 3))
    pts = (2.0 * NORM_DIV * ((cell_xyz(ids) + f) / ENC_G - 0.5)).astype(F32)
    got, _ = cells_f32(pts[None], 16)
    assert np.array_equal(got[0], ids), "a built point left its intended cell"
    perm = np.random.default_rng(seed + 1 if shuffle_seed is None else shuffle_seed).permutation(len(ids))
    return np.ascontiguousarray(pts[perm])


def singles(first, n, step=7):
    """n single-point cells first, first + step, ..."""
    return [(first + step * k, 1) for k in range(n)]


def face_cloud(T, seed):
    """(T,3) f32 of coordinates ON cell faces (f = 0: 2 * 1.101 * (c / 64 - 0.5), and the f32 neighbours on either side), on the faces of
    the 16^3 / 32^3 mask cells, and at / outside the box: +-1.0, +-1.101, +-1.3.  Which side of a face a value falls on is decided
    by the f32 operation sequence alone."""
    vals = []
    for c in (0, 1, 2, 4, 31, 32, 33, 36, 62, 63, 64):
        v = F32(2.0 * NORM_DIV * (c / ENC_G - 0.5))
        vals += [v, np.nextafter(v, F32(2)), np.nextafter(v, F32(-2))]
    vals += [F32(s * a) for s in (1, -1) for a in (1.0, 1.101, 1.3)] + [F32(0.0), F32(-0.0)]
    vals = np.array(vals, F32)
    g = np.random.default_rng(seed)
    pts = vals[g.integers(0, len(vals), (T, 3))]
    pts[: len(vals)] = np.stack([vals, np.roll(vals, 5), np.roll(vals, 11)], -1)[:T]     # every value at least once per axis
    return np.ascontiguousarray(pts)


# ---------------------------------------------------------------------------------------------------- VQ
def vq_ref(x, W, same=()):
    """x (N,D), W (K,D) f32 -> float64 distances (N,K) = |x|^2 - 2 x.w + |w|^2 and their [VQ] bound.  same: [(lo, hi), ...] codes whose
    rows are bit-identical - their distances are one number, and are returned as one (a BLAS matmul does not promise the same
    additions in the same order for two columns)."""
    x, W = t64(x), t64(W)
    D = x.shape[1]
    xx, ww = (x * x).sum(1, keepdim=True), (W * W).sum(1)[None]
    d, e = xx - 2.0 * (x @ W.T) + ww, gamma(D + 3) * (xx + 2.0 * (x.abs() @ W.abs().T) + ww)
    for lo, hi in same:
        assert torch.equal(W[lo], W[hi])
        d[:, hi], e[:, hi] = d[:, lo], e[:, lo]
    return d, e


def vq_argmin_ref(d, lowest=True):
    """The documented tie rule on a distance matrix: the LOWEST code index among the minima (lowest=False: the seeded fault)."""
    if lowest:
        return torch.argmin(d, 1)       # first minimum
    return d.shape[1] - 1 - torch.argmin(d.flip(1), 1)


def tie_codebook(K, D, seed, scale=0.5):
    """(K,D) f32 codebook with bit-identical duplicate rows (4, 8), (3, 35) [K > 35] and (0, K - 1); -> W, [(low, high), ...]."""
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(K, D, generator=g) * scale).numpy()
    pairs = [(4, 8), (0, K - 1)] + ([(3, 35)] if K > 35 else [])
    for lo, hi in pairs:
        W[hi] = W[lo]
    return W, pairs


# ---------------------------------------------------------------------------------------------------- decoder query
def gather_ref(grid, xyz, affine=None):
    """grid (B,32,G,G,G) f32, xyz (B,N,3) f32 ([-1,1] frame) -> c (B,N,32) float64 through axis_f32's cells and weights, its rounding
    bound e_c and the [IX] slack s_c (both (B,N,32))."""
    B, _, G = grid.shape[:3]
    xyz = np.ascontiguousarray(np.asarray(xyz), F32)
    ax = [axis_f32(xyz[..., a], G, with_ix=True) for a in range(3)]
    g = torch.as_tensor(grid).permute(0, 2, 3, 4, 1)           # (B,z,y,x,32); gathered in f32, widened after (exact)
    b = torch.arange(B)[:, None].expand(B, xyz.shape[1])
    c = mag = 0.0
    lo = hi = None
    for corner in range(8):
        dz, dy, dx = corner >> 2, (corner >> 1) & 1, corner & 1
        idx = [torch.from_numpy(ax[a][1 if d else 0].astype(np.int64)) for a, d in ((0, dx), (1, dy), (2, dz))]
        w = [t64(ax[a][3 if d else 2]) for a, d in ((0, dx), (1, dy), (2, dz))]
        v = g[b, idx[2], idx[1], idx[0]].double()              # (B,N,32)
        wt = (w[0] * w[1] * w[2])[..., None]
        c, mag = c + wt * v, mag + wt * v.abs()
        lo, hi = (v, v) if lo is None else (torch.minimum(lo, v), torch.maximum(hi, v))
    ulp = sum(t64(np.spacing(np.maximum(ax[a][4], F32(1.0)))) for a in range(3))       # ulp(ix) per axis, ix < 1 counted as 1
    e = gamma(10) * mag
    s = IX_SLACK_ULP * ulp[..., None] * (hi - lo)
    if affine is not None:
        sc, sh = t64(affine[0])[:, None], t64(affine[1])[:, None]
        c, e, s = c * sc + sh, e * sc.abs() + U * (c * sc + sh).abs(), s * sc.abs()
    return c, e, s


def mlp_ref(sd, xyz, c, e_c, s_c):
    """dec.py:88-100 in float64 with the kernel's chains -> logits (B,N), bound (B,N) by [JAC] (every rounding site's eps, e_c and the
    [IX] slack s_c of the gathered features through the logit's sensitivities: one autograd pass, the points are independent),
    slack (B,N): the s_c part alone."""
    s = sd64(sd, "decoder.")
    p = t64(np.asarray(xyz)) * 0.5
    sites = []

    def site(t, eps):                         # t + 0 with the zero a leaf: its gradient is d logit / d t
        z = torch.zeros_like(t, requires_grad=True)
        sites.append((z, eps.detach()))
        return t + z
    c = site(c, e_c + s_c)
    Wp, bp = s["decoder.fc_p.weight"], s["decoder.fc_p.bias"]
    net = site(F.linear(p, Wp, bp), gamma(Wp.shape[1] + 2) * F.linear(p.abs(), Wp.abs(), bp.abs()))
    for i in range(5):
        Wc, W0, b0, W1 = (s[k.format(i)] for k in ("decoder.fc_c.{}.weight", "decoder.blocks.{}.fc_0.weight", "decoder.blocks.{}.fc_0.bias",
                                                    "decoder.blocks.{}.fc_1.weight"))
        b = s[f"decoder.fc_c.{i}.bias"] + (s[f"decoder.blocks.{i - 1}.fc_1.bias"] if i else 0.0)
        net = site(net + F.linear(c, Wc, b), gamma(36) * (net.abs() + F.linear(c.abs(), Wc.abs(), b.abs())))                    # [ACC] K + 4
        h = site(F.linear(F.relu(net), W0, b0), gamma(34) * F.linear(F.relu(net), W0.abs(), b0.abs()))
        net = site(net + F.linear(F.relu(h), W1), gamma(35) * (net.abs() + F.linear(F.relu(h), W1.abs())))                      # [ACC] K + 3
    a = net + s["decoder.blocks.4.fc_1.bias"]
    a = site(a, U * a.abs())
    Wo, bo = s["decoder.fc_out.weight"], s["decoder.fc_out.bias"]
    out = F.linear(F.relu(a), Wo, bo)
    bound = gamma(34) * F.linear(F.relu(a), Wo.abs(), bo.abs())
    grads = torch.autograd.grad(out.sum(), [z for z, _ in sites])
    bound = bound[..., 0].detach() + sum((g.abs() * eps).sum(-1) for g, (_, eps) in zip(grads, sites))
    return out[..., 0].detach(), bound, (grads[0].abs() * s_c).sum(-1)


def query_ref(sd, grid, xyz, affine=None):
    """-> logits (B,N) float64, bound (B,N) (rounding + [IX] slack), slack (B,N) (the [IX] part alone)."""
    c, e, sl = gather_ref(grid, xyz, affine)
    return mlp_ref(sd, xyz, c, e, sl)


def sigmoid_bound(logit, bound):
    """[SIG]: -> sigmoid(logit), |err| bound."""
    y = torch.sigmoid(logit)
    return y, 0.25 * bound + y * (1.0 - y) * E_EXP * (1.0 + logit.abs()) * U + 3.0 * U * y + 2.0 ** -126


def lattice_points(axis, B, x_range=None):
    """nputil.makeGrid 'ij' from an f32 axis table: (B, Q^3 or slab, 3) f32, x slowest."""
    axis = np.asarray(axis, F32)
    ax = axis if x_range is None else axis[x_range[0]:x_range[1]]
    p = np.stack(np.meshgrid(ax, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    return np.ascontiguousarray(np.broadcast_to(p[None], (B,) + p.shape))


def query_points(B, N, G, seed):
    """(B,N,3) f32: +-1.0, +-1.3, +-1.101, points ON feature-cell faces (ix integral) and one f32 step either side of them, then
    uniform points in [-1.3, 1.3]^3."""
    vals = [F32(s * a) for s in (1, -1) for a in (1.0, 1.3, 1.101)]
    for k in sorted({0, 1, (G - 1) // 2, G - 2, G - 1}):
        v = F32(2.0 * NORM_DIV * (k / (G - 1) - 0.5))
        vals += [v, np.nextafter(v, F32(2)), np.nextafter(v, F32(-2))]
    vals = np.array(vals, F32)
    g = np.random.default_rng(seed)
    pts = (g.random((B, N, 3)) * 2.6 - 1.3).astype(F32)
    n = min(N, len(vals))
    for b in range(B):
        pts[b, :n] = np.stack([np.roll(vals, b), np.roll(vals, 3 + b), np.roll(vals, 7 + 2 * b)], -1)[:n]
    return pts
