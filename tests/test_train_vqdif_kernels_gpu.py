"""Every entry of csrc/train_vqdif.hip (and the forward sfmi_maxpool2_cl_f32 / sfmi_upcat_cl_f32 / sfmi_affine_cl_f32 of csrc/conv3d.hip)
through the C ABI against float64 (tests/train_vqdif_ref.py: references, derived per-element bounds, f32 mirrors of the index arithmetic
and of the launch rules), at every launch form: ReLU backward, the linear combination, the two per-(sample, channel) affine maps, the
GroupNorm-backward statistics at every rpp class and slice count, nearest upsampling / its sum-pool backward / the 2^3 max-pool forward
and backward / upsample + concat on every tie pattern, the point -> cell index, the encoder's local max pool forward and backward (the
tie contract: one winner per (cell, channel), the lowest-indexed point that attains the maximum), the 2^-32 fixed-point scatter-add,
scatter-mean and its backward, trilinear sampling forward and backward, BCE with logits, the quantizer's EMA statistics and update, the
conv / linear weight gradient at every tap geometry and slice count, one training step on a cloud drawn with replacement (as the data
loader draws it), and the argument checks (by return value).  Every float output sits SENT-filled between guard bands, every input
between NaN bands; every `[ratio]` line (pytest -s) is the largest error / bound of a family.  The case tables below are plain data:
tests/test_train_vqdif_ref_cpu.py imports them and proves, from the mirrors, that they reach every form.

Measured on one MI355X (largest error / bound per family): lincomb 0.998 (one rounding is the bound), affine 0.50, affine2
0.71, chan_dot_stats 0.32 (f64 roundings), scatter_add 0.999 (sfmi_fixed_to_float_f32 of the accumulator) and cell_mean 0.999 (the rounding to the 2^-32 grid / to f32 is the bound),
cell_mean_bwd 0.90, trilinear 0.40, trilinear_bwd 0.9999 (a lone point-corner pair at scale 1e-8: the grid rounding is the bound), BCE loss
0.18 / dlogits 0.15, vq_ema N 0.50 / z 0.81 / emb 0.22, wgrad 0.30; ReLU backward, pooling and resampling, both max-pools, the cell index,
the local max pool forward and backward and vq_stats are bit-exact.  Every bit-identity claim held (three runs and a permutation of the
points: scatter_add, trilinear_bwd).  The step on the redrawn cloud: worst tensor 1.0e-5 max-normalised under frozen masks.  Defect found
and fixed: the ties of the local max-pool backward (test_cell_max_backward_routes_each_cell_gradient_to_one_point); host defects: the
argument checks at the end of this file.  The file runs in 5 s."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import train_vqdif_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
SENT = 0x7FC0DEAD                    # NaN bit pattern of every "must stay untouched" float
SENT64 = 0x7FF80000DEADBEEF          # the same for a float64 output
ISENT = -0x5EAD                      # guard value of integer buffers
GUARD = 256                          # band elements on either side of every buffer
U = R.U
EINVAL = -1

# ---------------------------------------------------------------------------------------------------- the case tables
RELU_N = (4, 1020, 1024, 1028, 4 * 65537)
LINCOMB_N = (1, 255, 256, 257, 4099)
QUANT_BETA = 0.001
LINCOMB_AB = ("sub", "commit", "general", "no_y")          # _quantize's (1, -1) and (1, 2 beta / n); arbitrary scalars; y == NULL
AFFINE_CASES = [(1, 1, 4), (2, 5, 12), (3, 33, 64), (2, 64, 768)]     # (B, V, C)
CDS_C = (4, 12, 48, 64, 768, 1024)


def _cds_cases():
    """(B, V, C, S): per C every V around its rpp, one S > V (empty slices), V = 4097 at S = sfmi_gn_splits(V) = 16, B = 3 once per C"""
    out = []
    for C in CDS_C:
        rpp = R.chan_rpp(C)[1]
        for V in sorted({1, 3, rpp - 1, rpp, rpp + 1} - {0}):
            out.append((1, V, C, 1))
        out += [(3, rpp + 1, C, 4), (1, 3, C, 4), (1, 4097, C, 16)]
    out += [(3, 4097, 12, 16), (3, 1, 4, 16)]
    return out


CDS_CASES = _cds_cases()
GN_SPLIT_V = (1, 511, 512, 4095, 4096, 4097, 32767, 32768, 262144)
POOL_EXTENTS, POOL_C, POOL_B = [(1, 2, 3), (3, 1, 2), (4, 4, 4)], (4, 12, 64), (1, 3)       # extents of the COARSE grid
POOL_CASES = [(B, e, C) for B in POOL_B for e in POOL_EXTENTS for C in POOL_C]


def pool_shift(B, ext, C):
    """offset of the first window's pattern, so that small cases start at different patterns"""
    return 7 * POOL_CASES.index((B, ext, C))


CELLS_G = (2, 64)
CELL_POOL_C, CELL_POOL_SEEDS = (4, 32), (1, 2)
SCATTER_FORMS = [("one_cell", 300), ("one_each", 8)]          # all points in one cell (maximum contention) / one point per cell
SCATTER_SCALES = (1.0, 1e-4, 1e-8)
SCATTER_C, NCELL = (4, 32), 8
TRI_CASES = [(2, 4, 1), (2, 32, 255), (2, 4, 257), (3, 32, 1), (3, 4, 255), (3, 32, 257), (64, 4, 1), (64, 4, 255), (64, 32, 257)]   # (G, C, N), B = 2
BCE_LOGITS = (0.0, 1e-8, -1e-8, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4)
BCE_LABELS = (0.0, 1.0, 0.25)
BCE_N = (1, 255, 256, 257)
VQ_STATS_CASES = [(rows, D, K) for rows in (1, 300) for D in (4, 256) for K in (1, 5, 4096)]
VQ_EMA_CASES = [(K, D) for K in (1, 1000, 1024, 1025, 4096) for D in (4, 256)]
VQ_GAMMA, VQ_EPS = 0.99, 1e-7
# weight gradient: name, B, Di, Hi, Wi, Cin, Cout, KS, stride, pad, ldy, ldx, form ('' | 'fc_out': only column 0 of dy is non-zero |
# 'nan_pad': the columns of dy / x beyond Cout / Cin hold NaN and must never be read)
WG_LIN_M = (1, 15, 16, 17, 700)
WG_LIN_SHAPES = [(3, 64, 64, 16, "nan_pad"), (16, 32, 32, 16, ""), (48, 96, 96, 48, ""), (64, 64, 64, 64, ""), (65, 130, 133, 67, "nan_pad"),
                 (32, 32, 32, 32, "fc_out"), (32, 1, 32, 32, "nan_pad")]          # (Cin, Cout, ldy, ldx, form)
WG_CONV_GEOM = [("k3p1", 3, 1, 1), ("k2s2", 2, 2, 0), ("k1", 1, 1, 0), ("k3p0", 3, 1, 0)]
WG_CONV_EXT = [(3, 4, 5), (4, 4, 4)]
WG_CONV_CH = [(32, 64), (64, 32), (128, 128)]
WG_UNET_NSPLITS = (1, 2, 4, 10, 13, 16, 38, 128)    # what VQDIFTrainer._wgrad_into picks for UNet3D's layers at res 16 / 32, B = 1 (test_train_vqdif_ref_cpu.py)


def _wg_cases():
    out = []
    for M in WG_LIN_M:
        for Cin, Cout, ldy, ldx, form in WG_LIN_SHAPES:
            out.append((f"lin M{M} {Cin}->{Cout} {form}".strip(), 1, 1, 1, M, Cin, Cout, 1, 1, 0, ldy, ldx, form))
    for gname, KS, st, pad in WG_CONV_GEOM:
        for ext in WG_CONV_EXT:                                  # k2 s2 on (3, 4, 5): the output extent is a floor, the last plane / column is unread
            for Cin, Cout in WG_CONV_CH:
                out.append((f"{gname} {ext} {Cin}->{Cout}", 2, *ext, Cin, Cout, KS, st, pad, Cout, Cin, ""))
    out.append(("k3p1 (4, 4, 4) 768->256", 2, 4, 4, 4, 768, 256, 3, 1, 1, 256, 768, ""))
    return out


WG_CASES = _wg_cases()


def wg_nsplits(case):
    """1, 3, the smallest count whose last slices are empty; the narrow 3^3 pad 1 convolutions also run at every count the trainer picks for UNet3D"""
    _, B, Di, Hi, Wi, Cin, Cout, KS, st, pad = case[:10]
    rows = R.wgrad_rows(B, Di, Hi, Wi, KS, st, pad)
    ns = [1, 3, R.wgrad_empty_nsplit(rows)]
    if KS == 3 and pad == 1 and Cin * Cout <= 64 * 32:
        ns += [n for n in WG_UNET_NSPLITS if n not in ns]
    return ns


REDRAW_SEED = 0                      # np.random.RandomState(seed).choice(T, T, replace=True) of the fixture's Xbd; no tie between distinct points
FROZEN_GATE = 1e-4                   # tests/test_train_vqdif_gpu.py: every tensor under frozen ReLU masks and pool indices


# ---------------------------------------------------------------------------------------------------- plumbing
def _L():
    from shapeformer_amd import _lib as L
    return L


def _rc(name, *args):
    L = _L()
    return int(getattr(L.lib(), name)(*[a.data_ptr() if torch.is_tensor(a) else a for a in args], L.stream_ptr()))


def _call(name, *args):
    _L().check(_rc(name, *args), name)
    torch.cuda.synchronize()


def _in(t, dev, dtype=torch.float32):
    """a device copy of t between two NaN (or, for integers, sentinel) bands"""
    t = torch.as_tensor(np.ascontiguousarray(t) if isinstance(t, np.ndarray) else t)
    n = t.numel()
    fill = float("nan") if dtype.is_floating_point else ISENT
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    buf[GUARD:GUARD + n] = t.reshape(-1).to(dev, dtype)
    return buf[GUARD:GUARD + n].view(t.shape)


class Out:
    """a float output: SENT everywhere, the data view between two guard bands; init: values an accumulating / in-place entry starts from"""

    def __init__(self, shape, dev, init=None, f64=False):
        self.n = int(np.prod(shape))
        self.it, self.sent = (torch.int64, SENT64) if f64 else (torch.int32, SENT)
        self.buf = torch.full((self.n + 2 * GUARD,), self.sent, dtype=self.it, device=dev).view(torch.float64 if f64 else torch.float32)
        self.v = self.buf[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.v.copy_(torch.as_tensor(init).reshape(shape).to(dev))

    def check(self, what, written=True):
        bits = self.buf.view(self.it)
        assert bool((bits[:GUARD] == self.sent).all()) and bool((bits[GUARD + self.n:] == self.sent).all()), f"{what}: wrote outside the output"
        if written:
            assert not bool((bits[GUARD:GUARD + self.n] == self.sent).any()), f"{what}: left part of the output unwritten"
        return self.v

    def np(self, what, written=True):
        return self.check(what, written).cpu().numpy()

    def untouched(self, what):
        assert bool((self.buf.view(self.it) == self.sent).all()), f"{what}: a refused call wrote to its output"


class IOut:
    """an integer buffer (accumulator, count, key, index) holding `fill` between two guard bands"""

    def __init__(self, shape, dev, dtype, fill=0):
        self.n = int(np.prod(shape))
        self.fill = fill
        self.buf = torch.full((self.n + 2 * GUARD,), ISENT, dtype=dtype, device=dev)
        self.v = self.buf[GUARD:GUARD + self.n].view(shape)
        self.v.fill_(fill)

    def np(self, what):
        assert bool((self.buf[:GUARD] == ISENT).all()) and bool((self.buf[GUARD + self.n:] == ISENT).all()), f"{what}: wrote outside the buffer"
        return self.v.cpu().numpy()

    def untouched(self, what):
        assert bool((self.v == self.fill).all()), f"{what}: a refused call wrote to its output"
        self.np(what)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_bits(a, b):
    return bool(np.array_equal(_bits(a), _bits(b)))


def _rs(seed):
    return np.random.RandomState(seed)


def _dyadic(rs, shape):
    """f32 values on a 2^-3 grid in [-8, 8]: sums of eight of them are exact"""
    return (rs.randint(-64, 65, size=shape) / 8.0).astype(np.float32)


WORST = {}


def _note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def _report(*families):
    for f in families:
        print(f"[ratio] {f}: largest error / bound {int(WORST.get(f, 0.0) * 10000) / 10000:.4f}")     # rounded down


# ---------------------------------------------------------------------------------------------------- elementwise
@pytest.mark.parametrize("n", RELU_N)
def test_relu_bwd_exact_on_zeros_denormals_and_negatives(dev, n):
    rs = _rs(n)
    y, dy = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    y[:4] = np.array([0.0, -0.0, 1e-40, -1.0], np.float32)               # +0, -0: gradient 0; a positive denormal: passes; a negative
    if n > 8:
        y[-4:] = np.array([-1e-40, 2.0 ** -126, -0.0, 0.0], np.float32)
    dy[1], dy[2] = -0.0, -3.5
    o = Out((n,), dev)
    _call("sfmi_relu_bwd_f32", _in(dy, dev), _in(y, dev), o.v, n)
    assert _same_bits(o.np(f"relu_bwd n{n}"), R.relu_bwd_ref(dy, y))


def lincomb_ab(kind, n):
    return dict(sub=(1.0, -1.0), commit=(1.0, 2.0 * QUANT_BETA / n), general=(0.37, -1.9), no_y=(-1.25, 7.0))[kind]


@pytest.mark.parametrize("n", LINCOMB_N)
def test_lincomb_both_forms(dev, n):
    rs = _rs(n)
    x, y = rs.randn(n).astype(np.float32), (rs.randn(n) * 3).astype(np.float32)
    xd, yd = _in(x, dev), _in(y, dev)
    for kind in LINCOMB_AB:
        a, b = lincomb_ab(kind, n)
        o = Out((n,), dev)
        _call("sfmi_lincomb_f32", _L().f32(a), xd, _L().f32(b), None if kind == "no_y" else yd, o.v, n)
        ref, bnd = R.lincomb_ref(a, x, b, None if kind == "no_y" else y)
        assert _note("lincomb", R.ratio(o.np(f"lincomb {kind} n{n}"), ref, bnd)) <= 1.0, (kind, n)
    _report("lincomb")


@pytest.mark.parametrize("B,V,C", AFFINE_CASES)
def test_affine_maps_index_their_coefficients_by_sample_and_channel(dev, B, V, C):
    rs = _rs(B * 1000 + V + C)
    u, v = rs.randn(B, V, C).astype(np.float32), (rs.randn(B, V, C) + 1).astype(np.float32)
    A, Bc, Cc = ((rs.randn(B, C) * 2 + 0.01 * np.arange(B * C).reshape(B, C)).astype(np.float32) for _ in range(3))   # distinct per (b, c)
    o = Out((B, V, C), dev)
    _call("sfmi_affine2_cl_f32", _in(u, dev), _in(v, dev), _in(A, dev), _in(Bc, dev), _in(Cc, dev), o.v, B, V, C)
    ref, bnd = R.affine2_ref(u, v, A, Bc, Cc)
    assert _note("affine2", R.ratio(o.np(f"affine2 {B, V, C}"), ref, bnd)) <= 1.0
    o = Out((B, V, C), dev)
    _call("sfmi_affine_cl_f32", _in(u, dev), _in(A, dev), _in(Cc, dev), o.v, B, V, C)
    ref, bnd = R.affine_ref(u, A, Cc)
    assert _note("affine", R.ratio(o.np(f"affine {B, V, C}"), ref, bnd)) <= 1.0
    _report("affine2", "affine")


def test_gn_splits_mirror(dev):
    lib = _L().lib()
    for V in GN_SPLIT_V:
        assert int(lib.sfmi_gn_splits(V)) == R.gn_splits(V), V


@pytest.mark.parametrize("C", CDS_C)
def test_chan_dot_stats_every_rpp_class_and_slice_count(dev, C):
    for B, V, Cc, S in (c for c in CDS_CASES if c[2] == C):
        rs = _rs(V * 7 + S + B)
        dy, x = rs.randn(B, V, C).astype(np.float32), (rs.randn(B, V, C) * 2 + 0.5).astype(np.float32)
        o = Out((B, S, C, 2), dev, f64=True)
        _call("sfmi_chan_dot_stats_f32", _in(dy, dev), _in(x, dev), o.v, B, V, C, S)
        got = o.np(f"chan_dot_stats {B, V, C, S}")
        ref, bnd = R.chan_dot_stats_ref(dy, x, S)
        assert np.isfinite(got).all()
        for s in range(S):
            v0, v1 = R.stats_slice(V, s, S)
            if v1 == v0:
                assert not got[:, s].any(), f"empty slice {s} of {B, V, C, S} is not zero"
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bnd)
        assert _note("chan_dot_stats", float(r.max())) <= 1.0, (B, V, C, S)
    _report("chan_dot_stats")


# ---------------------------------------------------------------------------------------------------- pooling / resampling
@pytest.mark.parametrize("B,ext,C", POOL_CASES)
def test_pooling_and_resampling_exact_on_every_tie_pattern(dev, B, ext, C):
    D, H, W = ext
    rs = _rs(B + 10 * C + sum(ext))
    what = f"{B, ext, C}"
    # nearest x2 and upsample + concat
    low = _dyadic(rs, (B, D, H, W, C))
    o = Out((B, 2 * D, 2 * H, 2 * W, C), dev)
    _call("sfmi_upsample2_cl_f32", _in(low, dev), o.v, B, D, H, W, C)
    assert _same_bits(o.np("upsample2 " + what), R.upsample2_ref(low))
    Cs = POOL_C[(POOL_C.index(C) + 1) % len(POOL_C)]
    skip = _dyadic(rs, (B, 2 * D, 2 * H, 2 * W, Cs))
    o = Out((B, 2 * D, 2 * H, 2 * W, Cs + C), dev)
    _call("sfmi_upcat_cl_f32", _in(skip, dev), _in(low, dev), o.v, B, 2 * D, 2 * H, 2 * W, Cs, C)
    assert _same_bits(o.np("upcat " + what), R.upcat_ref(skip, low))
    # sum-pool of a channel slice (the backward of the above): the whole width, and an inner slice
    for Ct, c0 in ((C, 0), (C + 8, 4)):
        dy = _dyadic(rs, (B, 2 * D, 2 * H, 2 * W, Ct))
        o = Out((B, D, H, W, C), dev)
        _call("sfmi_sumpool2_cl_f32", _in(dy, dev), o.v, B, D, H, W, Ct, c0, C)
        assert _same_bits(o.np(f"sumpool2 {what} c0 {c0}"), R.sumpool2_ref(dy, c0, C).astype(np.float32))
    # 2^3 max-pool forward and backward
    x, _ = R.pool_input(B, D, H, W, C, pool_shift(B, ext, C))
    xd = _in(x, dev)
    o = Out((B, D, H, W, C), dev)
    _call("sfmi_maxpool2_cl_f32", xd, o.v, B, D, H, W, C)
    y, yref = o.np("maxpool2 " + what), R.maxpool2_ref(x)
    assert np.array_equal(y, yref) and _same_bits(np.where(yref != 0, y, 0), np.where(yref != 0, yref, 0))   # fmaxf(-0, +0) may return either zero
    dy = rs.randn(B, D, H, W, C).astype(np.float32)
    o = Out(x.shape, dev)
    _call("sfmi_maxpool2_bwd_cl_f32", xd, _in(y, dev), _in(dy, dev), o.v, B, D, H, W, C)
    dx = o.np("maxpool2_bwd " + what)
    assert _same_bits(dx, R.maxpool2_bwd_ref(x, y, dy))
    assert _same_bits(R._windows(dx).astype(np.float64).sum(-1).astype(np.float32) + 0.0, dy + 0.0)          # one child per window carries it


# ---------------------------------------------------------------------------------------------------- encoder pooling
@pytest.mark.parametrize("G", CELLS_G)
def test_cells_bit_exact_at_every_boundary(dev, G):
    v = R.cell_boundary_coords(G)
    T = len(v)
    i = np.arange(T)
    cloud = np.stack([np.stack([v[(i + 3 * b) % T], v[(7 * i + 3 + b) % T], v[(13 * i + 5 + 2 * b) % T]], -1) for b in range(2)]).astype(np.float32)
    cell_ref, half_ref = R.cells_ref(cloud, G)
    assert cell_ref.min() >= 0 and cell_ref.max() < G ** 3
    cd = _in(cloud, dev)
    for with_half in (False, True):
        c, h = IOut((2, T), dev, torch.int32, fill=ISENT), Out((2, T, 3), dev)
        _call("sfmi_cells_f32", cd, c.v, h.v if with_half else None, 2, T, G)
        assert np.array_equal(c.np(f"cells G{G}"), cell_ref)
        if with_half:
            assert _same_bits(h.np(f"cells G{G} p_half"), half_ref)
        else:
            h.untouched(f"cells G{G} without p_half")


@pytest.mark.parametrize("C", CELL_POOL_C)
def test_cell_max_forward_exact_in_a_column_window(dev, C):
    for seed in CELL_POOL_SEEDS:
        cs = R.cell_pool_case(C, seed)
        net, cell, ncell = cs["net"], cs["cell"], cs["ncell"]
        B, T, _ = net.shape
        co, ldo = 3, C + 5
        keys, o = IOut((B, ncell, C), dev, torch.int32, fill=R.INT_MIN), Out((B * T, ldo), dev)
        _call("sfmi_cell_max_f32", _in(net, dev), _in(cell, dev, torch.int32), keys.v, o.v, B, T, ncell, C, ldo, co)
        kref, pref = R.cell_max_ref(net, cell, ncell)
        assert np.array_equal(keys.np("cell_max keys"), kref)                       # empty cells keep INT_MIN
        got = o.np("cell_max", written=False)
        assert _same_bits(got[:, co:co + C], pref.reshape(B * T, C))
        side = np.concatenate([_bits(got[:, :co]), _bits(got[:, co + C:])], 1)
        assert (side == SENT).all(), "cell_max wrote outside its column window"


@pytest.mark.parametrize("C", CELL_POOL_C)
@pytest.mark.parametrize("accumulate", (0, 1))
def test_cell_max_backward_routes_each_cell_gradient_to_one_point(dev, C, accumulate):
    """The tie contract.  Exact copies of rows, ties between distinct points in single channels and three-way ties: the gradient of a
    (cell, channel) arrives at the lowest-indexed point that attains the maximum and nowhere else, and the sum over the cell's points is
    the cell's gradient (conservation).  Read from the kernel text of the parent commit, not from a run of it: its cell_max_bwd_kernel
    gave `acc[g]` to every point with f2key(net) == keys[g], so a cell with n tied points summed to n times its gradient and this test's
    per-point and conservation assertions both fail there (tests/test_train_vqdif_ref_cpu.py states that on the CPU)."""
    for seed in CELL_POOL_SEEDS:
        cs = R.cell_pool_case(C, seed)
        net, cell, ncell = cs["net"], cs["cell"], cs["ncell"]
        B, T, _ = net.shape
        rs = _rs(seed + C)
        keys, _ = R.cell_max_ref(net, cell, ncell)
        acc = R.to_fix(rs.randn(B, ncell, C).astype(np.float32) * 3)
        ldd = C + 3
        prev = rs.randn(B * T, ldd).astype(np.float32) if accumulate else None
        o = Out((B * T, ldd), dev, prev)
        win = IOut((B, ncell, C), dev, torch.int32, fill=12345)                      # scratch: stale contents must not matter
        ins = (_in(net, dev), _in(keys, dev, torch.int32), _in(acc, dev, torch.int64), _in(cell, dev, torch.int32))
        _call("sfmi_cell_max_bwd_ws_f32", *ins, win.v, o.v, B, T, ncell, C, ldd, accumulate)
        got = o.np("cell_max_bwd", written=False)
        o2 = Out((B * T, ldd), dev, prev)                                            # the entry that finds its own scratch: the same bits
        _call("sfmi_cell_max_bwd_f32", *ins, o2.v, B, T, ncell, C, ldd, accumulate)
        assert np.array_equal(_bits(o2.np("cell_max_bwd (own scratch)", written=False)), _bits(got))
        ref = R.cell_max_bwd_ref(net, keys, acc, cell, None if prev is None else prev[:, :C].reshape(B, T, C))
        assert _same_bits(got[:, :C], ref.reshape(B * T, C)), "a tied point received (or the winner missed) the cell's gradient"
        pad = _bits(got[:, C:])
        assert (pad == (_bits(prev[:, C:]) if accumulate else SENT)).all(), "cell_max_bwd wrote beyond column C of a row"
        wref, wgot = R.cell_winner(net, keys, cell), win.np("cell_max_bwd winners")
        occ = wref != R.INT_MAX
        assert np.array_equal(wgot[occ], wref[occ]) and (wgot[~occ] == 12345).all()
        # conservation per (cell, channel)
        d = got[:, :C].reshape(B, T, C).astype(np.float64) - (0 if prev is None else prev[:, :C].reshape(B, T, C).astype(np.float64))
        g = R.fix_to_float(acc).astype(np.float64)
        for b in range(B):
            tot = np.zeros((ncell, C))
            np.add.at(tot, cell[b], d[b])
            o_ = np.bincount(cell[b], minlength=ncell) > 0
            tol = 0 if not accumulate else 4 * U * (np.abs(g[b][o_]) + np.abs(prev).max()) * T
            assert (np.abs(tot[o_] - g[b][o_]) <= tol).all(), "the gradient of a cell is not conserved"
            assert not tot[~o_].any()


def _scatter_case(form, T, C, scale, seed):
    rs = _rs(seed)
    B = 2
    cell = np.zeros((B, T), np.int32) + 5 if form == "one_cell" else np.stack([rs.permutation(NCELL)[:T] for _ in range(B)]).astype(np.int32)
    return (rs.randn(B, T, C) * scale).astype(np.float32), cell


@pytest.mark.parametrize("form,T", SCATTER_FORMS)
def test_fixed_point_scatter_add_mean_and_mean_backward(dev, form, T):
    B = 2
    for C in SCATTER_C:
        for scale in SCATTER_SCALES:
            src, cell = _scatter_case(form, T, C, scale, T + C)
            acc_ref, cnt_ref, s, sa = R.cell_scatter_ref(src, cell, NCELL)
            celld = _in(cell, dev, torch.int32)
            # the concat form: a column window of wider rows, no counts
            cs_, lds = 3, C + 5
            wide = np.full((B, T, lds), np.nan, np.float32)
            wide[..., cs_:cs_ + C] = src
            a = IOut((B, NCELL, C), dev, torch.int64)
            _call("sfmi_cell_scatter_add_f32", _in(wide, dev), celld, a.v, None, B, T, NCELL, C, lds, cs_)
            assert np.array_equal(a.np("scatter_add window"), acc_ref), (form, C, scale)
            # the plain form with counts: three runs, then the points in another order
            first = None
            for run in range(4):
                p = np.arange(T) if run < 3 else _rs(run).permutation(T)
                a, n = IOut((B, NCELL, C), dev, torch.int64), IOut((B, NCELL), dev, torch.int32)
                _call("sfmi_cell_scatter_add_f32", _in(src[:, p], dev), _in(cell[:, p], dev, torch.int32), a.v, n.v, B, T, NCELL, C, C, 0)
                got, gn = a.np("scatter_add"), n.np("scatter_add count")
                assert np.array_equal(got, acc_ref) and np.array_equal(gn, cnt_ref), (form, C, scale, run)    # == the integer sum, exactly
                first = got if first is None else first
                assert np.array_equal(got, first)
            conv = Out((B, NCELL, C), dev)                                                                    # the device's conversion, as the trainer uses it
            _call("sfmi_fixed_to_float_f32", a.v, conv.v, B * NCELL * C, 0)
            assert _same_bits(conv.np("fixed_to_float"), R.fix_to_float(acc_ref))
            assert _note("scatter_add", R.ratio(conv.np("fixed_to_float"), s, R.fix_bound(cnt_ref[..., None], s))) <= 1.0
            # scatter-mean over every cell (zeros where empty) and its backward
            g = Out((B, NCELL, C), dev)
            _call("sfmi_cell_mean_f32", a.v, n.v, g.v, B, NCELL, C)
            m, bnd = R.cell_mean_ref(s, cnt_ref)
            gm = g.np("cell_mean")
            assert not gm[cnt_ref == 0].any()
            assert _note("cell_mean", R.ratio(gm, m, bnd)) <= 1.0, (form, C, scale)
            dgrid = (_rs(C).randn(B, NCELL, C) * scale).astype(np.float32)
            d = Out((B * T, C), dev)
            _call("sfmi_cell_mean_bwd_f32", _in(dgrid, dev), n.v, celld, d.v, B, T, NCELL, C)
            ref, bnd = R.cell_mean_bwd_ref(dgrid, cnt_ref, cell)
            assert _note("cell_mean_bwd", R.ratio(d.np("cell_mean_bwd").reshape(B, T, C), ref, bnd)) <= 1.0, (form, C, scale)
    _report("scatter_add", "cell_mean", "cell_mean_bwd")


# ---------------------------------------------------------------------------------------------------- trilinear sampling
@pytest.mark.parametrize("G,C,N", TRI_CASES)
def test_trilinear_forward_and_fixed_point_backward(dev, G, C, N):
    B = 2
    xyz = R.tri_points(G, N, G + C + N)
    gen = torch.Generator(device=dev).manual_seed(G * C + N)
    grid_d = torch.full((B * G ** 3 * C + 2 * GUARD,), float("nan"), device=dev)
    grid_v = grid_d[GUARD:-GUARD].view(B, G ** 3, C)
    grid_v.copy_(torch.randn(B, G ** 3, C, device=dev, generator=gen))
    xd = _in(xyz, dev)
    o = Out((B, N, C), dev)
    _call("sfmi_trilinear_cl_f32", xd, grid_v, o.v, B, N, G, C)
    ref, bnd = R.trilinear_ref(xyz, grid_v.cpu().numpy(), G)
    assert _note("trilinear", R.ratio(o.np(f"trilinear {G, C, N}"), ref, bnd)) <= 1.0
    del grid_d, grid_v
    base = _rs(N + C).randn(B, N, C)
    for scale in SCATTER_SCALES:
        dout = (base * scale).astype(np.float32)
        s, b_acc, _ = R.trilinear_bwd_ref(xyz, dout, G)
        first = None
        for run in range(4):
            p = np.arange(N) if run < 3 else _rs(run).permutation(N)
            acc = IOut((B, G ** 3, C), dev, torch.int64)
            _call("sfmi_trilinear_bwd_cl_f32", _in(xyz[:, p], dev), _in(dout[:, p], dev), acc.v, B, N, G, C)
            if first is None:
                first = acc
                got = acc.np(f"trilinear_bwd {G, C, N}").astype(np.float64) / R.FIX
                assert _note("trilinear_bwd", R.ratio(got, s, b_acc)) <= 1.0, (G, C, N, scale)
                # the weights of a point sum to one: column sums of the gradient == column sums of dout
                cs_, cd = got.sum(1), dout.astype(np.float64).sum(1)
                assert (np.abs(cs_ - cd) <= b_acc.sum(1) + 1e-15 * np.abs(dout).sum(1)).all(), (G, C, N, scale)
            else:
                assert torch.equal(acc.buf, first.buf), f"trilinear_bwd {G, C, N} run {run}: the accumulator depends on the order"
    _report("trilinear", "trilinear_bwd")


# ---------------------------------------------------------------------------------------------------- loss, quantizer
def bce_inputs(n, offset):
    combos = [(x, y) for x in BCE_LOGITS for y in BCE_LABELS]
    sel = [(combos[(offset + i) % len(combos)]) for i in range(n)]
    return np.array([c[0] for c in sel], np.float32), np.array([c[1] for c in sel], np.float32)


@pytest.mark.parametrize("n", BCE_N)
def test_bce_with_logits_at_the_edges_of_expf(dev, n):
    for offset in (range(len(BCE_LOGITS) * len(BCE_LABELS)) if n == 1 else (0, 17)):
        x, y = bce_inputs(n, offset)
        scale = 1.0 / n if offset % 2 == 0 else 0.37
        lo, dx = Out((n,), dev), Out((n,), dev)
        _call("sfmi_bce_logits_f32", _in(x, dev), _in(y, dev), lo.v, dx.v, n, _L().f32(scale))
        gl, gd = lo.np("bce loss"), dx.np("bce dlogits")
        assert np.isfinite(gl).all() and np.isfinite(gd).all(), (n, offset)
        loss, bl, d, bd = R.bce_ref(x, y, scale)
        assert _note("bce loss", R.ratio(gl, loss, bl)) <= 1.0, (n, offset)
        assert _note("bce dlogits", R.ratio(gd, d, bd)) <= 1.0, (n, offset)
    _report("bce loss", "bce dlogits")


@pytest.mark.parametrize("rows,D,K", VQ_STATS_CASES)
def test_vq_stats_exact_integer_sums(dev, rows, D, K):
    rs = _rs(rows + D + K)
    x = rs.randn(rows, D).astype(np.float32)
    for form in ("one_code", "spread"):
        idx = np.full(rows, K - 1, np.int32) if form == "one_code" else rs.randint(0, K, size=rows).astype(np.int32)
        sums, cnt = IOut((K, D), dev, torch.int64), IOut((K,), dev, torch.int32)
        _call("sfmi_vq_stats_f32", _in(x, dev), _in(idx, dev, torch.int32), sums.v, cnt.v, rows, D)
        sref, cref = R.vq_stats_ref(x, idx, K)
        assert np.array_equal(sums.np("vq_stats sums"), sref) and np.array_equal(cnt.np("vq_stats counts"), cref), (form, rows, D, K)


@pytest.mark.parametrize("K,D", VQ_EMA_CASES)
def test_vq_ema_update_in_place(dev, K, D):
    rs = _rs(K + D)
    N, z = (rs.rand(K) * 5 + 0.01).astype(np.float32), rs.randn(K, D).astype(np.float32)
    counts = (rs.randint(0, 6, size=K) * (rs.rand(K) > 0.4)).astype(np.float32)         # codes nobody chose: count 0, sum 0
    if K > 1:
        counts[0] = 0
    sums = (rs.randn(K, D) * counts[:, None]).astype(np.float32)
    Nd, zd, ed = Out((K,), dev, N), Out((K, D), dev, z), Out((K, D), dev)
    _call("sfmi_vq_ema_update_f32", Nd.v, zd.v, ed.v, _in(counts, dev), _in(sums, dev), K, D, _L().f32(VQ_GAMMA), _L().f32(VQ_EPS))
    ref = R.vq_ema_ref(N, z, counts, sums, VQ_GAMMA, VQ_EPS)
    for name, o in (("N", Nd), ("z", zd), ("emb", ed)):
        assert _note("vq_ema " + name, R.ratio(o.np(f"vq_ema {name} K{K} D{D}"), *ref[name])) <= 1.0, (name, K, D)
    _report("vq_ema N", "vq_ema z", "vq_ema emb")


# ---------------------------------------------------------------------------------------------------- conv weight gradient
@pytest.mark.parametrize("case", WG_CASES, ids=[c[0] for c in WG_CASES])
def test_conv3d_wgrad_every_slice_written_and_reduced(dev, case):
    name, B, Di, Hi, Wi, Cin, Cout, KS, st, pad, ldy, ldx, form = case
    rows = R.wgrad_rows(B, Di, Hi, Wi, KS, st, pad)
    rs = _rs(rows + Cin + Cout)
    dy, x = rs.randn(rows, ldy).astype(np.float32), rs.randn(B * Di * Hi * Wi, ldx).astype(np.float32)
    if form == "fc_out":
        dy[:, 1:] = 0
    if form == "nan_pad":
        dy[:, Cout:], x[:, Cin:] = np.nan, np.nan
    dW, sa = R.wgrad_ref(dy, x, B, Di, Hi, Wi, Cin, Cout, KS, st, pad)
    dyd, xd = _in(dy, dev), _in(x, dev)
    n = KS ** 3 * Cout * Cin
    for ns in wg_nsplits(case):
        part = Out((ns, n), dev)
        _call("sfmi_conv3d_wgrad_f32", dyd, xd, part.v, B, Di, Hi, Wi, Cin, Cout, KS, st, pad, ldy, ldx, ns)
        p = part.check(f"wgrad {name} nsplit {ns}")                                  # every element of (nsplit, taps, Cout, Cin) is written
        rps = R.rows_per_split(rows, ns)
        for s in range(ns):
            if s * rps >= rows:
                assert not bool(p[s].any()), f"wgrad {name}: the empty slice {s} of {ns} is not zero"
        g = Out((n,), dev)
        _call("sfmi_colsum_f32", p, g.v, ns, n, n, 0)
        assert _note("wgrad", R.ratio(g.np(f"wgrad {name} colsum").reshape(dW.shape), dW, R.wgrad_bound(sa, rows, ns))) <= 1.0, (name, ns)
    _report("wgrad")


# ---------------------------------------------------------------------------------------------------- the step on a cloud with copies
def redrawn_cloud(Xbd):
    """the data loader's draw (data.py: np.random.choice(..., boundary_N, replace=True)): about a third of the rows become exact copies"""
    T = Xbd.shape[1]
    return np.ascontiguousarray(Xbd[:, np.random.RandomState(REDRAW_SEED).choice(T, T, replace=True)])


def test_step_on_a_cloud_drawn_with_replacement_matches_the_oracle(dev):
    """Copies have identical features, so the oracle's even split (torch amax) and the reference's single arg-max give the same parameter
    gradients; with the ReLU masks and pool indices of our forward frozen, every tensor must agree as tightly as on a cloud without
    copies.  Under the parent's rule (every tied point takes the whole gradient) the encoder's tensors are off by O(1)."""
    from oracle import vqdif_oracle as VO, vqdif_train_oracle as TO
    from shapeformer_amd import weights as W
    from shapeformer_amd.train_vqdif import VQDIFTrainer
    from test_train_vqdif_gpu import _to_ref_layout
    G = np.load(os.path.join(HERE, "golden", "vqdif_train.npz"))
    Xbd = redrawn_cloud(G["Xbd"])
    assert len(np.unique(Xbd[0], axis=0)) < 0.7 * Xbd.shape[1]
    sd = W.make_state_dict(W.vqdif_spec(16))
    tr = VQDIFTrainer(sd, res=16, device=dev, beta=float(G["beta"]))
    tr.relu_tap, tr.pool_tap = [], []
    out = tr.loss_and_grad(Xbd, G["Xtg"], G["Ytg"])
    masks, pools, tr.relu_tap, tr.pool_tap = tr.relu_tap, tr.pool_tap, None, None
    o2, og = TO.loss_and_grads(VO.to_torch_sd(sd), torch.from_numpy(Xbd), torch.from_numpy(G["Xtg"]), torch.from_numpy(G["Ytg"]), float(G["beta"]),
                               relu_masks=masks, pool_index=pools)
    assert abs(float(o2["loss"].detach()) - float(out["loss"])) < 2e-5
    errs = {}
    for k, ref in og.items():
        got = _to_ref_layout(tr, k, tr.g[k])
        ref = ref.numpy().astype(np.float64)
        assert got.shape == ref.shape, k
        errs[k] = float(np.abs(got.astype(np.float64) - ref).max() / (np.abs(ref).max() + 1e-12))
    worst = max(errs, key=errs.get)
    print(f"[step] redrawn cloud, frozen masks: worst max-normalised gradient error {errs[worst]:.2e} ({worst})")
    bad = sorted(((e, k) for k, e in errs.items() if e >= FROZEN_GATE), reverse=True)
    assert not bad, bad[:40]


# ---------------------------------------------------------------------------------------------------- argument checks
def _arg_cases(dev):
    """name -> (valid argument list, {position: bad values}, outputs).  Every pointer is a real buffer large enough for the valid call."""
    f = lambda *s: _in(np.ones(s, np.float32), dev)
    i = lambda *s: _in(np.zeros(s, np.int32), dev, torch.int32)
    O, IO, L = (lambda *s: Out(s, dev)), (lambda dt, *s: IOut(s, dev, dt)), _L()
    c = {}
    o = O(8);              c["sfmi_relu_bwd_f32"] = ([f(8), f(8), o.v, 8], {3: (0, -4, 6)}, [o])
    o = O(8);              c["sfmi_lincomb_f32"] = ([L.f32(1.0), f(8), L.f32(1.0), f(8), o.v, 8], {5: (0, -1)}, [o])
    o = O(2, 3, 4);        c["sfmi_affine2_cl_f32"] = ([f(2, 3, 4), f(2, 3, 4), f(2, 4), f(2, 4), f(2, 4), o.v, 2, 3, 4], {6: (0, -1), 7: (0, -1), 8: (0, -4)}, [o])
    o = O(2, 3, 4);        c["sfmi_affine_cl_f32"] = ([f(2, 3, 4), f(2, 4), f(2, 4), o.v, 2, 3, 4], {4: (0, -1), 5: (0, -1), 6: (0, -4, 3, 2)}, [o])
    o = Out((2, 2, 8, 2), dev, f64=True)
    c["sfmi_chan_dot_stats_f32"] = ([f(2, 3, 8), f(2, 3, 8), o.v, 2, 3, 8, 2], {3: (0, -1), 4: (0, -1), 5: (0, -4, 6, 1028), 6: (0, -1)}, [o])
    o = O(2, 2, 4, 6, 4);  c["sfmi_upsample2_cl_f32"] = ([f(2, 1, 2, 3, 4), o.v, 2, 1, 2, 3, 4], {k: (0, -1) for k in range(2, 7)}, [o])
    o = O(2, 1, 2, 3, 4);  c["sfmi_sumpool2_cl_f32"] = ([f(2, 2, 4, 6, 12), o.v, 2, 1, 2, 3, 12, 4, 4], {2: (0,), 3: (0,), 4: (-1,), 5: (0,), 7: (-4, 9), 8: (0, -4, 12)}, [o])
    o = O(2, 1, 2, 3, 4);  c["sfmi_maxpool2_cl_f32"] = ([f(2, 2, 4, 6, 4), o.v, 2, 1, 2, 3, 4], {2: (0,), 3: (-1,), 4: (0,), 5: (0,), 6: (0, -4, 2)}, [o])
    o = O(2, 2, 4, 6, 4);  c["sfmi_maxpool2_bwd_cl_f32"] = ([f(2, 2, 4, 6, 4), f(2, 1, 2, 3, 4), f(2, 1, 2, 3, 4), o.v, 2, 1, 2, 3, 4], {k: (0, -1) for k in range(4, 9)}, [o])
    o = O(2, 2, 4, 6, 12); c["sfmi_upcat_cl_f32"] = ([f(2, 2, 4, 6, 8), f(2, 1, 2, 3, 4), o.v, 2, 2, 4, 6, 8, 4], {3: (0,), 4: (0, 1), 5: (-2, 3), 6: (0, 5), 7: (0, 6, -8), 8: (0, 2)}, [o])
    o, h = IO(torch.int32, 2, 5), O(2, 5, 3)
    c["sfmi_cells_f32"] = ([f(2, 5, 3), o.v, h.v, 2, 5, 2], {3: (0, -1), 4: (0, -1), 5: (0, -2)}, [o, h])
    k, o = IO(torch.int32, 2, 8, 4), O(10, 9)
    c["sfmi_cell_max_f32"] = ([f(2, 5, 4), i(2, 5), k.v, o.v, 2, 5, 8, 4, 9, 3], {4: (0,), 5: (0,), 6: (0, -8), 7: (0, -4), 8: (6, 4, 0), 9: (-1, 6)}, [k, o])
    a, n = IO(torch.int64, 2, 8, 4), IO(torch.int32, 2, 8)
    c["sfmi_cell_scatter_add_f32"] = ([f(2, 5, 9), i(2, 5), a.v, n.v, 2, 5, 8, 4, 9, 3], {4: (0,), 5: (-1,), 6: (0,), 7: (0,), 8: (6, 0), 9: (-1, 6)}, [a, n])
    w, o = IO(torch.int32, 2, 8, 4), O(10, 6)
    c["sfmi_cell_max_bwd_ws_f32"] = ([f(2, 5, 4), i(2, 8, 4), _in(np.zeros((2, 8, 4), np.int64), dev, torch.int64), i(2, 5), w.v, o.v, 2, 5, 8, 4, 6, 0],
                                     {6: (0,), 7: (0,), 8: (0,), 9: (0, -4), 10: (3, 0, -6)}, [w, o])
    o = O(10, 6)
    c["sfmi_cell_max_bwd_f32"] = ([f(2, 5, 4), i(2, 8, 4), _in(np.zeros((2, 8, 4), np.int64), dev, torch.int64), i(2, 5), o.v, 2, 5, 8, 4, 6, 0],
                                  {5: (0,), 6: (0,), 7: (0, -8), 8: (0, -4), 9: (3, 0, -6)}, [o])
    o = O(2, 8, 4);        c["sfmi_cell_mean_f32"] = ([_in(np.zeros((2, 8, 4), np.int64), dev, torch.int64), i(2, 8), o.v, 2, 8, 4], {3: (0,), 4: (0, -8), 5: (0, -4)}, [o])
    o = O(10, 4);          c["sfmi_cell_mean_bwd_f32"] = ([f(2, 8, 4), i(2, 8) + 1, i(2, 5), o.v, 2, 5, 8, 4], {4: (0,), 5: (0,), 6: (0,), 7: (0, -4)}, [o])
    o = O(2, 5, 4);        c["sfmi_trilinear_cl_f32"] = ([f(2, 5, 3) * 0.3, f(2, 8, 4), o.v, 2, 5, 2, 4], {3: (0, -1), 4: (0, -5), 5: (0, -2), 6: (0, -4)}, [o])
    a = IO(torch.int64, 2, 8, 4)
    c["sfmi_trilinear_bwd_cl_f32"] = ([f(2, 5, 3) * 0.3, f(2, 5, 4), a.v, 2, 5, 2, 4], {3: (0, -1), 4: (0, -5), 5: (0, -2), 6: (0, -4)}, [a])
    o, d = O(8), O(8);     c["sfmi_bce_logits_f32"] = ([f(8), f(8), o.v, d.v, 8, L.f32(0.125)], {4: (0, -8)}, [o, d])
    a, n = IO(torch.int64, 5, 4), IO(torch.int32, 5)
    c["sfmi_vq_stats_f32"] = ([f(6, 4), i(6), a.v, n.v, 6, 4], {4: (0, -6), 5: (0, -4)}, [a, n])
    N, z, e = Out((5,), dev), Out((5, 4), dev), Out((5, 4), dev)
    c["sfmi_vq_ema_update_f32"] = ([N.v, z.v, e.v, f(5), f(5, 4), 5, 4, L.f32(0.99), L.f32(1e-7)], {5: (0, -5), 6: (0, -4)}, [N, z, e])
    o = O(2, 27 * 8 * 4)
    c["sfmi_conv3d_wgrad_f32"] = ([f(2 * 3 * 4 * 5, 10), f(2 * 3 * 4 * 5, 6), o.v, 2, 3, 4, 5, 4, 8, 3, 1, 1, 10, 6, 2],
                                  {3: (0,), 4: (0,), 5: (-4,), 6: (0,), 7: (0, -4), 8: (0, -8), 9: (0, -3, 6, 7), 10: (0, -1), 11: (-1,), 12: (7, 0), 13: (3, 0), 14: (0, -2)}, [o])
    return c


ARG_CHECKED = ("sfmi_relu_bwd_f32", "sfmi_lincomb_f32", "sfmi_affine2_cl_f32", "sfmi_affine_cl_f32", "sfmi_chan_dot_stats_f32", "sfmi_upsample2_cl_f32",
               "sfmi_sumpool2_cl_f32", "sfmi_maxpool2_cl_f32", "sfmi_maxpool2_bwd_cl_f32", "sfmi_upcat_cl_f32", "sfmi_cells_f32", "sfmi_cell_max_f32",
               "sfmi_cell_scatter_add_f32", "sfmi_cell_max_bwd_f32", "sfmi_cell_max_bwd_ws_f32", "sfmi_cell_mean_f32", "sfmi_cell_mean_bwd_f32", "sfmi_trilinear_cl_f32",
               "sfmi_trilinear_bwd_cl_f32", "sfmi_bce_logits_f32", "sfmi_vq_stats_f32", "sfmi_vq_ema_update_f32", "sfmi_conv3d_wgrad_f32")


def test_argument_checks_refuse_before_any_launch(dev):
    """non-positive counts and extents, C % 4 where a kernel uses 16-byte accesses, short leading dimensions, negative offsets and pads, a
    kernel larger than the padded input, G < 1, K <= 0: SFMI_EINVAL by return value, and the outputs keep their fill"""
    cases = _arg_cases(dev)
    assert sorted(cases) == sorted(ARG_CHECKED)
    for name, (args, bad, outs) in cases.items():
        for pos, values in bad.items():
            for v in values:
                a = list(args)
                a[pos] = v
                assert _rc(name, *a) == EINVAL, f"{name}: argument {pos} = {v} was accepted"
        torch.cuda.synchronize()
        for o in outs:
            o.untouched(name)
        assert _rc(name, *args) == 0, f"{name}: the valid call was refused"
        torch.cuda.synchronize()
