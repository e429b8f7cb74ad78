"""Every entry of csrc/train.hip through the C ABI against float64 (tests/train_ref.py: references, derived per-element bounds, mirrors
of the launch rules), at every launch form: transpose, the three column-sum families, GELU, the LayerNorm backward in its wave and
block forms with the fused / separate dropout, cross entropy, the 2^-32 fixed-point embedding scatter, dropout, AdamW in its five
entries, the training attention forward and backward with explicit dropout masks, one training step at the product's width
(n_embd 1024, 16 heads) against the float64 oracle, and the argument checks (by return value).  Every output sits NaN-filled between
sentinel bands; every `[ratio]` line (pytest -s) is the largest error / bound of a family.  The case tables below are plain data:
tests/test_train_ref_cpu.py imports them and proves, from the mirrors, that they reach every form.

Measured on one MI355X (largest error / bound per family): colsum 0.55, colsum_ws 0.12, col_reduce 0.15, gelu 0.49, gelu_bwd 0.42,
LayerNorm rows wave 0.15 / block 0.19 (stats 0.19 / 0.22), three-launch form 0.24, cross entropy loss 0.61 / dlogits 0.62, scatter 0.99
(one row on an element: the rounding to the 2^-32 grid IS the bound), AdamW p 0.54 / m 0.61 / v 0.63, attention forward y 0.03 / lse 0.03,
delta 0.08, dqkv 0.018 in both backward forms (the [ATTN] bound is dominated by its worst-case exponent terms and still keeps tenfold
teeth: test_train_ref_cpu.py).  The step at width 1024: every tensor within 1.6 x the oracle's own fp32 error (eval: L0.bfc1 1.45,
pos_emb 1.40; train mode: L0.bproj 1.61).  Every bit-identity claim held: dx2 == sfmi_dropout_f32(dx) on both D paths, seed by value ==
seed from device memory (LayerNorm, dropout, attention forward and backward), AdamW vector == scalar path, bc_dev == launch-time form,
pflat == p (also aliasing g), three col_reduce / scatter runs, sfmi_ce_fwd_bwd_f32's loss == sfmi_ce_rows_f32.  No kernel defect was
found; the host defects are the argument checks at the end of this file.  The file runs in 6 s."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import train_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
SENT = 0x7FC0DEAD          # NaN bit pattern of every "must stay untouched" float
GUARD = 256                # band elements on either side of every buffer
U = R.U

# ---------------------------------------------------------------------------------------------------- the case tables
TRANSPOSE_CASES = [(1, 1), (31, 33), (32, 32), (33, 31), (499, 1024), (1024, 260)]
COLSUM_M, COLSUM_N = (1, 3, 4, 5, 8), (1, 63, 64, 65, 24 * 128)
COLSUM_WS_CASES = [(15, 64), (16, 64), (17, 65), (33, 64), (97, 132), (2050, 64), (3000, 4096)]
GELU_N = (1, 255, 256, 257, 4099)
LN_D_WAVE, LN_D_BLOCK, LN_M = (128, 256, 512, 1024), (64, 192, 320, 2048), (1, 3, 4, 5, 499)
LN_FULL_CASES = [(5, 128), (499, 1024), (2100, 192)]
CR_M = (1, 15, 16, 17, 1024, 1025, 1537, 8200)
CR_NJOBS = (1, 3, 8)
CR_JOBS = [(3072, 3072, 0), (64, 72, 1), (1024, 1024, 1), (4, 4, 0), (60, 60, 1), (68, 68, 0), (64, 64, 0), (1024, 1024, 1)]   # (N, ld, kind)
CE_VLD, CE_L, CE_B = [(1, 4), (255, 256), (256, 256), (257, 260), (4097, 4128)], (1, 7, 64), (1, 3)
SCATTER_D, SCATTER_SCALES, SCATTER_ROWS = (4, 128, 1024), (1.0, 1e-4, 1e-8), 37
DROPOUT_N, DROPOUT_P = (4, 1028, 4 * 65537), (0.0, 0.1, 0.9)
ADAM_LENS, ADAM_WD = (1, 7, 1024, 4100, 40000), (0.0, 0.01, 0.01, 0.0, 0.01)
ADAM_FOFF = {"aligned": (0, 4, 12, 1036, 5136), "offset": (0, 5, 12, 1038, 5140)}
ADAM_STEPS = (1, 2, 1000, 100000)
ADAM_HP = dict(lr=1e-3, b1=0.9, b2=0.95, eps=1e-8)
ADAM_GSCALE = (1.0, 0.0, 1e-6, 1e-3, 1.0)      # gradient magnitudes per tensor; tensor 1: g = m = v = 0
ATTN_CASES = [(1, 1, 1), (1, 15, 2), (2, 31, 1), (1, 32, 2), (1, 33, 4), (2, 63, 2), (1, 64, 16), (1, 65, 2), (1, 97, 4), (1, 129, 16), (3, 129, 16)]
ATTN_P = (0.0, 0.2)
STEP_KW = dict(n_embd=1024, n_head=16, n_layers=(1, 1), block_size=96)
STEP_PDROP = (0.1, 0.15, 0.2)
GATE_X = 8.0               # per-tensor gate of a whole step: 8 x the error of the oracle's own fp32 CPU autograd (floor 8 U)


def adam_chunks(kind):
    """(ctensor, coff, clen) of a chunk table over ADAM_LENS.  'vector': 4096-element chunks (lengths and offsets multiples of 4 wherever
    the tensor allows); 'scalar': lengths 1, 3, 255, 1025 in turn; 'partial': only [len / 4, len / 2) of every tensor."""
    ct, co, cl = [], [], []
    for t, n in enumerate(ADAM_LENS):
        if kind == "partial":
            a, b = n // 4, max(n // 2, n // 4 + 1)
            ct, co, cl = ct + [t], co + [a], cl + [b - a]
            continue
        o, i = 0, 0
        while o < n:
            c = min(4096 if kind == "vector" else (1, 3, 255, 1025)[i % 4], n - o)
            ct, co, cl = ct + [t], co + [o], cl + [c]
            o, i = o + c, i + 1
    return ct, co, cl


def adam_chunk_is_vector(layout, t, off, n):
    """the alignment rule of adamw_multi_kernel: flat offset, tensor offset and length all multiples of 4"""
    return ((ADAM_FOFF[layout][t] + off) | off | n) & 3 == 0


# ---------------------------------------------------------------------------------------------------- plumbing
def _L():
    from shapeformer_amd import _lib as L
    return L


def _call(name, *args):
    L = _L()
    L.check(getattr(L.lib(), name)(*args), name)


def _in(t, dev, dtype=torch.float32):
    """a device copy of t between two NaN (or, for integers, sentinel) bands"""
    t = torch.as_tensor(t)
    n = t.numel()
    fill = float("nan") if dtype.is_floating_point else -0x5EAD
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    buf[GUARD:GUARD + n] = t.reshape(-1).to(dev, dtype)
    return buf[GUARD:GUARD + n].view(t.shape)


class Out:
    """a float output: SENT everywhere, the data view between two guard bands; init: values an accumulating / in-place entry starts from"""

    def __init__(self, shape, dev, init=None):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        self.v = self.buf[GUARD:GUARD + self.n].view(shape)
        if init is not None:
            self.v.copy_(torch.as_tensor(init).reshape(shape).to(dev))

    def check(self, what, written=True):
        bits = self.buf.view(torch.int32)
        assert bool((bits[:GUARD] == SENT).all()) and bool((bits[GUARD + self.n:] == SENT).all()), f"{what}: wrote outside the output"
        if written:
            assert not bool((bits[GUARD:GUARD + self.n] == SENT).any()), f"{what}: left part of the output unwritten"
        return self.v

    def np(self, what, written=True):
        return self.check(what, written).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32) if isinstance(a, np.ndarray) else a.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b))) if torch.is_tensor(a) else bool(np.array_equal(_bits(a), _bits(b)))


def _sync():
    torch.cuda.synchronize()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


WORST = {}


def _note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def _report(family):
    print(f"[ratio] {family}: largest error / bound {WORST.get(family, 0.0):.3f}")


def _u32(seed, dev):
    """the 32-bit seed word in device memory"""
    return torch.tensor([seed if seed < 2 ** 31 else seed - 2 ** 32], dtype=torch.int32, device=dev)


# ---------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("Rr,C", TRANSPOSE_CASES)
def test_transpose_exact_with_zero_fill(dev, Rr, C):
    ldin = C + 3
    x = torch.randn(Rr, ldin, generator=_gen(Rr * 7 + C))
    x[:, C:] = float("nan")                                       # never read: a NaN would show in the output
    xd = _in(x, dev)
    for Rpad in sorted({Rr, Rr + 1, (Rr + 15) // 16 * 16}):
        o = Out((C, Rpad), dev)
        _call("sfmi_transpose_f32", xd.data_ptr(), o.v.data_ptr(), Rr, C, ldin, Rpad, _L().stream_ptr())
        _sync()
        assert _same_bits(o.np(f"transpose {Rr}x{C} Rpad {Rpad}"), R.transpose_ref(x[:, :C].numpy(), Rpad))


# ---------------------------------------------------------------------------------------------------- column sums
@pytest.mark.parametrize("N", COLSUM_N)
def test_colsum_with_row_stride_and_column_offset(dev, N):
    """the pos-emb form: M rows of stride ld = Lq * D, a window of N columns at a column offset"""
    c0, ld = 3, 2 * N + 5
    for M in COLSUM_M:
        x = torch.randn(M, ld, generator=_gen(M * 100 + N))
        xd = _in(x, dev)
        a = x[:, c0:c0 + N].numpy()
        for acc in (0, 1):
            prev = torch.randn(N, generator=_gen(N + acc)) if acc else None
            o = Out((N,), dev, prev)
            _call("sfmi_colsum_f32", xd.data_ptr() + 4 * c0, o.v.data_ptr(), M, N, ld, acc, _L().stream_ptr())
            _sync()
            s, b = R.colsum_ref(a, R.colsum_depth("plain", M), prev)
            assert _note("colsum", R.ratio(o.np(f"colsum M{M} N{N}"), s, b)) <= 1.0, (M, N, acc)
    _report("colsum")


@pytest.mark.parametrize("M,N", COLSUM_WS_CASES)
def test_colsum_two_stage(dev, M, N):
    L = _L()
    ld = N + 4
    x = torch.randn(M, ld, generator=_gen(M + N))
    x[:, N:] = float("nan")
    xd = _in(x, dev)
    RS = int(L.lib().sfmi_colsum_slices(M, N))
    assert RS == R.colsum_slices(M, N)
    for acc in (0, 1):
        prev = torch.randn(N, generator=_gen(N + acc)) if acc else None
        o, scr = Out((N,), dev, prev), Out((RS * N,), dev)
        _call("sfmi_colsum_ws_f32", xd.data_ptr(), o.v.data_ptr(), M, N, ld, acc, scr.v.data_ptr(), L.stream_ptr())
        _sync()
        scr.check(f"colsum_ws scratch {M}x{N}")
        s, b = R.colsum_ref(x[:, :N].numpy(), R.colsum_depth("ws", M, N), prev)
        assert _note("colsum_ws", R.ratio(o.np(f"colsum_ws {M}x{N}"), s, b)) <= 1.0, (M, N, acc)
    _report("colsum_ws")


@pytest.fixture(scope="module")
def cr_data(dev):
    """operands of the eight CR_JOBS at the largest M, made once on the device: (a, x, stats) per job; smaller M use the first rows"""
    Mx = max(CR_M)
    g = torch.Generator(device=dev).manual_seed(11)              # its own generator: the global one stays as the other tests expect it
    out = []
    for N, ld, kind in CR_JOBS:
        a = torch.randn(Mx, ld, device=dev, generator=g)
        x = torch.randn(Mx, ld, device=dev, generator=g) + 3.0 if kind else None
        st = torch.stack([torch.randn(Mx, device=dev, generator=g) + 3.0, torch.rand(Mx, device=dev, generator=g) + 0.5], 1).contiguous() if kind else None
        if ld > N:
            a[:, N:] = float("nan")
            x[:, N:] = float("nan")
        out.append((a, x, st))
    return out


@pytest.mark.parametrize("M", CR_M)
def test_col_reduce_every_slice_count_and_job_mix(dev, cr_data, M):
    L = _L()
    lib = L.lib()
    RS = int(lib.sfmi_col_reduce_slices(M))
    assert RS == R.col_reduce_slices(M)
    n = R.colsum_depth("col_reduce", M)
    # float64 sums on the device (exact enough), once per M
    ref = []
    for (N, ld, kind), (a, x, st) in zip(CR_JOBS, cr_data):
        A = a[:M, :N].double()
        r = dict(s=A.sum(0).cpu().numpy(), sa=A.abs().sum(0).cpu().numpy())
        if kind:
            T = A * (x[:M, :N].double() - st[:M, :1].double()) * st[:M, 1:2].double()
            r.update(g=T.sum(0).cpu().numpy(), ga=T.abs().sum(0).cpu().numpy())
        ref.append(r)
    for nj in CR_NJOBS:
        jobs = CR_JOBS[:nj]
        cols = sum(N for N, _, _ in jobs)
        blocks = sum((N + 63) // 64 for N, _, _ in jobs)
        pf = int(lib.sfmi_col_reduce_part_floats(M, cols))
        part, cnt = Out((max(pf, 1),), dev), torch.zeros(blocks + 2 * GUARD, dtype=torch.int32, device=dev)
        cnt[:GUARD], cnt[GUARD + blocks:] = -0x5EAD, -0x5EAD
        first = None
        for acc, rep in ((0, 0), (0, 1), (0, 2), (1, 0)):
            prevs = [(torch.randn(N, generator=_gen(N + 1)), torch.randn(N, generator=_gen(N + 2))) if acc else (None, None) for N, _, _ in jobs]
            outs = [(Out((N,), dev, prevs[i][0]), Out((N,), dev, prevs[i][1]) if kind else None) for i, (N, _, kind) in enumerate(jobs)]
            pa = lambda seq: np.array([0 if t is None else t.data_ptr() for t in seq], np.uint64)
            kinds, Ns, lds = (np.array(v, np.int32) for v in ([k for _, _, k in jobs], [N for N, _, _ in jobs], [l for _, l, _ in jobs]))
            ap, xp, sp = pa([cr_data[i][0] for i in range(nj)]), pa([cr_data[i][1] for i in range(nj)]), pa([cr_data[i][2] for i in range(nj)])
            op, o2p = pa([o.v for o, _ in outs]), pa([None if o2 is None else o2.v for _, o2 in outs])
            L.check(lib.sfmi_col_reduce_f32(nj, kinds.ctypes.data, ap.ctypes.data, xp.ctypes.data, sp.ctypes.data, op.ctypes.data, o2p.ctypes.data,
                                            Ns.ctypes.data, lds.ctypes.data, M, acc, part.v.data_ptr(), pf, cnt[GUARD:].data_ptr(), blocks, L.stream_ptr()),
                    "col_reduce")
            _sync()
            part.check("col_reduce partials", written=False)
            assert bool((cnt[GUARD:GUARD + blocks] == 0).all()) and bool((cnt[:GUARD] == -0x5EAD).all()) and bool((cnt[GUARD + blocks:] == -0x5EAD).all()), \
                "col_reduce: the ticket counters are not back at zero"
            got = []
            for i, ((N, ld, kind), (o, o2)) in enumerate(zip(jobs, outs)):
                what = f"col_reduce M{M} jobs{nj} job{i} acc{acc}"
                p0, p1 = (None, None) if not acc else (prevs[i][0].double().numpy(), prevs[i][1].double().numpy())
                if kind == 0:
                    s, sa = ref[i]["s"] + (p0 if acc else 0), ref[i]["sa"] + (np.abs(p0) if acc else 0)
                    assert _note("col_reduce", R.ratio(o.np(what), s, R.gamma(n) * sa)) <= 1.0, what
                else:
                    g, ga = ref[i]["g"] + (p0 if acc else 0), ref[i]["ga"] + (np.abs(p0) if acc else 0)
                    s, sa = ref[i]["s"] + (p1 if acc else 0), ref[i]["sa"] + (np.abs(p1) if acc else 0)
                    assert _note("col_reduce", R.ratio(o.np(what + " dgamma"), g, R.gamma(n + 3) * ga)) <= 1.0, what
                    assert _note("col_reduce", R.ratio(o2.np(what + " dbeta"), s, R.gamma(n) * sa)) <= 1.0, what
                got += [o.v.clone()] + ([o2.v.clone()] if kind else [])
            if not acc:
                first = first or got
                assert all(_same_bits(a, b) for a, b in zip(first, got)), f"col_reduce M{M} jobs{nj}: run {rep} differs from run 0"
    _report("col_reduce")


# ---------------------------------------------------------------------------------------------------- GELU
def _gelu_x(n, seed):
    x = (torch.rand(n, generator=_gen(seed)) * 20 - 10)
    sp = torch.tensor([0.0, 1e-30, -1e-30, 40.0, -40.0])
    x[:min(n, 5)] = sp[:min(n, 5)] if n >= 5 else sp[3:3 + n]
    return x


@pytest.mark.parametrize("n", GELU_N)
def test_gelu_forward_and_backward_in_place(dev, n):
    L = _L()
    x, dy = _gelu_x(n, n), torch.randn(n, generator=_gen(n + 1))
    xd = _in(x, dev)
    y, b = R.gelu_ref(x)
    o = Out((n,), dev)
    _call("sfmi_gelu_f32", xd.data_ptr(), o.v.data_ptr(), n, L.stream_ptr())
    o2 = Out((n,), dev, x)
    _call("sfmi_gelu_f32", o2.v.data_ptr(), o2.v.data_ptr(), n, L.stream_ptr())
    _sync()
    assert _note("gelu", R.ratio(o.np("gelu"), y, b)) <= 1.0
    assert _same_bits(o.v, o2.check("gelu in place")), "gelu in place differs"
    dx, bd = R.gelu_bwd_ref(dy, x)
    o3 = Out((n,), dev, dy)                                         # dx aliases dy, as in train.py
    _call("sfmi_gelu_bwd_f32", o3.v.data_ptr(), xd.data_ptr(), o3.v.data_ptr(), n, L.stream_ptr())
    _sync()
    assert _note("gelu_bwd", R.ratio(o3.np("gelu_bwd"), dx, bd)) <= 1.0
    _report("gelu"), _report("gelu_bwd")


# ---------------------------------------------------------------------------------------------------- LayerNorm backward
def ln_inputs(M, D, seed):
    """x = 100 + randn (cancellation in x - mean), row 1 constant (M >= 3), gamma with mixed signs and one zero"""
    g = _gen(seed)
    x = 100.0 + torch.randn(M, D, generator=g)
    if M >= 3:
        x[1] = 37.25
    gam = torch.randn(D, generator=g)
    gam[D // 3] = 0.0
    return x, torch.randn(M, D, generator=g), gam, torch.randn(M, D, generator=g)


@pytest.mark.parametrize("D", LN_D_WAVE + LN_D_BLOCK)
def test_layernorm_backward_rows_every_width(dev, D):
    L = _L()
    lib = L.lib()
    ns = R.ln_sum_depth(D)
    for M in LN_M:
        x, dy, gam, dres = ln_inputs(M, D, M * 10000 + D)
        xd, dyd, gd, rd = (_in(t, dev) for t in (x, dy, gam, dres))
        for use_res in (True, False):
            ref = R.ln_bwd_rows_ref(dy, x, gam, dres if use_res else None, ns)
            dx, st = Out((M, D), dev), Out((M, 2), dev)
            _call("sfmi_layernorm_bwd_rows_f32", dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), rd.data_ptr() if use_res else None, dx.v.data_ptr(),
                  st.v.data_ptr(), M, D, L.stream_ptr())
            _sync()
            what = f"ln rows M{M} D{D} res{int(use_res)}"
            assert _note(f"ln_rows {R.ln_rows_form(D)}", R.ratio(dx.np(what), ref["dx"], ref["b_dx"])) <= 1.0, what
            assert _note(f"ln_stats {R.ln_rows_form(D)}", R.ratio(st.np(what), ref["stats"], ref["b_stats"])) <= 1.0, what
        # the dropped second output (dres absent: dx is the last launch's)
        dx0 = dx.v.clone()
        for p in (0.1, 0.5):
            seed = 0x9E3779B1 ^ (M * D)
            d1, s1, d2 = Out((M, D), dev), Out((M, 2), dev), Out((M, D), dev)
            L.check(lib.sfmi_layernorm_bwd_rows_drop_f32(dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), None, d1.v.data_ptr(), s1.v.data_ptr(), d2.v.data_ptr(),
                                                         p, seed, M, D, L.stream_ptr()), "rows_drop")
            e1, t1, e2 = Out((M, D), dev), Out((M, 2), dev), Out((M, D), dev)
            sd = _u32(seed, dev)
            L.check(lib.sfmi_layernorm_bwd_rows_drop_sd_f32(dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), None, e1.v.data_ptr(), t1.v.data_ptr(), e2.v.data_ptr(),
                                                            p, 12345, sd.data_ptr(), M, D, L.stream_ptr()), "rows_drop_sd")
            dd = Out((M, D), dev)
            _call("sfmi_dropout_f32", d1.v.data_ptr(), dd.v.data_ptr(), M * D, p, seed, L.stream_ptr())
            _sync()
            what = f"ln rows_drop M{M} D{D} p{p}"
            assert _same_bits(d1.check(what), dx0) and _same_bits(s1.check(what), st.v), what + ": dx / stats differ from the plain entry"
            assert _same_bits(e1.check(what), dx0) and _same_bits(e2.check(what), d2.check(what)), what + ": seed from device memory gives other bits"
            assert _same_bits(d2.v, dd.check(what)), what + ": dx2 differs from sfmi_dropout_f32(dx)"
            mul = R.dropout_mul(seed, np.arange(M * D, dtype=np.int64), p).reshape(M, D)
            dxn, got = dx0.cpu().numpy(), d2.v.cpu().numpy()
            assert np.array_equal(got[mul == 0], np.zeros_like(got[mul == 0])), what + ": zero pattern"
            want = dxn * R.inv_keep(p)
            assert bool((np.abs(got - want)[mul != 0] <= np.spacing(np.abs(want))[mul != 0]).all()), what + ": kept elements"
    for f in ("wave", "block"):
        _report(f"ln_rows {f}"), _report(f"ln_stats {f}")


@pytest.mark.parametrize("M,D", LN_FULL_CASES)
def test_layernorm_backward_three_launch_form(dev, M, D):
    """sfmi_layernorm_bwd_f32: the block-per-row kernel at every width, parameter sums in two stages that ACCUMULATE"""
    L = _L()
    lib = L.lib()
    x, dy, gam, dres = ln_inputs(M, D, M + D)
    xd, dyd, gd, rd = (_in(t, dev) for t in (x, dy, gam, dres))
    g0, b0 = torch.randn(D, generator=_gen(1)), torch.randn(D, generator=_gen(2))
    nscr = int(lib.sfmi_layernorm_bwd_scratch_floats(M, D))
    assert nscr == 2 * M + 2 * D * R.colsum_slices(M, D)
    dx, dg, db, scr = Out((M, D), dev), Out((D,), dev, g0), Out((D,), dev, b0), Out((nscr,), dev)
    _call("sfmi_layernorm_bwd_f32", dyd.data_ptr(), xd.data_ptr(), gd.data_ptr(), rd.data_ptr(), dx.v.data_ptr(), dg.v.data_ptr(), db.v.data_ptr(),
          scr.v.data_ptr(), M, D, L.stream_ptr())
    _sync()
    ref = R.ln_bwd_rows_ref(dy, x, gam, dres, -(-D // 256) + 8)
    stats = scr.np("ln scratch")[:2 * M].reshape(M, 2)
    assert _note("ln_full", R.ratio(dx.np("ln dx"), ref["dx"], ref["b_dx"])) <= 1.0
    assert _note("ln_full", R.ratio(stats, ref["stats"], ref["b_stats"])) <= 1.0
    n = R.colsum_depth("ws", M, D)
    s, b = R.colsum_ref(R.ln_param_terms(dy, x, stats), n + 3, g0)
    assert _note("ln_full", R.ratio(dg.np("dgamma"), s, b)) <= 1.0
    s, b = R.colsum_ref(dy.numpy(), n, b0)
    assert _note("ln_full", R.ratio(db.np("dbeta"), s, b)) <= 1.0
    _report("ln_full")


# ---------------------------------------------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("V,ld", CE_VLD)
def test_cross_entropy_forward_backward(dev, V, ld):
    L_ = _L()
    for L in CE_L:
        for B in CE_B:
            M = B * L
            g = _gen(V * 1000 + L * 10 + B)
            z = torch.randn(M, ld, generator=g) * 3
            z[M // 2, :V] = torch.where(torch.rand(V, generator=g) < 0.5, 80.0, -80.0)
            z[:, V:] = float("nan")
            tg = torch.randint(0, V, (M,), generator=g)
            tg[0] = 0
            tg[-1] = V - 1
            zd, td = _in(z, dev), _in(tg, dev, torch.int32)
            scale = 1.0 / (M + 1)                                  # never 1: an omitted scale shows
            for t0 in sorted({0, L - 1}):
                lo, dl, l2 = Out((M,), dev), Out((M, ld), dev), Out((M,), dev)
                _call("sfmi_ce_fwd_bwd_f32", zd.data_ptr(), td.data_ptr(), lo.v.data_ptr(), dl.v.data_ptr(), M, V, ld, L, t0, scale, L_.stream_ptr())
                _call("sfmi_ce_rows_f32", zd.data_ptr(), td.data_ptr(), l2.v.data_ptr(), M, V, ld, L_.stream_ptr())
                _sync()
                what = f"ce V{V} L{L} B{B} t0 {t0}"
                ref = R.ce_ref(z.numpy(), tg.numpy(), V, L, t0, scale)
                gl, gd = lo.np(what), dl.np(what)
                assert _note("ce loss", R.ratio(gl, ref["loss"], ref["b_loss"])) <= 1.0, what
                assert _note("ce dlogits", R.ratio(gd, ref["dlogits"], ref["b_dl"])) <= 1.0, what
                act = ref["active"]
                assert not gd[~act].any() and not gl[~act].any() and not gd[:, V:].any(), what + ": inactive rows / pad columns must be zero"
                assert bool((np.abs(gd[act].astype(np.float64).sum(1)) <= ref["b_dl"][act].sum(1)).all()), what + ": an active row does not sum to 0"
                # sfmi_ce_rows_f32 (same arithmetic, no gradient) on the active rows: both are within the bound of the exact loss
                assert bool((np.abs(gl[act].astype(np.float64) - l2.np(what)[act]) <= 2 * ref["b_loss"][act]).all()), what
                WORST["ce rows bit-identical"] = min(WORST.get("ce rows bit-identical", 1.0), float(_same_bits(gl[act], l2.v.cpu().numpy()[act])))
    _report("ce loss"), _report("ce dlogits")
    print(f"[bits] sfmi_ce_fwd_bwd_f32 loss == sfmi_ce_rows_f32 on active rows: {bool(WORST['ce rows bit-identical'])}")


# ---------------------------------------------------------------------------------------------------- embedding scatter
@pytest.mark.parametrize("D", SCATTER_D)
def test_embedding_scatter_is_exact_fixed_point(dev, D):
    L = _L()
    rows = SCATTER_ROWS
    g = _gen(D)
    pats = {"one index": torch.full((2048,), 7, dtype=torch.int64),
            "spread": torch.cat([torch.tensor([0, rows - 1, 0]), torch.randint(0, rows, (496,), generator=g)])}
    for pname, idx in pats.items():
        M = idx.numel()
        for sc in SCATTER_SCALES:
            dxv = torch.randn(M, D, generator=g) * sc
            dxd, idd = _in(dxv, dev), _in(idx, dev, torch.int32)
            res = []
            for rep in range(3):
                acc = torch.zeros(rows * D + 2 * GUARD, dtype=torch.int64, device=dev)
                acc[:GUARD], acc[GUARD + rows * D:] = -0x5EAD, -0x5EAD
                _call("sfmi_embed_scatter_f32", dxd.data_ptr(), idd.data_ptr(), acc[GUARD:].data_ptr(), M, D, L.stream_ptr())
                for accm in (0, 1):
                    prev = torch.randn(rows, D, generator=_gen(5)) * sc if accm else None
                    o = Out((rows, D), dev, prev)
                    _call("sfmi_fixed_to_float_f32", acc[GUARD:].data_ptr(), o.v.data_ptr(), rows * D, accm, L.stream_ptr())
                    _sync()
                    what = f"scatter D{D} {pname} scale {sc} acc{accm}"
                    got = o.np(what)
                    assert bool((acc[:GUARD] == -0x5EAD).all()) and bool((acc[GUARD + rows * D:] == -0x5EAD).all()), what + ": wrote outside acc"
                    pn = None if prev is None else prev.numpy()
                    assert _same_bits(got, R.scatter_fixed_ref(dxv.numpy(), idx.numpy(), rows, pn)), what + ": not the exact fixed-point sum"
                    s, b = R.scatter_ref(dxv.numpy(), idx.numpy(), rows, pn)
                    assert _note("scatter", R.ratio(got, s, b)) <= 1.0, what
                    res.append(got)
            assert all(_same_bits(res[i], res[i % 2]) for i in range(6)), f"scatter D{D} {pname}: runs differ"
    _report("scatter")


# ---------------------------------------------------------------------------------------------------- dropout / add
@pytest.mark.parametrize("n", DROPOUT_N)
def test_dropout_matches_the_counter_hash(dev, n):
    L = _L()
    x = torch.randn(n, generator=_gen(n))
    for p in DROPOUT_P:
        seed = 0xC0FFEE11 + n
        a, b = Out((n,), dev, x), Out((n,), dev, x)
        _call("sfmi_dropout_f32", a.v.data_ptr(), a.v.data_ptr(), n, p, seed, L.stream_ptr())                      # in place
        sd = _u32(seed, dev)
        _call("sfmi_dropout_sd_f32", b.v.data_ptr(), b.v.data_ptr(), n, p, 1, sd.data_ptr(), L.stream_ptr())
        _sync()
        got = a.np(f"dropout n{n} p{p}")
        assert _same_bits(got, b.np("dropout_sd")), "seed from device memory gives other bits"
        mul = R.dropout_mul(seed, np.arange(n, dtype=np.int64), p)
        assert _same_bits(got, (x.numpy() * mul).astype(np.float32)), (n, p)
        if p == 0:
            assert _same_bits(got, x.numpy())
        if n == 4 * 65537:
            kept = float((got != 0).mean())
            assert abs(kept - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n) + 1e-12, (p, kept)


def test_add_is_exact(dev):
    L = _L()
    for n in (1, 255, 4099):
        a, b = torch.randn(n, generator=_gen(n)), torch.randn(n, generator=_gen(n + 1)) * 1e-3
        o, ad, bd = Out((n,), dev), _in(a, dev), _in(b, dev)
        _call("sfmi_add_f32", ad.data_ptr(), bd.data_ptr(), o.v.data_ptr(), n, L.stream_ptr())
        _sync()
        assert _same_bits(o.np("add"), a.numpy() + b.numpy())


# ---------------------------------------------------------------------------------------------------- AdamW
class _Adam:
    """The five-tensor table of ADAM_LENS on the device: parameters in separate sentinel-banded buffers, flat g / m / v at ADAM_FOFF[layout]."""

    def __init__(self, dev, layout, step):
        self.dev, self.layout, self.step = dev, layout, step
        self.foff = ADAM_FOFF[layout]
        self.nflat = self.foff[-1] + ADAM_LENS[-1]
        g = _gen(step)
        self.p0 = [torch.randn(n, generator=g) for n in ADAM_LENS]
        self.g0 = [torch.randn(n, generator=g) * sc for n, sc in zip(ADAM_LENS, ADAM_GSCALE)]
        self.m0 = [torch.randn(n, generator=g) * 0.1 if step > 1 else torch.zeros(n) for n in ADAM_LENS]
        self.v0 = [torch.rand(n, generator=g) * 0.01 if step > 1 else torch.zeros(n) for n in ADAM_LENS]
        self.m0[1].zero_(), self.v0[1].zero_()                                # g = m = v = 0: no NaN, p moves by its decay only
        bc = np.zeros(2, np.float32)
        _L().check(_L().lib().sfmi_adamw_bias_corrections(ADAM_HP["b1"], ADAM_HP["b2"], step, bc.ctypes.data), "bias corrections")
        self.bc = bc

    def flat(self, parts):
        f = torch.full((self.nflat,), float("nan"))
        for t, o in zip(parts, self.foff):
            f[o:o + t.numel()] = t
        return f

    def run(self, table, entry="multi", pflat=None, lr_arg=None, bc_dev=False):
        """one update; returns (p list, m flat, v flat, pflat or None, g flat) as numpy after the guard checks"""
        L = _L()
        lib, dev, hp = L.lib(), self.dev, ADAM_HP
        P = [Out((n,), dev, t) for n, t in zip(ADAM_LENS, self.p0)]
        G, Mo, Vo = Out((self.nflat,), dev, self.flat(self.g0)), Out((self.nflat,), dev, self.flat(self.m0)), Out((self.nflat,), dev, self.flat(self.v0))
        ct, co, cl = table
        dp = torch.tensor([o.v.data_ptr() for o in P], dtype=torch.int64, device=dev)
        tabs = [dp, torch.tensor(self.foff, dtype=torch.int64, device=dev), torch.tensor(ADAM_WD, dtype=torch.float32, device=dev),
                torch.tensor(ct, dtype=torch.int32, device=dev), torch.tensor(co, dtype=torch.int64, device=dev), torch.tensor(cl, dtype=torch.int32, device=dev)]
        tp = [t.data_ptr() for t in tabs]
        lr = hp["lr"] if lr_arg is None else lr_arg
        PF = None
        if pflat == "own":
            PF = Out((self.nflat,), dev)
        pfp = None if pflat is None else G.v.data_ptr() if pflat == "g" else PF.v.data_ptr()
        tail = (G.v.data_ptr(), Mo.v.data_ptr(), Vo.v.data_ptr(), lr, hp["b1"], hp["b2"], hp["eps"], self.step)
        if entry == "multi":
            L.check(lib.sfmi_adamw_multi_f32(*tp, len(ct), *tail, L.stream_ptr()), entry)
        elif entry == "shard":
            L.check(lib.sfmi_adamw_multi_shard_f32(*tp, len(ct), *tail, pfp, L.stream_ptr()), entry)
        else:
            bcd = torch.tensor([self.bc[0], self.bc[1], hp["lr"]], dtype=torch.float32, device=dev) if bc_dev else None
            L.check(lib.sfmi_adamw_multi_shard_bc_f32(*tp, len(ct), *tail[:-1], 0 if bc_dev else self.step, L.ptr(bcd), pfp, L.stream_ptr()), entry)
        _sync()
        return ([o.np(f"adam p{i}") for i, o in enumerate(P)], Mo.np("adam m", False), Vo.np("adam v", False),
                None if PF is None else PF.np("adam pflat", False), G.np("adam g", False))

    def covered(self, table):
        """per tensor: bool mask of the elements some chunk updates"""
        cov = [np.zeros(n, bool) for n in ADAM_LENS]
        for t, o, n in zip(*table):
            cov[t][o:o + n] = True
        return cov

    def check(self, table, res, what):
        hp = ADAM_HP
        ps, mf, vf = res[:3]
        cov = self.covered(table)
        for t, n in enumerate(ADAM_LENS):
            c, o = cov[t], self.foff[t]
            ref = R.adamw_ref(self.p0[t], self.g0[t], self.m0[t], self.v0[t], hp["lr"], hp["b1"], hp["b2"], hp["eps"], ADAM_WD[t], self.bc[0], self.bc[1])
            for name, got, old in (("p", ps[t], self.p0[t]), ("m", mf[o:o + n], self.m0[t]), ("v", vf[o:o + n], self.v0[t])):
                assert _note(f"adamw {name}", R.ratio(got[c], ref[name][c], ref["b_" + name][c])) <= 1.0, (what, t, name)
                assert _same_bits(got[~c], old.numpy()[~c]), (what, t, name, "an element outside every chunk changed")
        t = 1                                                          # g = m = v = 0
        c = cov[t]
        want = self.p0[t].double().numpy() * (1.0 - float(np.float32(hp["lr"])) * float(np.float32(ADAM_WD[t])))
        assert np.isfinite(ps[t]).all() and bool((np.abs(ps[t] - want)[c] <= 3 * U * np.abs(want)[c]).all()), (what, "zero gradient: p moves by its decay only")


@pytest.mark.parametrize("step", ADAM_STEPS)
def test_adamw_every_entry_against_float64_and_each_other(dev, step):
    L = _L()
    lib, hp = L.lib(), ADAM_HP
    A = _Adam(dev, "aligned", step)
    bc, bb = R.bias_corrections_ref(hp["b1"], hp["b2"], step)
    assert bool((np.abs(A.bc.astype(np.float64) - bc) <= bb).all()), (A.bc, bc)
    tv, ts, tpart = adam_chunks("vector"), adam_chunks("scalar"), adam_chunks("partial")
    rv = A.run(tv)
    A.check(tv, rv, f"step {step} vector")
    rs = A.run(ts)
    A.check(ts, rs, f"step {step} scalar")
    same = lambda a, b: all(_same_bits(x, y) for x, y in zip(a[0], b[0])) and _same_bits(a[1], b[1]) and _same_bits(a[2], b[2])
    assert same(rv, rs), "vector and scalar paths differ in bits"
    rp = A.run(tpart)
    A.check(tpart, rp, f"step {step} partial")
    # other flat offsets: tensors 1 and 3 start off a multiple of 4 (scalar path); the same bits per tensor
    Bo = _Adam(dev, "offset", step)
    ro = Bo.run(tv)
    Bo.check(tv, ro, f"step {step} offset layout")
    assert all(_same_bits(x, y) for x, y in zip(rv[0], ro[0])), "the flat layout changes the bits"
    # pflat (own buffer, then aliasing g), bc_dev with a wrong launch-time lr
    r1 = A.run(tpart, "shard", "own")
    assert same(rp, r1)
    cov = A.covered(tpart)
    for t, n in enumerate(ADAM_LENS):
        o = A.foff[t]
        assert _same_bits(r1[3][o:o + n][cov[t]], r1[0][t][cov[t]]), "pflat != p"
        assert bool((_bits(r1[3][o:o + n][~cov[t]]) == SENT).all()), "pflat written outside the chunks"
    r2 = A.run(tv, "shard", "g")
    assert same(rv, r2) and all(_same_bits(r2[4][A.foff[t]:A.foff[t] + n], r2[0][t]) for t, n in enumerate(ADAM_LENS)), "pflat aliasing g"
    r3 = A.run(tv, "bc", None, lr_arg=123.0, bc_dev=True)
    assert same(rv, r3), "bc_dev form differs from the launch-time form (or took lr from the launch argument)"
    r4 = A.run(tv, "bc", None)
    assert same(rv, r4)
    # the single-tensor entry on tensor 3 (wd 0) and tensor 4 (wd 0.01)
    for t in (3, 4):
        n = ADAM_LENS[t]
        p, m, v, gd = Out((n,), dev, A.p0[t]), Out((n,), dev, A.m0[t]), Out((n,), dev, A.v0[t]), _in(A.g0[t], dev)
        _call("sfmi_adamw_f32", p.v.data_ptr(), gd.data_ptr(), m.v.data_ptr(), v.v.data_ptr(), n, hp["lr"], hp["b1"], hp["b2"], hp["eps"],
              ADAM_WD[t], step, L.stream_ptr())
        _sync()
        ref = R.adamw_ref(A.p0[t], A.g0[t], A.m0[t], A.v0[t], hp["lr"], hp["b1"], hp["b2"], hp["eps"], ADAM_WD[t], A.bc[0], A.bc[1])
        for name, o in (("p", p), ("m", m), ("v", v)):
            assert _note(f"adamw {name}", R.ratio(o.np("adamw_f32"), ref[name], ref["b_" + name])) <= 1.0, (t, name)
    for k in "pmv":
        _report(f"adamw {k}")


def test_unflatten_copies_inside_its_chunks_only(dev):
    L = _L()
    lib = L.lib()
    foff = ADAM_FOFF["offset"]
    nflat = foff[-1] + ADAM_LENS[-1]
    flat = torch.randn(nflat, generator=_gen(3))
    ct, co, cl = adam_chunks("partial")
    P = [Out((n,), dev) for n in ADAM_LENS]
    tabs = [torch.tensor([o.v.data_ptr() for o in P], dtype=torch.int64, device=dev), torch.tensor(foff, dtype=torch.int64, device=dev),
            torch.tensor(ct, dtype=torch.int32, device=dev), torch.tensor(co, dtype=torch.int64, device=dev), torch.tensor(cl, dtype=torch.int32, device=dev)]
    fd = _in(flat, dev)
    L.check(lib.sfmi_unflatten_multi_f32(*[t.data_ptr() for t in tabs], len(ct), fd.data_ptr(), L.stream_ptr()), "unflatten")
    _sync()
    for t, o, n in zip(ct, co, cl):
        got = P[t].np("unflatten", written=False)
        assert _same_bits(got[o:o + n], flat.numpy()[foff[t] + o:foff[t] + o + n])
        assert bool((_bits(got[:o]) == SENT).all()) and bool((_bits(got[o + n:]) == SENT).all())


# ---------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("B,L,H", ATTN_CASES)
def test_attention_training_forward_and_backward(dev, B, L, H):
    L_ = _L()
    lib = L_.lib()
    D, Lmax = 64 * H, L + 1
    g = _gen(B * 1000 + L * 10 + H)
    qkv, dy = torch.randn(B * L, 3 * D, generator=g), torch.randn(B * L, D, generator=g)
    qd, dyd = _in(qkv, dev), _in(dy, dev)
    nval = torch.full((B,), L, device=dev, dtype=torch.int32)
    small = R.attn_fwd_small(B, L, H)
    for p in ATTN_P:
        seed = 0x51ED270B + L
        sd = _u32(seed, dev)
        fw = R.attn_fwd_ref(qkv, B, L, H, R.attn_mask(seed, B, H, L, p) if p else None)
        what = f"attn B{B} L{L} H{H} p{p}"
        ys = []
        for form in ("prefill", "prefill_sd", "small", "small_sd"):
            y, lse = Out((B * L, D), dev), Out((B, H, L), dev)
            if form.startswith("prefill"):
                kc, vc = Out((B * Lmax * D,), dev), Out((B * Lmax * D,), dev)
                if form == "prefill":
                    rc = lib.sfmi_gpt_attn_prefill_lse_f32(qd.data_ptr(), kc.v.data_ptr(), vc.v.data_ptr(), nval.data_ptr(), y.v.data_ptr(), B, L, D, H, Lmax, None,
                                                           p, seed, lse.v.data_ptr(), L_.stream_ptr())
                else:
                    rc = lib.sfmi_gpt_attn_prefill_lse_sd_f32(qd.data_ptr(), kc.v.data_ptr(), vc.v.data_ptr(), nval.data_ptr(), y.v.data_ptr(), B, L, D, H, Lmax,
                                                              None, p, 1, sd.data_ptr(), lse.v.data_ptr(), L_.stream_ptr())
            elif form == "small":
                rc = lib.sfmi_attn_train_fwd_small_f32(qd.data_ptr(), y.v.data_ptr(), lse.v.data_ptr(), B, L, D, H, p, seed, L_.stream_ptr())
            else:
                rc = lib.sfmi_attn_train_fwd_small_sd_f32(qd.data_ptr(), y.v.data_ptr(), lse.v.data_ptr(), B, L, D, H, p, 1, sd.data_ptr(), L_.stream_ptr())
            if form.startswith("small") and not small:
                assert rc == L_.SFMI_EINVAL, what
                continue
            L_.check(rc, form)
            _sync()
            if form.startswith("prefill"):
                kc.check(what + " K cache", written=False), vc.check(what + " V cache", written=False)
            fam = "attn fwd " + form.split("_")[0]
            assert _note(fam + " y", R.ratio(y.np(what + form), fw["y"], fw["b_y"])) <= 1.0, (what, form)
            assert _note(fam + " lse", R.ratio(lse.np(what + form), fw["lse"], fw["b_lse"])) <= 1.0, (what, form)
            ys.append((form, y, lse))
        by = dict((f, (y, l)) for f, y, l in ys)
        assert _same_bits(by["prefill"][0].v, by["prefill_sd"][0].v), what + ": seed from device memory gives other bits (prefill)"
        if small:
            assert _same_bits(by["small"][0].v, by["small_sd"][0].v), what + ": seed from device memory gives other bits (small forward)"
        y, lse = by["small" if small else "prefill"]
        # backward from the forward's y and lse
        bw = R.attn_bwd_ref(fw, dy, B, L, H)
        dref, dbound = R.delta_ref(y.v, dy, B, L, H)
        outs = {}
        for form in ("lse", "lse_sd", "stats"):
            dq = Out((B * L, 3 * D), dev)
            if form == "stats":
                scr = Out((2, B, H, L), dev)
                L_.check(lib.sfmi_attn_bwd_f32(qd.data_ptr(), y.v.data_ptr(), dyd.data_ptr(), scr.v.data_ptr(), dq.v.data_ptr(), B, L, D, H, p, seed, L_.stream_ptr()), form)
                _sync()
                s = scr.np(what + " stats scratch")
                assert _note("attn stats lse", R.ratio(s[0], fw["lse"], fw["b_lse"])) <= 1.0, what
                assert _note("attn delta", R.ratio(s[1], dref, dbound)) <= 1.0, what
            else:
                de = Out((B, H, L), dev)
                if form == "lse":
                    L_.check(lib.sfmi_attn_bwd_lse_f32(qd.data_ptr(), y.v.data_ptr(), dyd.data_ptr(), lse.v.data_ptr(), de.v.data_ptr(), dq.v.data_ptr(), B, L, D, H,
                                                       p, seed, L_.stream_ptr()), form)
                else:
                    L_.check(lib.sfmi_attn_bwd_lse_sd_f32(qd.data_ptr(), y.v.data_ptr(), dyd.data_ptr(), lse.v.data_ptr(), de.v.data_ptr(), dq.v.data_ptr(), B, L, D, H,
                                                          p, 1, sd.data_ptr(), L_.stream_ptr()), form)
                _sync()
                assert _note("attn delta", R.ratio(de.np(what + " delta"), dref, dbound)) <= 1.0, what
                assert _note("attn delta vs f64 y", R.ratio(de.v, bw["delta"], bw["b_delta"])) <= 1.0, what
            fam = "attn bwd <%d,%d>" % R.attn_bwd_form(B, L, H)
            assert _note(fam, R.ratio(dq.np(what + " dqkv " + form), bw["dqkv"], bw["b_dqkv"])) <= 1.0, (what, form)
            outs[form] = dq.v
        assert _same_bits(outs["lse"], outs["lse_sd"]), what + ": seed from device memory gives other bits (backward)"
    for k in sorted(WORST):
        if k.startswith("attn"):
            _report(k)


# ---------------------------------------------------------------------------------------------------- one step at the product's width
@pytest.fixture(scope="module")
def step_setup(dev):
    from oracle import gpt_oracle as GO
    from shapeformer_amd import weights as W
    from shapeformer_amd.gpt import CondTupleGPT
    kw = dict(STEP_KW)
    nh = kw.pop("n_head")
    sd = W.make_state_dict(W.gpt_spec(**kw))
    cfg = GO.GPTCfg(n_head=nh, **kw)
    g = CondTupleGPT(sd, n_head=nh, device=dev, **kw)
    t = np.load(os.path.join(HERE, "golden", "gpt_tiny.npz"))
    return sd, cfg, g, torch.from_numpy(t["c_idx"]), torch.from_numpy(t["z_idx"])


@pytest.mark.parametrize("mode", ["eval", "train"])
def test_training_step_at_width_1024_against_the_float64_oracle(dev, step_setup, mode):
    from shapeformer_amd.train import GPTTrainer
    from test_train_gpu import _map
    sd, cfg, g, c, z = step_setup
    pd = STEP_PDROP if mode == "train" else None
    tr = GPTTrainer(g, pdrop=pd) if pd else GPTTrainer(g)
    tr.debug_poison_grads = True
    loss = tr.loss_and_grad(c, z, dropout_key="k7").item() if pd else tr.loss_and_grad(c, z).item()
    l64, rows = R.step_ratios(sd, cfg, c, z, dict(key="k7", p=pd) if pd else None, _map(tr, cfg), lambda name: tr.grad[name].cpu())
    assert abs(loss - l64) < 1e-5 * max(1.0, abs(l64)), (loss, l64)                 # the gate of test_train_gpu.py
    bad = []
    for name, e_gpu, e_cpu, ratio in rows:
        print(f"[step {mode}] {name:14s} gpu {e_gpu:.2e}  cpu fp32 {e_cpu:.2e}  ratio {ratio:.2f}")
        if ratio > GATE_X:
            bad.append((name, round(ratio, 2)))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- argument checks
def test_argument_ranges_are_refused_before_any_launch(dev):
    """by return value only: every pointer is a real buffer large enough for the VALID call, only one integer is out of range"""
    L = _L()
    lib, st, E = L.lib(), L.stream_ptr(), L.SFMI_EINVAL
    f = lambda *shape: torch.zeros(*shape, device=dev)
    a, o, ti = f(64, 64), f(64, 64), torch.zeros(64, dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr()
    assert lib.sfmi_transpose_f32(p(a), p(o), 8, 8, 7, 8, st) == E                                       # ldin < C
    assert lib.sfmi_colsum_f32(p(a), p(o), 8, 8, 7, 0, st) == E                                          # ld < N
    assert lib.sfmi_colsum_ws_f32(p(a), p(o), 8, 8, 7, 0, p(f(64)), st) == E
    kinds, Ns, lds = np.array([0], np.int32), np.array([8], np.int32), np.array([4], np.int32)            # ld[i] < N[i]
    ap, op = np.array([p(a)], np.uint64), np.array([p(o)], np.uint64)
    assert lib.sfmi_col_reduce_f32(1, kinds.ctypes.data, ap.ctypes.data, None, None, op.ctypes.data, None, Ns.ctypes.data, lds.ctypes.data, 8, 0, None, 0, None, 0, st) == E
    ce = lambda M, V, ld, Lr, t0: lib.sfmi_ce_fwd_bwd_f32(p(a), p(ti), p(f(64)), p(o), M, V, ld, Lr, t0, 1.0, st)
    assert ce(8, 0, 8, 4, 0) == E and ce(8, 9, 8, 4, 0) == E and ce(8, 8, 8, 0, 0) == E and ce(8, 8, 8, 4, -1) == E
    q, y, scr = f(4, 192), f(4, 64), f(2, 4)
    ab = lambda B, Lr, H: lib.sfmi_attn_bwd_f32(p(q), p(y), p(y), p(scr), p(f(4, 192)), B, Lr, 64 * max(H, 0), H, 0.0, 0, st)
    assert ab(0, 4, 1) == E and ab(1, 0, 1) == E and ab(1, 4, 0) == E
    al = lambda B, Lr: lib.sfmi_attn_bwd_lse_f32(p(q), p(y), p(y), p(scr), p(scr[1]), p(f(4, 192)), B, Lr, 64, 1, 0.0, 0, st)
    assert al(0, 4) == E and al(1, 0) == E
    # the block-form LayerNorm (D = 3) with a dropped output of M * D = 15 elements: refused BEFORE the row kernel runs - dx keeps its fill
    dx = Out((5, 3), dev)
    rc = lib.sfmi_layernorm_bwd_rows_drop_sd_f32(p(f(5, 3)), p(f(5, 3)), p(f(3)), None, p(dx.v), p(f(5, 2)), p(f(5, 3)), 0.1, 1, None, 5, 3, st)
    _sync()
    assert rc == E and bool((_bits(dx.v) == SENT).all()), "the M * D % 4 check must come before the first launch"
