"""csrc/sgemm.hip and csrc/sgemm_sk.hip through the C ABI against float64 (tests/gemm_ref.py: reference, derived per-element bound,
mirrors of the host rules and of the device-side work split) at every instance and work split: the four operand forms, the split-K
slice counts 1 / 2 / 4 / 8 with the scratch-driven halving, the twelve stream-K instances (128 x 128, 64 x 64 plain loop, 64 x 64
pipelined loop), every `sk_grid`, natural and padded lda / ldb / ldc, the fused epilogues against train_ref's dropout and GELU, the
bit-identity claims of csrc/sfmi_common.h, and the argument checks by return value.  Operand rows and columns carry scales over
2^-10 .. 2^10, so the per-element bounds differ by orders of magnitude inside one tile.  Every output and scratch buffer is SENT-filled
between guard bands, every input sits between NaN bands with NaN padding columns; every `[ratio]` line (pytest -s) is the largest
error / bound of a family.  The case tables below are plain data: tests/test_gemm_ref_cpu.py imports them and proves, from the
mirrors, that they reach every form.

Measured on one MI355X (largest error / bound per family).  Products: sgemm.hip S = 1 0.50 (K = 4, where the bound is five roundings;
0.11 at K = 36, 0.002 at K = 2052), S = 2 0.0014, S = 4 0.0007, S = 8 0.0004; stream-K 64 x 64 0.20 in both loops (K = 4; 0.076 at K = 68,
0.010 at K = 224, 0.003 at K = 288), 128 x 128 0.23 (K = 4; 0.15 at K = 36, 0.067 at K = 68).  The [PROD] bound grows with K^2 while the error of random operands grows
with K, so the deep-K families (S > 1 needs K >= 512) sit at about 1 / K of it; the bound keeps its teeth there all the same:
test_gemm_ref_cpu.py applies the mutants to these very cases, and one dropped k index out of 2052 in one tile lands at 15 x the bound, a
skipped slice at 221 x, a swapped row pair at 5e7 x.  Epilogues: sgemm.hip direct 0.83 / 0.74 / 0.41 (act 0 / 1 / 2), through the reduce
kernel 0.28 / 0.26 / 0.16; stream-K direct 0.81 / 0.79 / 0.42 / 0.47 (act 0 .. 3; C2 0.81), cut tiles 0.41 / 0.41 / 0.20 / 0.26 (C2 0.27).
No measured constant enters a bound: the matrix core's f32 multiply-adds behave as individually rounded operations.
Every bit-identity claim held: three launches of the same product (both entries, every S, cut tiles at every grid, both loops),
sk_loop 1 == sk_loop 0 at every case of the 64 x 64 table and in every epilogue combination it ran, sk_stagger 3 == 0, the seed from
device memory == the seed by value, the same S reached from two scratch sizes, resid aliasing C == a separate buffer, and the zeros of
csrc/sgemm.hip == those of csrc/sgemm_sk.hip == train_ref.dropout_mul's.  No kernel defect was found.  Host defects fixed with this
file: sfmi_sgemm_mfma_f32 accepted any act (3 ran without an activation) and a negative ws_floats; both entries accepted an lda, ldb
or ldc shorter than the row it strides (rows overlapping in memory: a C whose rows overwrite each other).  The file runs in 3 s."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import gemm_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
SENT = 0x7FC0DEAD          # NaN bit pattern of every "must stay untouched" float
ISENT = -0x5EAD            # the same for ticket counters
GUARD = 256                # band elements on either side of every buffer
EINVAL = -1

# ---------------------------------------------------------------------------------------------------- the case tables
# stream-K: (M, N, K, sk_tile, sk_grid); tests/test_gemm_ref_cpu.py states what each row reaches and refuses a row that adds nothing
SK_CASES = [
    (64, 64, 288, 1, 512),         # one tile, nine contributors, G clamped to 9 units
    (640, 576, 224, 1, 256),       # 3-4 contributors, both slots, odd and even multi-chunk partials
    (640, 576, 224, 1, 512),       # 5-6 contributors: two gather rounds
    (260, 132, 1060, 1, 256),      # 17-18 contributors: five gather rounds, the last one short
    (1284, 1156, 68, 1, 256),      # pw / wp / pwp workgroups, a last panel of five M-tiles, a K tail
    (1284, 1156, 68, 1, 768),      # the other two grids, unclamped
    (1284, 1156, 68, 1, 1024),
    (1284, 1156, 68, 2, 256),      # both slots in the 128 x 128 form
    (2564, 2308, 36, 2, 256),      # 128 x 128: whole and cut tiles in one workgroup (pw / wp / pwp)
    (1284, 1028, 228, 2, 256),     # 128 x 128: odd multi-chunk partials, 3-4 contributors
    (4, 4, 4, 1, 512),             # one unit
    (4, 4, 4, 2, 512),
]
SK_ODD_K = (260, 132, 1059, 1, 256)            # K % 4 != 0: the (transA, !transB) form only
SK_PADS = (0, 4, 36)                            # added to lda, ldb and ldc
SK_STAGGER_CASES = [(640, 576, 224, 1, 256), (1284, 1156, 68, 2, 256)]
# sgemm.hip: (M, N, K); SG_WS: the scratch sizes every case runs with, in units of M * N floats (None: ws = NULL)
SG_CASES = ([(132, 132, 2052), (1028, 132, 36)] + [(132, 132, K) for K in (4, 28, 32, 64, 68, 100)]
            + [(4, 124, 36), (124, 128, 36), (128, 4, 36)])
SG_ODD_K = (132, 132, 2051)                     # (transA, !transB) only
SG_WS = (8, 4, 2, 1, None)
SG_PADS = (0, 4, 36)
# epilogues: (M, N, K) of a cut and a direct case per entry
SK_EPI_CASES = {"cut": (132, 68, 288), "direct": (132, 68, 32)}            # stream-K: every tile cut in nine / one chunk per tile
SG_EPI_CASES = {"reduce": (132, 68, 516), "direct": (132, 68, 36)}         # sgemm.hip: S = 2 through the reduce kernel (8 + 9 chunks) / S = 1
EPI_P = (0.0, 0.1, 0.9)
EPI_RESID = ("none", "separate", "alias")
SK_ACTS = ((0, False), (1, False), (2, False), (2, True), (3, False))      # (act, with C2)
SG_ACTS = (0, 1, 2)
SK_INSTANCES = ((2, 0), (1, 0), (1, 1))                                     # (sk_tile, sk_loop)

# argument tuples both entries refuse (EINVAL) or accept: name -> overrides of BASE_ARGS; "sk only" / "sg only" rows carry a prefix
BASE_ARGS = dict(tA=0, tB=1, M=132, N=68, K=36, lda=36, ldb=36, ldc=68, act=0, drop_p=0.0)
ARG_TABLE = [
    ("base", {}), ("padded", dict(lda=40, ldb=72, ldc=72)),
    ("M0", dict(M=0)), ("N0", dict(N=0)), ("K0", dict(K=0)), ("N%4", dict(N=66, ldc=68)), ("K%4 form 01", dict(K=34)),
    ("K%4 form 00", dict(tB=0, K=34, ldb=68)), ("K%4 form 11", dict(tA=1, K=34, lda=132)), ("K odd form 10", dict(tA=1, tB=0, K=35, lda=132, ldb=68)),
    ("M%4 transA", dict(tA=1, M=130, lda=132)), ("lda%4", dict(lda=38)), ("ldb%4", dict(ldb=38)), ("ldc%4", dict(ldc=70)),
    ("lda<K", dict(lda=32)), ("lda<M transA", dict(tA=1, lda=128)), ("lda=M transA", dict(tA=1, lda=132)), ("ldb<K", dict(ldb=32)),
    ("ldb<N", dict(tB=0, ldb=64)), ("ldb=N", dict(tB=0, ldb=68)), ("ldc<N", dict(ldc=64)),
    ("act -1", dict(act=-1)), ("act 3", dict(act=3)), ("act 3 aux", dict(act=3, aux=True)), ("act 4", dict(act=4, aux=True)),
    ("p<0", dict(drop_p=-0.1)), ("p=1", dict(drop_p=1.0)), ("p=.9", dict(drop_p=0.9)),
    ("A null", dict(A=False)), ("B null", dict(B=False)), ("C null", dict(C=False)),
    ("sg ws_floats<0", dict(ws_floats=-1)), ("sg ws small", dict(ws_floats=1)),
    ("sk slab null", dict(slab=False)), ("sk cnt null", dict(cnt=False)), ("sk slab short", dict(slab_short=1)), ("sk cnt short", dict(cnt_short=1)),
]


def forms_of(M, K):
    """the operand forms a shape may run in: K % 4 is needed unless (transA, !transB), M % 4 when transA"""
    return [(tA, tB) for tA, tB in R.FORMS if not (tA and M % 4) and not (K % 4 and (not tA or tB))]


# ---------------------------------------------------------------------------------------------------- plumbing
def _L():
    from shapeformer_amd import _lib as L
    return L


def _tune(**kw):
    L = _L()
    for k, v in kw.items():
        L.check(L.lib().sfmi_tune_set(k.encode(), int(v)), f"tune {k}")


def _defaults():
    _tune(sk_tile=0, sk_grid=R.SK_GRID_DEFAULT, sk_loop=0, sk_stagger=0)


def _in(a, dev):
    """a device copy of the numpy array a (padding columns included) between two NaN bands"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.full((t.numel() + 2 * GUARD,), float("nan"), device=dev)
    buf[GUARD:GUARD + t.numel()] = t.reshape(-1).to(dev)
    return buf[GUARD:GUARD + t.numel()].view(t.shape)


class Out:
    """an (M, N; ld) float output or a flat scratch: SENT everywhere, the data between two guard bands; init: the (M, N) values an
    accumulating launch starts from"""

    def __init__(self, M, N, ld, dev, init=None):
        self.M, self.N, self.ld = M, N, ld
        self.buf = torch.full((M * ld + 2 * GUARD,), SENT, dtype=torch.int32, device=dev).view(torch.float32)
        self.full = self.buf[GUARD:GUARD + M * ld].view(M, ld)
        self.v = self.full[:, :N]
        if init is not None:
            self.v.copy_(init if torch.is_tensor(init) else torch.from_numpy(np.ascontiguousarray(init)).to(dev))

    def ptr(self):
        return self.full.data_ptr()

    def check(self, what, written=True, untouched=False):
        bits = self.buf.view(torch.int32)
        inner = bits[GUARD:GUARD + self.M * self.ld].view(self.M, self.ld)
        assert bool((bits[:GUARD] == SENT).all()) and bool((bits[GUARD + self.M * self.ld:] == SENT).all()), f"{what}: wrote outside the buffer"
        assert bool((inner[:, self.N:] == SENT).all()), f"{what}: wrote into the padding columns N .. ld - 1"
        if untouched:
            assert bool((inner == SENT).all()), f"{what}: wrote although nothing may be written"
        elif written:
            assert not bool((inner[:, :self.N] == SENT).any()), f"{what}: left part of the output unwritten"
        return self.v


class Scratch:
    """slab and ticket counters of EXACTLY the size the launch needs (the mirror's G * 2 * BM * BM floats, 4 * tiles ints)"""

    def __init__(self, M, N, K, tile, grid, dev):
        g = R.sk_geometry(M, N, K, R.sk_tile(M, N, K, tile), grid)
        self.slab_floats, self.cnt_ints = g.slab, 4 * g.tiles
        self.slab = Out(1, g.slab, g.slab, dev)
        self.cbuf = torch.full((self.cnt_ints + 2 * GUARD,), ISENT, dtype=torch.int32, device=dev)
        self.cnt = self.cbuf[GUARD:GUARD + self.cnt_ints]
        self.cnt.zero_()

    def check(self, what):
        self.slab.check(what + " slab", written=False)
        assert bool((self.cbuf[:GUARD] == ISENT).all()) and bool((self.cbuf[GUARD + self.cnt_ints:] == ISENT).all()), f"{what}: wrote outside the counters"
        assert not bool(self.cnt.any()), f"{what}: a ticket counter was left armed"


def _bits(a):
    return a.contiguous().view(torch.int32)


def _same_bits(a, b):
    return bool(torch.equal(_bits(a), _bits(b)))


def _sync():
    torch.cuda.synchronize()


def _dev64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _ratio_dev(got, ref, bound):
    """train_ref.ratio on the device: max |got - ref| / bound, inf for a non-finite value or an error at a zero bound"""
    g = got.double()
    if not bool(torch.isfinite(g).all()):
        return math.inf
    d = (g - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    return float(r.max()) if r.numel() else 0.0


WORST = {}


def _note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def _report(*families):
    for f in families:
        if f in WORST:
            print(f"[ratio] {f}: largest error / bound {WORST[f]:.3g}")


def _u32(seed, dev):
    return torch.tensor([seed if seed < 2 ** 31 else seed - 2 ** 32], dtype=torch.int32, device=dev)


def _operands_dev(op, tA, tB, pad, dev):
    """(A, lda, B, ldb) as the entry reads them: stored form, row stride padded by `pad` NaN columns"""
    M, K = op["A"].shape
    N = op["B"].shape[1]
    lda, ldb = (M if tA else K) + pad, (K if tB else N) + pad
    return _in(R.stored(op["A"], tA, lda), dev), lda, _in(R.stored(op["B"], tB, ldb), dev), ldb


def _p(t):
    return None if t is None else (t.ptr() if isinstance(t, Out) else t.data_ptr())


def _sg(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, acc=0, bias=None, act=0, resid=None, ws=None, ws_floats=0, p=0.0, seed=0):
    L = _L()
    return L.lib().sfmi_sgemm_mfma_f32(tA, tB, M, N, K, _p(A), lda, _p(B), ldb, _p(C), ldc, acc, _p(bias), act, _p(resid), _p(ws), ws_floats, p, seed,
                                       L.stream_ptr())


def _sk(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, scr, c2=None, acc=0, bias=None, act=0, aux=None, resid=None, p=0.0, seed=0, seed_dev=None,
        slab_floats=None, cnt_ints=None, by_value_entry=False):
    L = _L()
    sf = scr.slab_floats if slab_floats is None else slab_floats
    ci = scr.cnt_ints if cnt_ints is None else cnt_ints
    if by_value_entry:
        return L.lib().sfmi_sgemm_sk_f32(tA, tB, M, N, K, _p(A), lda, _p(B), ldb, _p(C), _p(c2), ldc, acc, _p(bias), act, _p(aux), _p(resid), p, seed,
                                         _p(scr.slab), sf, scr.cnt.data_ptr(), ci, L.stream_ptr())
    return L.lib().sfmi_sgemm_sk_sd_f32(tA, tB, M, N, K, _p(A), lda, _p(B), ldb, _p(C), _p(c2), ldc, acc, _p(bias), act, _p(aux), _p(resid), p, seed,
                                        _p(seed_dev), _p(scr.slab), sf, scr.cnt.data_ptr(), ci, L.stream_ptr())


# ---------------------------------------------------------------------------------------------------- sgemm.hip: product and split-K
@pytest.mark.parametrize("M,N,K", SG_CASES + [SG_ODD_K])
def test_sgemm_product_every_form_stride_and_slice_count(dev, M, N, K):
    L = _L()
    op = R.operands(M, N, K, seed=M * 7 + N * 3 + K, epilogue=False)
    want_S = int(L.lib().sfmi_sgemm_mfma_splits(M, N, K))
    assert want_S == R.mfma_splits(M, N, K)
    ref, absprod = _dev64(R.f64(op["A"]) @ R.f64(op["B"]), dev), _dev64(R.abs_product(op["A"], op["B"]), dev)
    for tA, tB in forms_of(M, K):
        for pad in SG_PADS:
            A, lda, B, ldb = _operands_dev(op, tA, tB, pad, dev)
            ldc = N + pad
            first, seen = {}, set()
            for w in SG_WS:
                ws_floats = None if w is None else w * M * N
                S = R.mfma_launch_splits(M, N, K, ws_floats)
                if pad and (S, w is None) in seen:                    # a scratch size that repeats an S: at natural strides only
                    continue
                seen.add((S, w is None))
                C = Out(M, N, ldc, dev)
                ws = None if w is None else Out(1, ws_floats, ws_floats, dev)
                what = f"sgemm {tA}{tB} {M}x{N}x{K} pad {pad} ws {w} S {S}"
                outs = []
                for _ in range(1 if pad else 3):
                    assert _sg(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, ws=ws, ws_floats=ws_floats or 0) == 0, what
                    _sync()
                    outs.append(C.check(what).clone())
                assert all(_same_bits(outs[0], o) for o in outs[1:]), what + ": not bit-identical from run to run"
                if ws is not None:                                    # slices 0 .. S - 1 written in full, nothing past S * M * N
                    ws.check(what + " ws", written=False)
                    wsb, used = ws.full.view(torch.int32).reshape(-1), (S * M * N if S > 1 else 0)
                    assert not bool((wsb[:used] == SENT).any()) and bool((wsb[used:] == SENT).all()), what + ": ws beyond S * M * N"
                r = _note(f"sgemm S{S}", _ratio_dev(outs[0], ref, absprod * float(R.gamma(K + S))))
                assert r <= 1.0, (what, r)
                if S in first:                                        # the same S from another scratch size (or ws = NULL) is the same launch
                    assert _same_bits(first[S], outs[0]), what + ": differs from the same S reached another way"
                first.setdefault(S, outs[0])
    _report(*(f"sgemm S{S}" for S in (1, 2, 4, 8)))


# ---------------------------------------------------------------------------------------------------- sgemm_sk.hip: product and work split
@pytest.mark.parametrize("case", SK_CASES + [SK_ODD_K], ids=lambda c: "x".join(map(str, c[:3])) + f"-t{c[3]}-g{c[4]}")
def test_sk_product_every_instance_grid_and_stride(dev, case):
    M, N, K, tile, grid = case
    L = _L()
    _defaults()
    assert int(L.lib().sfmi_sgemm_sk_cnt_ints(M, N)) == R.sk_cnt_ints(M, N) and int(L.lib().sfmi_sgemm_sk_slab_floats()) == R.sk_slab_floats()
    assert int(L.lib().sfmi_sgemm_sk_tile(M, N, K)) == R.sk_tile(M, N, K)
    plan = R.sk_plan(M, N, K, tile, grid)
    op = R.operands(M, N, K, seed=M + 3 * N + 5 * K + tile + grid, epilogue=False)
    P, b = R.product_ref(op["A"], op["B"], max(plan.contributors))
    ref, bound = _dev64(P, dev), _dev64(b, dev)
    fam = f"sk {'128' if tile == 2 else '64'}"
    try:
        _tune(sk_tile=tile, sk_grid=grid)
        scr = Scratch(M, N, K, tile, grid, dev)
        for fi, (tA, tB) in enumerate(forms_of(M, K)):
            for pad in SK_PADS:
                A, lda, B, ldb = _operands_dev(op, tA, tB, pad, dev)
                ldc = N + pad
                what = f"sk {tA}{tB} {M}x{N}x{K} tile {tile} grid {grid} pad {pad}"
                if fi == 0 and pad == 0:                             # one float less of slab, one counter less: refused, nothing written
                    C = Out(M, N, ldc, dev)
                    assert _sk(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, scr, slab_floats=scr.slab_floats - 1) == EINVAL, what
                    assert _sk(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, scr, cnt_ints=scr.cnt_ints - 1) == EINVAL, what
                    _sync()
                    C.check(what + " refused", untouched=True)
                    scr.slab.check(what + " refused slab", untouched=True)
                res = {}
                for loop in ((0, 1) if tile == 1 else (0,)):
                    _tune(sk_loop=loop)
                    outs = []
                    for _ in range(3 if pad == 0 else 1):
                        C = Out(M, N, ldc, dev)
                        assert _sk(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, scr) == 0, what
                        _sync()
                        outs.append(C.check(f"{what} loop {loop}"))
                        scr.check(f"{what} loop {loop}")
                    assert all(_same_bits(outs[0], o) for o in outs[1:]), f"{what} loop {loop}: not bit-identical from run to run"
                    r = _note(f"{fam} loop {loop}", _ratio_dev(outs[0], ref, bound))
                    assert r <= 1.0, (what, loop, r)
                    res[loop] = outs[0]
                if 1 in res:
                    assert _same_bits(res[0], res[1]), what + ": sk_loop 1 is not bit-identical to sk_loop 0"
    finally:
        _defaults()
    _report(*([fam + " loop 0"] + ([fam + " loop 1"] if tile == 1 else [])))


@pytest.mark.parametrize("case", SK_STAGGER_CASES, ids=lambda c: "x".join(map(str, c[:3])) + f"-t{c[3]}")
def test_sk_stagger_is_bit_identical(dev, case):
    M, N, K, tile, grid = case
    op = R.operands(M, N, K, seed=11, epilogue=False)
    _defaults()
    try:
        _tune(sk_tile=tile, sk_grid=grid)
        scr = Scratch(M, N, K, tile, grid, dev)
        for tA, tB in forms_of(M, K):
            A, lda, B, ldb = _operands_dev(op, tA, tB, 0, dev)
            res = []
            for stagger in (0, 3):
                _tune(sk_stagger=stagger)
                C = Out(M, N, N, dev)
                assert _sk(tA, tB, M, N, K, A, lda, B, ldb, C, N, scr) == 0
                _sync()
                res.append(C.check(f"stagger {stagger}"))
                scr.check(f"stagger {stagger}")
            assert _same_bits(res[0], res[1]), (case, tA, tB)
    finally:
        _defaults()


# ---------------------------------------------------------------------------------------------------- epilogues
class _Epi:
    """operands of one epilogue case on the device, the float64 product and its bound"""

    def __init__(self, M, N, K, c, dev, seed):
        self.M, self.N, self.K, self.dev = M, N, K, dev
        self.op = R.operands(M, N, K, seed)
        self.P, self.bP = R.product_ref(self.op["A"], self.op["B"], c)
        self.stored = {}

    def ab(self, tA, tB):
        if (tA, tB) not in self.stored:
            self.stored[(tA, tB)] = _operands_dev(self.op, tA, tB, 4, self.dev)
        return self.stored[(tA, tB)]

    def padded(self, name, ldc):
        return _in(R.stored(self.op[name], False, ldc), self.dev)


def _epilogue_combos():
    """(accumulate, bias, resid mode, p) in a fixed order; the index picks the operand form, the instance and ldc"""
    return [(acc, bias, rm, p) for acc in (0, 1) for bias in (0, 1) for rm in EPI_RESID for p in EPI_P]


def _check_epilogue(e, launch, act, has_c2, ldc, acc, bias, rm, p, seed, fam, what):
    """run `launch(C, C2, resid)` for one combination and check C, C2 (has_c2: the launch receives one), the dropped positions and the
    aliasing claim"""
    op, dev, M, N = e.op, e.dev, e.M, e.N
    cinit = op["C0"] if (acc or rm == "alias") else None
    res_np = None if rm == "none" else (op["C0"] if rm == "alias" else op["resid"])
    want = R.epilogue_ref(e.P, e.bP, C0=op["C0"] if acc else None, bias=op["bias"] if bias else None, act=act, aux=op["aux"], resid=res_np, p=p, seed=seed)
    C = Out(M, N, ldc, dev, cinit)
    C2 = Out(M, N, ldc, dev) if has_c2 else None
    rsep = None if rm == "none" else _in(R.stored(res_np, False, ldc), dev)
    assert launch(C, C2, rsep) == 0, what
    _sync()
    got = C.check(what).cpu().numpy()
    if rm == "alias":                                                 # the residual read from C itself: bit-identical to the separate buffer
        Ca = Out(M, N, ldc, dev, cinit)
        assert launch(Ca, None, Ca) == 0, what
        _sync()
        assert _same_bits(Ca.check(what + " alias"), C.v), what + ": resid aliasing C differs from the separate buffer"
    assert _note(fam, R.ratio(got, want["y"], want["b"])) <= 1.0, (what, WORST[fam])
    if p > 0:                                                         # dropped positions: exactly the residual (or zero)
        base = np.zeros((M, N), np.float32) if res_np is None else res_np
        d = ~want["keep"]
        assert np.array_equal(got[d], base[d]), what + ": a dropped position is not exactly the residual"
        assert 0 < d.sum() < d.size
    if C2 is not None:
        if act == 2:
            assert _note(fam + " C2", R.ratio(C2.check(what + " C2").cpu().numpy(), want["pre"], want["b_pre"])) <= 1.0, what
        else:
            C2.check(what + " C2", untouched=True)


@pytest.mark.parametrize("act", SG_ACTS)
@pytest.mark.parametrize("kind", list(SG_EPI_CASES))
def test_sgemm_epilogues(dev, kind, act):
    M, N, K = SG_EPI_CASES[kind]
    S = R.mfma_splits(M, N, K)
    assert (S > 1) == (kind == "reduce")
    e = _Epi(M, N, K, S, dev, seed=K)
    bias_d = _in(e.op["bias"], dev)
    fam = f"sgemm epilogue {kind} act {act}"
    for i, (acc, bias, rm, p) in enumerate(_epilogue_combos()):
        tA, tB = R.FORMS[i % 4]
        ldc = N + (4, 36)[(i // 4) % 2]
        A, lda, B, ldb = e.ab(tA, tB)
        ws = Out(1, S * M * N, S * M * N, dev) if S > 1 else None
        seed = 1000 + i
        what = f"{fam} form {tA}{tB} ldc {ldc} acc {acc} bias {bias} resid {rm} p {p}"
        launch = lambda C, C2, r: _sg(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, acc=acc, bias=bias_d if bias else None, act=act, resid=r, ws=ws,
                                      ws_floats=S * M * N if S > 1 else 0, p=p, seed=seed)
        _check_epilogue(e, launch, act, False, ldc, acc, bias, rm, p, seed, fam, what)
        if ws is not None:
            ws.check(what + " ws")
    _report(fam)


@pytest.mark.parametrize("act,c2", SK_ACTS)
@pytest.mark.parametrize("kind", list(SK_EPI_CASES))
def test_sk_epilogues(dev, kind, act, c2):
    M, N, K = SK_EPI_CASES[kind]
    e = _Epi(M, N, K, R.cdiv(K, R.KC), dev, seed=K + 1)
    bias_d = _in(e.op["bias"], dev)
    fam = f"sk epilogue {kind} act {act}" + (" +C2" if c2 else "")
    _defaults()
    try:
        scrs = {t: Scratch(M, N, K, t, R.SK_GRID_DEFAULT, dev) for t in (1, 2)}
        for t in (1, 2):
            assert all((x == 1) == (kind == "direct") for x in R.sk_plan(M, N, K, t, R.SK_GRID_DEFAULT).contributors)
        for i, (acc, bias, rm, p) in enumerate(_epilogue_combos()):
            tA, tB = R.FORMS[i % 4]
            tile, loop = SK_INSTANCES[(i // 4) % 3]
            ldc = N + (4, 36)[(i // 12) % 2]
            _tune(sk_tile=tile, sk_loop=loop)
            A, lda, B, ldb = e.ab(tA, tB)
            aux = e.padded("aux", ldc) if act == 3 else None
            seed = 2000 + i
            scr = scrs[tile]
            what = f"{fam} form {tA}{tB} tile {tile} loop {loop} ldc {ldc} acc {acc} bias {bias} resid {rm} p {p}"
            # C2 is passed at every act but the plain act 2 row; at act != 2 it must stay untouched
            launch = lambda C, C2, r: _sk(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, scr, c2=C2, acc=acc, bias=bias_d if bias else None, act=act, aux=aux,
                                          resid=r, p=p, seed=seed, by_value_entry=True)
            _check_epilogue(e, launch, act, c2 or act != 2, ldc, acc, bias, rm, p, seed, fam, what)
            scr.check(what)
    finally:
        _defaults()
    _report(fam, fam + " C2")


def test_dropout_seed_from_device_memory_and_across_entries(dev):
    """sfmi_sgemm_sk_sd_f32 with the seed in device memory == the seed by value; csrc/sgemm.hip drops the positions csrc/sgemm_sk.hip
    drops at the same (seed, M, N), which are train_ref.dropout_mul's zeros."""
    M, N, K = SK_EPI_CASES["cut"]
    e = _Epi(M, N, K, R.cdiv(K, R.KC), dev, seed=5)
    ldc, seed, p = N + 4, 0x9E3779B9, 0.5
    zeros = R.dropout_mul(seed, np.arange(M * N, dtype=np.int64).reshape(M, N), p) == 0
    _defaults()
    try:
        for tile, loop in SK_INSTANCES:
            _tune(sk_tile=tile, sk_loop=loop)
            scr = Scratch(M, N, K, tile, R.SK_GRID_DEFAULT, dev)
            for tA, tB in R.FORMS:
                A, lda, B, ldb = e.ab(tA, tB)
                outs = []
                for sd in (None, _u32(seed, dev)):
                    C = Out(M, N, ldc, dev)
                    assert _sk(tA, tB, M, N, K, A, lda, B, ldb, C, ldc, scr, p=p, seed=seed if sd is None else 12345, seed_dev=sd) == 0
                    _sync()
                    outs.append(C.check("seed from device memory"))
                assert _same_bits(outs[0], outs[1]), (tile, loop, tA, tB)
                Cg = Out(M, N, ldc, dev)
                assert _sg(tA, tB, M, N, K, A, lda, B, ldb, Cg, ldc, p=p, seed=seed) == 0
                _sync()
                z0, z1 = (Cg.check("sgemm dropout") == 0).cpu().numpy(), (outs[0] == 0).cpu().numpy()
                assert np.array_equal(z0, zeros) and np.array_equal(z1, zeros), (tile, loop, tA, tB)
    finally:
        _defaults()


# ---------------------------------------------------------------------------------------------------- argument checks
def arg_case(over):
    """BASE_ARGS with one row's overrides applied -> (arguments, extras)"""
    a = dict(BASE_ARGS)
    x = dict(aux=False, A=True, B=True, C=True, slab=True, cnt=True, ws_floats=0, slab_short=0, cnt_short=0)
    for k, v in over.items():
        (a if k in a else x)[k] = v
    return a, x


def arg_expect(name, a, x):
    """(sgemm.hip accepts or None when the row is not its own, stream-K accepts or None) from the mirrors"""
    sg = None if name.startswith("sk ") else R.mfma_accepts(a["tA"], a["tB"], a["M"], a["N"], a["K"], a["lda"], a["ldb"], a["ldc"], a["act"], x["ws_floats"],
                                                            a["drop_p"], x["A"], x["B"], x["C"])
    g = R.sk_geometry(max(a["M"], 1), max(a["N"], 1), max(a["K"], 1), 1, R.SK_GRID_DEFAULT)
    sk = None if name.startswith("sg ") else R.sk_accepts(a["tA"], a["tB"], a["M"], a["N"], a["K"], a["lda"], a["ldb"], a["ldc"], a["act"], x["aux"], a["drop_p"],
                                                          g.slab - x["slab_short"], 4 * g.tiles - x["cnt_short"], 0, R.SK_GRID_DEFAULT, x["A"], x["B"], x["C"],
                                                          x["slab"], x["cnt"])
    return sg, sk


def arg_call(lib, entry, a, x, ptrs, stream):
    """one call of `entry` ('sg' / 'sk') with the row's arguments; ptrs: dict(A, B, C, aux, ws, slab, cnt) of addresses"""
    pa, pb, pc = (ptrs[k] if x[k] else None for k in "ABC")
    if entry == "sg":
        return lib.sfmi_sgemm_mfma_f32(a["tA"], a["tB"], a["M"], a["N"], a["K"], pa, a["lda"], pb, a["ldb"], pc, a["ldc"], 0, None, a["act"], None,
                                       ptrs["ws"], x["ws_floats"], a["drop_p"], 0, stream)
    g = R.sk_geometry(max(a["M"], 1), max(a["N"], 1), max(a["K"], 1), 1, R.SK_GRID_DEFAULT)
    return lib.sfmi_sgemm_sk_f32(a["tA"], a["tB"], a["M"], a["N"], a["K"], pa, a["lda"], pb, a["ldb"], pc, None, a["ldc"], 0, None, a["act"],
                                 ptrs["aux"] if x["aux"] else None, None, a["drop_p"], 0, ptrs["slab"] if x["slab"] else None, g.slab - x["slab_short"],
                                 ptrs["cnt"] if x["cnt"] else None, 4 * g.tiles - x["cnt_short"], stream)


def test_argument_checks_by_return_value(dev):
    """the full table on the device: a refused call returns SFMI_EINVAL and writes nothing, an accepted one returns 0"""
    L = _L()
    _defaults()
    big = 256 * 256
    A, B, aux = (torch.ones(big, device=dev) for _ in range(3))
    for name, over in ARG_TABLE:
        a, x = arg_case(over)
        for entry, ok in zip(("sg", "sk"), arg_expect(name, a, x)):
            if ok is None:
                continue
            C, ws, slab = Out(1, big, big, dev), Out(1, big, big, dev), Out(1, 2 * big, 2 * big, dev)
            cnt = torch.zeros(4096, dtype=torch.int32, device=dev)
            ptrs = dict(A=A.data_ptr(), B=B.data_ptr(), C=C.ptr(), aux=aux.data_ptr(), ws=ws.ptr(), slab=slab.ptr(), cnt=cnt.data_ptr())
            rc = arg_call(L.lib(), entry, a, x, ptrs, L.stream_ptr())
            _sync()
            assert rc == (0 if ok else EINVAL), (name, entry, rc)
            if not ok:
                for o, w in ((C, "C"), (ws, "ws"), (slab, "slab")):
                    o.check(f"{name} {entry} {w}", untouched=True)
            assert not bool(cnt.any()), (name, entry)
