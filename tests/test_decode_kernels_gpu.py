"""The decode-step kernels of csrc/gpt.hip against float64 (tests/decode_ref.py: references and derived per-element error bounds) at
every launch form the launchers can reach:

* dgemm_kernel through sfmi_decode_gemm_f32: every instance decode_gemm_launch instantiates (asserted with decode_ref.dgemm_form
  against the DG* macro list), M 1..192 in one and several row groups, K-slices of every NW (16 / 8 / 4 / 1), split-K with S not a
  multiple of 4, packed and row-major output (ldo > N), LayerNorm fold through the production path (sfmi_ln_fold_pack_f32) with
  rows of |mean|/std 0, 3, 30 and a constant row, GELU, c2, residual and residual aliasing the output (proj / fc2, gpt.py
  decode_step).  Per launch: the [GEMM] bound, the split-K tickets re-armed, guard bands after the slab / ticket / output buffers
  untouched, rows >= M and columns >= round_up(N, 4) of a row-major output untouched, a second launch bit-identical.
* attn_decode_kernel through sfmi_gpt_attn_decode_gated_f32: head dims 4..64, ragged lengths 1..1024, 1..192 rows, a row whose
  scores span more than 60 and a row of equal keys, the shared-prefix instance against the expanded cache, the prefill ->
  decode KV-cache contract.
* the launch-shape knobs (csrc/sfmi_common.h): the ones documented as result-preserving bit for bit, the others within the bound.

Measured on one MI355X (largest error / bound over all launches of a family; printed as `[ratio] ...` lines with pytest -s): decode
GEMM 0.18 (LayerNorm rows: |mean|/std = 30 at most 0.09, 0.013 at K = 4096; the constant row 0.05 - the one-pass variance stays well
inside its derived budget), decode attention 0.06, prefill attention 0.04."""
import contextlib
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import decode_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
SENT = 0x7FC0DEAD          # NaN bit pattern of every "must stay untouched" float
CSENT = 0x5A5A5A5A         # the same for ints
GUARD = 1024               # guard-band elements after every buffer a kernel writes
LOGIT_TOL = 1e-3           # model-level logits tolerance of the project (tests/test_gpt_gpu.py, SURVEY App.B)


def _L():
    from shapeformer_amd import _lib as L
    return L


def _sent(n, dev):
    return torch.full((n,), SENT, dtype=torch.int32, device=dev).view(torch.float32)


def _is_sent(t):
    return t.contiguous().view(torch.int32) == SENT


def _bits(t):
    return t.contiguous().view(torch.int32)


@contextlib.contextmanager
def _knobs(**kv):
    """sfmi_tune_set for the duration; every knob restored in a finally (as tests/test_gpt_gpu.py does)."""
    L = _L()
    lib = L.lib()
    old = {k: int(lib.sfmi_tune_get(k.encode())) for k in kv}
    try:
        for k, v in kv.items():
            L.check(lib.sfmi_tune_set(k.encode(), int(v)), k)
        yield
    finally:
        for k, v in old.items():
            L.check(lib.sfmi_tune_set(k.encode(), v), k)


def _report(family, what, ratio):
    print(f"[ratio] {family} {what}: {ratio:.3g}")


# ---------------------------------------------------------------------------------------------------- decode GEMM
MS = [1, 5, 16, 17, 47, 48, 80, 96, 97, 130, 191, 192]
KS = [(1024, 1), (1024, 2), (1024, 4), (1024, 8), (4096, 1), (4096, 2), (1280, 5), (192, 1), (192, 3), (576, 1), (576, 3),
      (48, 1), (48, 3), (96, 1), (96, 2), (96, 3)]


def _base_cases(ki):
    """(M, N, packed, ldo, ln, act, c2, resid, alias) for every M at KS[ki]: the epilogue variants rotate over the rows."""
    out = []
    for i, M in enumerate(MS):
        ln, act = (i + ki) % 2, ((i + ki) // 2) % 2
        use_c2 = bool(ln) or i % 3 != 0
        use_res = i % 4 in (1, 2)
        packed = i % 6 != 5
        N, ldo = (48, 48) if packed else ((50, 56) if (i // 6 + ki) % 2 == 0 else (4097, 4104))
        out.append((M, N, int(packed), ldo, ln, act, use_c2, use_res, use_res and packed and i % 4 == 2))
    return out


# knob sweeps: each shape runs the default and every combination below; forms of one NW must agree bit for bit (same k order, same
# chains, same wave and slice sums), every NW is checked against the bound
KNOB_SHAPES = [(1, 1024, 1), (17, 4096, 1), (47, 1024, 1), (97, 4096, 2), (80, 1024, 4), (192, 1024, 1), (16, 384, 1),
               (80, 192, 1), (130, 96, 1), (97, 1024, 1), (60, 1024, 1), (33, 4096, 1)]
KNOB_SETS = ([{"dgemm_un": u} for u in range(1, 9)] + [{"dgemm_prio": p} for p in (1, 2, 3)]
             + [{"dgemm_nt2": n, "dgemm_un": u} for n in (0, 2) for u in (0, 1, 3)]
             + [{"dgemm_nw": w, "dgemm_un": u, "dgemm_nt2": n} for w in (4, 8, 16) for u in (0, 1, 2) for n in (0, 1)])


def _form(M, K, S, kn):
    return R.dgemm_form(M, K, S, {k: v for k, v in kn.items() if k in R.DGEMM_DEFAULT_KNOBS})


def test_dgemm_cases_reach_every_instance():
    """The launches of this file reach every dgemm_kernel instance of decode_gemm_launch (dgemm_form mirrors its rule)."""
    seen = set()
    for ki, (K, S) in enumerate(KS):
        for M, *_ in _base_cases(ki):
            seen.add(R.dgemm_form(M, K, S)[:4])
    for M, K, S in KNOB_SHAPES:
        for kn in [{}] + KNOB_SETS:
            seen.add(_form(M, K, S, kn)[:4])
    assert sorted(seen) == R.DGEMM_INSTANCES, sorted(set(R.DGEMM_INSTANCES) - seen)


class _Gemm:
    """Inputs, float64 reference and bound of one decode-GEMM shape; launch() runs it under the current knobs and checks the
    launch-level invariants."""

    def __init__(self, dev, M, K, S, N=48, packed=1, ldo=48, ln=0, act=0, use_c2=True, use_res=False, alias=False, seed=0):
        L = _L()
        lib = L.lib()
        g = torch.Generator().manual_seed(seed)
        self.dev, self.M, self.K, self.S, self.N, self.packed, self.ln, self.act, self.alias = dev, M, K, S, N, packed, ln, act, alias
        self.ldo = N if packed else ldo
        self.Mp = int(lib.sfmi_decode_gemm_padded_rows(M))
        Np = (N + 15) // 16 * 16
        x = torch.randn(M, K, generator=g)
        if ln:      # LayerNorm stress rows: |mean|/std = 0, 3, 30 and a constant row (var = 0)
            x[1::4] += 3.0
            x[2::4] += 30.0
            x[3::4] = 0.3
        self.kind = torch.arange(M) % 4 if ln else torch.zeros(M, dtype=torch.long)
        W = torch.randn(N, K, generator=g) * 0.05
        self.x, self.W = x, W
        self.xp = R.pack(x, self.Mp).to(dev)
        resid = torch.randn(M, N, generator=g) if use_res else None
        if ln:
            gam, bet, bias = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g), torch.randn(N, generator=g)
            Wd, gd, bd, biasd = (t.to(dev) for t in (W, gam, bet, bias))
            self.wp, self.c1, self.c2 = (torch.empty(Np * K, device=dev), torch.empty(Np, device=dev), torch.empty(Np, device=dev))
            L.check(lib.sfmi_ln_fold_pack_f32(L.ptr(Wd), L.ptr(gd), L.ptr(bd), L.ptr(biasd), L.ptr(self.wp), L.ptr(self.c1),
                                              L.ptr(self.c2), N, K, L.stream_ptr()), "sfmi_ln_fold_pack_f32")
            torch.cuda.synchronize()
            self.ref = R.ln_linear_ref(x, W, gam, bet, bias, act, resid)
            self.lnp = (gam, bet, bias, self.c1.cpu()[:N], resid)
        else:
            self.wp, self.c1 = R.pack(W).to(dev), None
            c2 = torch.randn(Np, generator=g) if use_c2 else None
            self.c2 = c2.to(dev) if c2 is not None else None
            self.ref = R.ln_linear_ref(x, W, bias=c2[:N] if c2 is not None else None, act=act, resid=resid)
            self.plain = (c2, resid)
        self.out_len = self.Mp * (N if packed else self.ldo)
        init = torch.full((self.out_len + GUARD,), SENT, dtype=torch.int32).view(torch.float32)
        if use_res:
            if packed:
                rb = R.pack(resid, self.Mp)
            else:
                rb = _sent(self.Mp * self.ldo, "cpu").view(self.Mp, self.ldo)
                rb[:M, :N] = resid
                rb = rb.reshape(-1)
            if alias:
                init[:self.out_len] = rb
                self.res_dev = None
            else:
                self.res_dev = rb.to(dev)
        else:
            self.res_dev = None
        self.init = init
        self.use_res = use_res
        self._bounds = {}

    def bound(self, NW):
        if NW not in self._bounds:
            n = R.dgemm_depth(self.K, self.S, NW)
            if self.ln:
                gam, bet, bias, c1, resid = self.lnp
                self._bounds[NW] = R.dgemm_ln_bound(self.x, self.W, gam, bet, bias, c1, self.act, resid, n,
                                                    R.dgemm_stats_depth(self.K, self.S, NW))
            else:
                c2, resid = self.plain
                self._bounds[NW] = R.dgemm_plain_bound(self.x, self.W, c2, self.act, resid, n)
        return self._bounds[NW]

    def launch(self, kn=None):
        """One launch under the current knobs (kn: the values set, for dgemm_form).  Returns (out (M, N) f32, form)."""
        L = _L()
        lib = L.lib()
        M, K, S, N = self.M, self.K, self.S, self.N
        form = _form(M, K, S, kn or {})
        NT, MT, NW, UN, groups = form
        ncnt = groups * MT * ((N + 15) // 16)
        nslab = int(lib.sfmi_decode_gemm_slab_floats(M, N, S))
        slab = _sent(nslab + GUARD, self.dev)
        cnt = torch.full((ncnt + GUARD,), CSENT, dtype=torch.int32, device=self.dev)
        cnt[:ncnt] = 0
        out = self.init.to(self.dev)
        res = out if self.alias else self.res_dev
        L.check(lib.sfmi_decode_gemm_f32(L.ptr(self.xp), L.ptr(self.wp), L.ptr(self.c1) if self.ln else None, L.ptr(self.c2),
                                         L.ptr(res), L.ptr(out), M, N, K, self.ldo, self.ln, self.act, self.packed, S,
                                         L.ptr(slab) if S > 1 else None, L.ptr(cnt) if S > 1 else None, L.stream_ptr()),
                "sfmi_decode_gemm_f32")
        torch.cuda.synchronize()
        out, slab, cnt = out.cpu(), slab.cpu(), cnt.cpu()
        what = (M, K, S, N, form)
        assert bool((cnt[:ncnt] == 0).all()), f"split-K tickets not re-armed {what}"
        assert bool((cnt[ncnt:] == CSENT).all()), f"ticket index beyond groups * MT * ntiles {what}"
        if S > 1:
            assert bool(_is_sent(slab[nslab:]).all()), f"slab written beyond sfmi_decode_gemm_slab_floats {what}"
        assert bool(_is_sent(out[self.out_len:]).all()), f"output written beyond its padded rows {what}"
        if self.packed:
            got = R.unpack(out[:self.out_len], M, N)
        else:
            grid, ginit = out[:self.out_len].view(self.Mp, self.ldo), self.init[:self.out_len].view(self.Mp, self.ldo)
            assert torch.equal(_bits(grid[M:]), _bits(ginit[M:])), f"row-major rows >= M written {what}"
            n4 = (N + 3) // 4 * 4
            assert torch.equal(_bits(grid[:M, n4:]), _bits(ginit[:M, n4:])), f"row-major columns >= round_up(N, 4) written {what}"
            got = grid[:M, :N].clone()
        return got, form

    def check(self, got, form, tag):
        ratio_el = (got.double() - self.ref).abs() / self.bound(form[2])
        assert bool(torch.isfinite(got).all()), (tag, form)
        ratio = float(ratio_el.max())
        assert ratio <= 1.0, f"{tag} {form}: error / bound {ratio:.3g} at {np.unravel_index(int(ratio_el.argmax()), ratio_el.shape)}"
        if self.ln:
            for k, name in enumerate(("ln mean/std=0", "ln mean/std=3", "ln mean/std=30", "ln const row")):
                rows = self.kind == k
                if bool(rows.any()):
                    _report("dgemm", f"{name} K={self.K}", float(ratio_el[rows].max()))
        return ratio


@pytest.mark.parametrize("ki", range(len(KS)), ids=[f"K{K}_S{S}" for K, S in KS])
def test_decode_gemm_vs_float64(dev, ki):
    """Every M of the grid at one (K, S), default knobs: the [GEMM] bound and the launch invariants; a second launch is
    bit-identical."""
    K, S = KS[ki]
    worst = 0.0
    for j, (M, N, packed, ldo, ln, act, use_c2, use_res, alias) in enumerate(_base_cases(ki)):
        c = _Gemm(dev, M, K, S, N, packed, ldo, ln, act, use_c2, use_res, alias, seed=1000 * ki + j)
        got, form = c.launch()
        worst = max(worst, c.check(got, form, f"M={M} N={N} packed={packed} ln={ln} act={act} c2={use_c2} res={use_res} alias={alias}"))
        again, _ = c.launch()
        assert torch.equal(_bits(again), _bits(got)), ("second launch differs", M, K, S)
    _report("dgemm", f"K={K} S={S}", worst)


@pytest.mark.parametrize("M,K,S", KNOB_SHAPES)
def test_decode_gemm_knobs(dev, M, K, S):
    """dgemm_un (every value), dgemm_prio and dgemm_nt2 keep every result bit (sfmi_common.h); dgemm_nw changes the wave split of
    K, so its results are held to the float64 bound only - but forms with the same NW agree bit for bit."""
    ln = (M + K) % 2
    c = _Gemm(dev, M, K, S, 48, 1, 48, ln, 1 - ln, True, True, alias=True, seed=M * 7 + K)
    base, form0 = c.launch()
    by_nw = {form0[2]: base}
    worst = c.check(base, form0, "default")
    for kn in KNOB_SETS:
        with _knobs(**kn):
            got, form = c.launch(kn)
        nw = form[2]
        if nw in by_nw:
            assert torch.equal(_bits(got), _bits(by_nw[nw])), f"knobs {kn} ({form}) change result bits of the NW={nw} form"
        else:
            by_nw[nw] = got
            worst = max(worst, c.check(got, form, f"knobs {kn}"))
    _report("dgemm", f"knobs M={M} K={K} S={S}", worst)


# ---------------------------------------------------------------------------------------------------- decode attention
TS = [0, 1, 63, 64, 255, 256, 257, 812, 1023]


class _Attn:
    """One decode-attention step: caches holding each row's history (positions < t), NaN-sentinel everywhere else."""

    def __init__(self, dev, B, H, HD, Lmax, seed, nshared=0, stress=True):
        g = torch.Generator().manual_seed(seed)
        ts = [t for t in TS if t < Lmax]
        t = [max(ts)] + [ts[(b * 5 + 3) % len(ts)] for b in range(1, B)]      # row 0 the longest (the shared-prefix owner)
        self.dev, self.B, self.H, self.HD, self.Lmax, self.t, self.nshared = dev, B, H, HD, Lmax, t, nshared
        D = H * HD
        self.D, self.Bp = D, (B + 15) // 16 * 16
        q, kn, vn = (torch.randn(B, H, HD, generator=g) for _ in range(3))
        Kh, Vh = torch.randn(B, H, Lmax, HD, generator=g), torch.randn(B, H, Lmax, HD, generator=g)
        if stress and B >= 3:
            b1 = 1 if t[1] >= 255 else 0                                    # a long row whose scores span more than 60
            q[b1] *= 4.0
            Kh[b1] *= 4.0
            kn[b1] *= 4.0
            Kh[2] = kn[2][:, None, :]                                        # all keys of row 2 equal
            self.span_row = b1
        self.q, self.kn, self.vn = q, kn, vn
        K0 = torch.full((B, H, Lmax, HD), SENT, dtype=torch.int32).view(torch.float32)
        V0 = K0.clone()
        for b in range(B):
            lo = min(nshared, t[b]) if b > 0 else 0      # shared positions of rows > 0 are never read: NaN proves it
            K0[b, :, lo:t[b]], V0[b, :, lo:t[b]] = Kh[b, :, lo:t[b]], Vh[b, :, lo:t[b]]
        self.K0, self.V0 = K0, V0
        qkv = torch.cat([q.reshape(B, D), kn.reshape(B, D), vn.reshape(B, D)], 1)
        self.qkv = R.pack(qkv, self.Bp).to(dev)
        self.len = torch.tensor([x + 1 for x in t], dtype=torch.int32, device=dev)
        self.shared = torch.tensor([nshared], dtype=torch.int32, device=dev)
        self._ref = {}

    def ref(self, nwv):
        if nwv not in self._ref:
            self._ref[nwv] = R.decode_attn_ref(self.q, self.kn, self.vn, self.K0, self.V0, [x + 1 for x in self.t], self.nshared, nwv)
        return self._ref[nwv]

    def launch(self, shared=None):
        L = _L()
        lib = L.lib()
        n = self.K0.numel()
        Kc, Vc = _sent(n + GUARD, self.dev), _sent(n + GUARD, self.dev)
        Kc[:n], Vc[:n] = self.K0.reshape(-1).to(self.dev), self.V0.reshape(-1).to(self.dev)
        y = _sent(self.Bp * self.D + GUARD, self.dev)
        L.check(lib.sfmi_gpt_attn_decode_gated_f32(L.ptr(self.qkv), L.ptr(Kc), L.ptr(Vc), L.ptr(self.len), L.ptr(y), self.B, self.D,
                                                   self.H, self.Lmax, L.ptr(self.shared) if shared else None, None, None, 0, None,
                                                   L.stream_ptr()), "sfmi_gpt_attn_decode_gated_f32")
        torch.cuda.synchronize()
        Kc, Vc, y = Kc.cpu(), Vc.cpu(), y.cpu()
        for name, C, C0, new in (("K", Kc, self.K0, self.kn), ("V", Vc, self.V0, self.vn)):
            assert bool(_is_sent(C[n:]).all()), f"{name} cache written beyond (B, H, Lmax, HD)"
            C = C[:n].view(self.B, self.H, self.Lmax, self.HD)
            want = C0.clone()
            for b in range(self.B):
                want[b, :, self.t[b]] = new[b]
            assert torch.equal(_bits(C), _bits(want)), f"{name} cache: position t must hold the new {name}, every other position its old bits"
        assert bool(_is_sent(y[self.Bp * self.D:]).all()) and bool(_is_sent(R.unpack(y[:self.Bp * self.D], self.Bp, self.D)[self.B:]).all()), \
            "y written beyond its B rows"
        return R.unpack(y[:self.Bp * self.D], self.B, self.D).view(self.B, self.H, self.HD)

    def check(self, y, nwv, tag):
        ref, bound = self.ref(nwv)
        assert bool(torch.isfinite(y).all()), tag
        r = (y.double() - ref).abs() / bound
        ratio = float(r.max())
        assert ratio <= 1.0, f"{tag}: error / bound {ratio:.3g} at {np.unravel_index(int(r.argmax()), r.shape)} (t = {self.t})"
        return ratio


@pytest.mark.parametrize("HD,B,Lmax", [(4, 17, 1024), (16, 3, 813), (32, 96, 1024), (60, 17, 813), (64, 1, 1024), (64, 192, 1024),
                                       (16, 192, 813), (64, 17, 813)])
def test_decode_attention_vs_float64(dev, HD, B, Lmax):
    """Ragged lengths t + 1 in one launch (t in 0 .. 1023), head dims 4..64 (H = 4), the stress rows: [ATTN] bound, the new k / v at
    position t and nothing else written, padded rows of y untouched."""
    a = _Attn(dev, B, 4, HD, Lmax, seed=HD * 100 + B)
    if B >= 3:
        b1, t1 = a.span_row, a.t[a.span_row]
        K = torch.cat([a.K0[b1, :, :t1], a.kn[b1, :, None]], 1).double()
        s = torch.einsum("hd,htd->ht", a.q[b1].double(), K) / math.sqrt(HD)
        assert float((s.max(1).values - s.min(1).values).max()) > 60, "the stress row must span more than 60 in the scores"
    ratio = a.check(a.launch(), 16, f"HD={HD} B={B} Lmax={Lmax}")
    _report("attn", f"HD={HD} B={B} Lmax={Lmax}", ratio)


@pytest.mark.parametrize("HD,B", [(64, 17), (32, 5)])
def test_decode_attention_shared_prefix(dev, HD, B):
    """The shared-prefix instance (positions < shared_len from row 0's cache) against the expanded-cache reference; shared_len = 0 is
    bit-identical to the plain instance (csrc/gpt.hip attn_decode_item)."""
    worst = 0.0
    plain = _Attn(dev, B, 4, HD, 1024, seed=HD + B)
    y_plain = plain.launch()
    worst = max(worst, plain.check(y_plain, 16, "plain"))
    y0 = plain.launch(shared=True)                    # shared_len = 0
    assert torch.equal(_bits(y0), _bits(y_plain)), "shared instance with shared_len = 0 differs from the plain instance"
    ts = plain.t
    for ns in (1, min(ts), min(x for x in ts if x > 1), max(ts)):
        a = _Attn(dev, B, 4, HD, 1024, seed=HD + B, nshared=ns)
        worst = max(worst, a.check(a.launch(shared=True), 16, f"shared_len={ns}"))
    _report("attn", f"shared prefix HD={HD} B={B}", worst)


@pytest.mark.parametrize("HD", [64, 32])
def test_decode_attention_knobs(dev, HD):
    """attn_unroll, attn_blocks (persistent grid) and attn_lds_pad keep every bit (a lane meets its keys in the same order); attn_waves
    8 / 4 sum in another order and are held to the bound for their wave count."""
    B, H = 17, 4
    a = _Attn(dev, B, H, HD, 1024, seed=HD)
    base = a.launch()
    worst = a.check(base, 16, "default")
    for kn in [{"attn_unroll": 2}, {"attn_unroll": 8}, {"attn_blocks": 1}, {"attn_blocks": 5}, {"attn_blocks": B * H - 1},
               {"attn_blocks": B * H + 3}, {"attn_lds_pad": 16384}, {"attn_blocks": 5, "attn_unroll": 8}]:
        with _knobs(**kn):
            y = a.launch()
        assert torch.equal(_bits(y), _bits(base)), f"{kn} changes result bits"
    for waves, unrolls in ((8, (2, 4, 8)), (4, (8, 16))):
        first = None
        for u in unrolls:
            with _knobs(attn_waves=waves, attn_unroll=u):
                y = a.launch()
            worst = max(worst, a.check(y, waves, f"attn_waves={waves} attn_unroll={u}"))
            if first is None:
                first = y
            assert torch.equal(_bits(y), _bits(first)), f"attn_unroll changes result bits at attn_waves={waves}"
        with _knobs(attn_waves=waves, attn_unroll=unrolls[0], attn_blocks=7):
            assert torch.equal(_bits(a.launch()), _bits(first)), f"attn_blocks changes result bits at attn_waves={waves}"
    _report("attn", f"knobs HD={HD}", worst)


@pytest.mark.parametrize("HD", [16, 32, 64])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130])
def test_prefill_then_decode_kv_contract(dev, HD, P):
    """sfmi_gpt_attn_prefill_f32 over P positions (ragged nval) fills the caches the decode step reads: the prefill output against
    float64 causal attention, the cache rows equal to the projected k / v, then one decode step at t = nval[b] against float64
    attention over the nval[b] + 1 positions built from the original projections (not from the cache)."""
    L = _L()
    lib = L.lib()
    B, H, Lmax = 3, 2, 256
    D = H * HD
    g = torch.Generator().manual_seed(P * 10 + HD)
    nval = [P, max(1, P // 2), 1]
    qkv = torch.randn(B, P, 3, H, HD, generator=g)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))            # (B, H, P, HD)
    n = B * H * Lmax * HD
    Kc, Vc = _sent(n + GUARD, dev), _sent(n + GUARD, dev)
    y = _sent(B * P * D + GUARD, dev)
    nv = torch.tensor(nval, dtype=torch.int32, device=dev)
    qkv_d = qkv.reshape(B * P, 3 * D).to(dev)
    L.check(lib.sfmi_gpt_attn_prefill_f32(L.ptr(qkv_d), L.ptr(Kc), L.ptr(Vc), L.ptr(nv), L.ptr(y), B, P, D,
                                          H, Lmax, None, 0.0, 0, L.stream_ptr()), "sfmi_gpt_attn_prefill_f32")
    torch.cuda.synchronize()
    yc, bound = R.causal_attn_ref(q, k, v, nval)
    yg = y[:B * P * D].cpu().view(B, P, H, HD).permute(0, 2, 1, 3)
    Kh, Vh = Kc[:n].cpu().view(B, H, Lmax, HD), Vc[:n].cpu().view(B, H, Lmax, HD)
    worst = 0.0
    for b in range(B):
        nb = nval[b]
        r = (yg[b, :, :nb].double() - yc[b, :, :nb]).abs() / bound[b, :, :nb]
        worst = max(worst, float(r.max()))
        assert bool(torch.isfinite(yg[b, :, :nb]).all()) and float(r.max()) <= 1.0, ("prefill", b, float(r.max()))
        assert torch.equal(Kh[b, :, :nb], k[b, :, :nb]) and torch.equal(Vh[b, :, :nb], v[b, :, :nb]), "prefill cache rows"
        assert bool(_is_sent(Kh[b, :, nb:]).all()) and bool(_is_sent(Vh[b, :, nb:]).all()), "prefill wrote cache rows >= nval"
    _report("prefill", f"HD={HD} P={P}", worst)
    # one decode step at t = nval[b]
    qn, kn, vn = (torch.randn(B, H, HD, generator=g) for _ in range(3))
    Bp = 16
    step = R.pack(torch.cat([qn.reshape(B, D), kn.reshape(B, D), vn.reshape(B, D)], 1), Bp).to(dev)
    ln_ = torch.tensor([x + 1 for x in nval], dtype=torch.int32, device=dev)
    yd = _sent(Bp * D, dev)
    L.check(lib.sfmi_gpt_attn_decode_gated_f32(L.ptr(step), L.ptr(Kc), L.ptr(Vc), L.ptr(ln_), L.ptr(yd), B, D, H, Lmax, None, None, None,
                                               0, None, L.stream_ptr()), "sfmi_gpt_attn_decode_gated_f32")
    torch.cuda.synchronize()
    Kref = torch.zeros(B, H, Lmax, HD)
    Vref = torch.zeros(B, H, Lmax, HD)
    for b in range(B):
        Kref[b, :, :nval[b]], Vref[b, :, :nval[b]] = k[b, :, :nval[b]], v[b, :, :nval[b]]
    want, bd = R.decode_attn_ref(qn, kn, vn, Kref, Vref, [x + 1 for x in nval])
    got = R.unpack(yd.cpu(), B, D).view(B, H, HD)
    r = float(((got.double() - want).abs() / bd).max())
    assert bool(torch.isfinite(got).all()) and r <= 1.0, ("decode after prefill", r)
    _report("attn", f"after prefill HD={HD} P={P}", r)


# ---------------------------------------------------------------------------------------------------- narrow models end to end
@pytest.mark.parametrize("n_embd", [192, 96])
def test_narrow_models_sample_80_rows(dev, n_embd):
    """n_embd 192 (K-slices of 64: NW = 4) and 96 (K-slices of 32: NW = 1) with 80 rows (five row tiles: more than those forms have
    instances for in one row group) run the whole sampling loop, and the first step's masked logits of every row match the CPU oracle
    (oracle/gpt_oracle.py) within the project's model-level logits tolerance."""
    from oracle import gpt_oracle as GO, vqdif_oracle as VO
    from shapeformer_amd import weights as W
    from shapeformer_amd.gpt import CondTupleGPT
    kw = dict(n_embd=n_embd, n_layers=(2, 1), block_size=96)
    sd = W.make_state_dict(W.gpt_spec(**kw))
    g = CondTupleGPT(sd, n_head=3, device=dev, **kw)
    B, Lc = 80, 12
    rs = np.random.RandomState(n_embd)
    c = np.full((B, Lc, 2), 4096, np.int32)
    for b in range(B):
        c[b, :Lc - 1, 0] = np.sort(rs.choice(4096, Lc - 1, replace=False))
        c[b, :Lc - 1, 1] = rs.randint(0, 4096, Lc - 1)
    out = g.sample(torch.from_numpy(c), torch.full((B,), Lc, dtype=torch.int32), max_steps=2, seed=3, stop_early=False,
                   return_logits=True)
    got = out["samples"].numpy()
    hist = [h.numpy() for h in out["logits_history"]]
    assert got.shape == (B, 2, 2)
    cfg = GO.GPTCfg(n_embd=n_embd, n_head=3, n_layers=(2, 1), block_size=96)
    _, oh, _ = GO.sample_indices(VO.to_torch_sd(sd), cfg, torch.from_numpy(c).long(), 2, GO.uniforms(3, 2, B), use_cache=True,
                                 stop_early=False, force_tokens=got, best_in_first=True)
    for i in range(2):
        a, r = hist[i][:, 0], oh[i][:, 0]
        fin = np.isfinite(r)
        assert np.array_equal(np.isfinite(a), fin), f"mask differs, tuple {i}"
        err = float(np.abs(a[fin] - r[fin]).max())
        assert err < LOGIT_TOL, (n_embd, i, err)
