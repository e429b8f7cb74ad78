"""CPU side of the sampler / embedding / row-kernel harness (tests/sampler_ref.py): the exact mirrors against the oracle, the conditions
[DRAW] puts on the inputs (asserted for the reference alone, over the case tables of tests/test_sampler_kernels_gpu.py), the tables'
reach, seeded mutants of the mirror that the reference must refuse, and the monotone bracket itself.  No GPU.

Measured here (pytest -s): at most 3 of a family's 272 .. 320 draws (0.94 %, whole vocabulary at top_p 0.8 / T 1.3) have more than one
accepted token and no set has more than 2; the f32 oracle's draw is a member on every row that does not overflow the 512-candidate
buffer (where the kernel truncates in rank order and the oracle keeps every tie).  Every draw mutant puts 22 .. 100 % of
the draws of its best family outside the accepted sets (printed as `[mutant]` lines; the lowest is the uniform indexed by local row,
which only the launches with a row offset can see); unbiased variance exceeds the LayerNorm bound 97-fold at D = 4096 and 400- to
1e5-fold below; a float32 numpy LayerNorm sits at 0.10 .. 0.19 of it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import sampler_ref as R                                   # noqa: E402
import test_sampler_kernels_gpu as G                      # noqa: E402
from oracle import tokens_oracle as TO                    # noqa: E402

ALL_CASES = [c for fam in G.SAMPLER_FAMILIES for c in fam] + G.TIE_CASES
_cache = {}


def _exp(c, mut=None, oracle=False):
    """inputs and expectation of a case, computed once and shared"""
    key = (c["name"], mut, oracle)
    if key not in _cache:
        if ("inp", c["name"]) not in _cache:
            _cache[("inp", c["name"])] = R.build_sampler_inputs(c)
        _cache[key] = R.sampler_expect(c, _cache[("inp", c["name"])], mut=mut, oracle=oracle)
    return _cache[("inp", c["name"])], _cache[key]


# ---------------------------------------------------------------------------------------------------- exact mirrors against the oracle
def test_mask_mirror_equals_the_oracle_masker():
    n = 0
    for c in ALL_CASES[::3] + [G.OPT_CASE, G.OPT_CASE1]:
        inp, exp = _exp(c)
        x = R.slab_sum(inp["part"])[:, :c["V"]]
        for b in range(c["B"]):
            L, lc = int(inp["len"][b]), int(inp["Lc"][b])
            want = TO.sampling_masker(x[b:b + 1], inp["seq"][b:b + 1, :L + 1], lc, exp[b]["j"], c["tup"], (c["end0"], c["end1"]),
                                      bool(c["inv"]), bool(c["comp"]))[0]
            assert np.array_equal(exp[b]["ml"].view(np.uint32), want.view(np.uint32)), (c["name"], b)
            n += 1
    assert n > 500


def test_extra_index_mirror_equals_the_oracle():
    seq, ln, Lc = R.build_token_rows("cpu/extra", 64, 97, 12)
    end0 = 96
    seen = set()
    for b in range(64):
        lc, L = int(Lc[b]), int(ln[b])
        if L == lc:
            continue
        c_idx, z_idx = seq[b:b + 1, :lc].astype(np.int64), seq[b:b + 1, lc:L].astype(np.int64)
        want = TO.extra_indices_AR_N(c_idx, z_idx, end0)[0, :, 0]
        got = [R.token_extra(seq[b, :, 0], t, lc, end0) for t in range(L)]
        assert list(want) == got, b
        for t in range(lc, L):
            p = int(seq[b, t, 0])
            seen.add("end" if p == end0 else "cond" if p in seq[b, :lc, 0] else "beyond" if p > seq[b, :lc - 1, 0].max(initial=-1) else "between")
    assert seen == {"end", "cond", "beyond", "between"}, seen


def test_the_division_is_correctly_rounded_by_the_build_flags():
    """[DRAW] does not widen the top-p quotients: that needs a correctly rounded f32 division, clang's default for HIP unless one of
    these flags is given."""
    from shapeformer_amd import build as B
    flags = " ".join(B.FLAGS)
    for bad in ("-ffast-math", "-Ofast", "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-funsafe-math", "-freciprocal-math", "-fapprox-func"):
        assert bad not in flags, bad


# ---------------------------------------------------------------------------------------------------- conditions of [DRAW]
@pytest.mark.parametrize("fi", range(len(G.KPT)))
def test_draw_conditions_hold_for_the_family(fi):
    draws = multi = largest = 0
    for c in G.SAMPLER_FAMILIES[fi]:
        inp, exp = _exp(c, oracle=True)
        for b, e in enumerate(exp):
            draws += 1
            multi += len(e["accept"]) > 1
            largest = max(largest, len(e["accept"]))
            assert e["mirror"] in e["accept"], (c["name"], b)
            assert not e["over"]
            if e["oracle"] is not None:
                assert e["oracle"] in e["accept"], (c["name"], b, e["oracle"], e["accept"])
    print(f"[share] k,p,T={G.KPT[fi]}: {multi} of {draws} draws ambiguous ({100.0 * multi / draws:.2f} %), largest set {largest}")
    assert draws >= 250 and multi <= 0.04 * draws and largest <= 8


def test_draw_conditions_hold_for_the_tie_cases():
    for c in G.TIE_CASES:
        inp, exp = _exp(c, oracle=True)
        multi = sum(len(e["accept"]) > 1 for e in exp)
        assert multi <= 0.04 * len(exp) and max(len(e["accept"]) for e in exp) <= 8, c["name"]
        for b, e in enumerate(exp):
            assert e["mirror"] in e["accept"]
            if not e["over"]:          # beyond 512 candidates the kernel truncates in rank order, the oracle keeps every tie
                assert e["oracle"] in e["accept"], (c["name"], b)


# ---------------------------------------------------------------------------------------------------- reach
def test_case_tables_reach_every_path():
    sort_small = sort_big = c1 = c_gt_k = fewer = over = 0
    kinds, vs, ss, sos, ks, ps, ts = set(), set(), set(), set(), set(), set(), set()
    tup1 = set()
    for c in ALL_CASES:
        inp, exp = _exp(c)
        k = R.eff_k(c["kpt"][0], c["V"])
        big = k <= 0 or k > R.SMP_MAXC
        vs.add((c["V"], c["ldv"])); ss.add(c["S"]); sos.add(c["so"]); ks.add(c["kpt"][0]); ps.add(c["kpt"][1]); ts.add(c["kpt"][2])
        for b, e in enumerate(exp):
            kinds.add((c["tup"], inp["kinds"][b], c["inv"], c["comp"]))
            if c["tup"] == 1:
                tup1.add(int(inp["seq"][b, inp["len"][b], 0]) == c["end0"])
            if e["greedy"]:
                continue
            sort_big += big and e["C"] > 1
            sort_small += (not big) and e["C"] > 1
            c1 += e["C"] == 1
            c_gt_k += (not big) and k < e["C"] <= R.SMP_MAXC and not e["over"]
            over += e["over"]
            fewer += k > 0 and e["C"] < min(k, c["V"])
    assert sort_small > 100 and sort_big > 100 and c1 > 20 and c_gt_k > 20 and over > 20 and fewer > 20
    assert vs == set(G.VS) | {(512, 512)} and ss == {1, 2, 3} and sos == {0, 3}
    assert ks >= {1, 2, 100, 511, 512, 513, 0, -5} and ps >= {0.0, 1e-9, 0.4, 0.9, 1.0} and ts == {1.0, 0.7, 1.3, 4.0}
    for kind in R.KINDS0:
        assert any(kk[0] == 0 and kk[1] == kind and kk[2] == 1 for kk in kinds), kind
    assert any(kk[0] == 0 and kk[2] == 0 for kk in kinds) and {kk[3] for kk in kinds if kk[0] == 0} == {0, 1}
    assert tup1 == {True, False}
    # a completion mask with a next condition position, and one with the last position beyond every condition
    nxt = set()
    for c in ALL_CASES:
        if c["tup"] == 0 and c["comp"]:
            inp, _ = _exp(c)
            for b in range(c["B"]):
                L, lc = int(inp["len"][b]), int(inp["Lc"][b])
                nxt.add(bool(np.searchsorted(inp["seq"][b, :lc, 0], inp["seq"][b, L - 1, 0], side="right") < lc))
    assert nxt == {True, False}
    # staged and unstaged position column; every tail; ended rows and packed chains share LIVE_CASES
    assert G.OPT_CASE["Lmax"] <= R.SMP_NPOS < R.SMP_NPOS + 1 and G.OPT_CASE["tup"] == 0 and G.OPT_CASE1["tup"] == 1
    assert all({c["tup"] for c in G.TAIL_CASES[D]} == {0, 1} for D in G.TAIL_D) and G.TAIL_D == [16, 192, 1024]
    assert [c["tup"] for c in G.LIVE_CASES] == [0, 1]
    # rowprep: every branch of the kernel
    forms = {f[0] for f in G.EMBED_FORMS}
    assert forms == {"decode", "rect", "packed", "packed1"}
    assert any(f[3] for f in G.EMBED_FORMS) and any(f[4] for f in G.EMBED_FORMS) and any(not f[4] for f in G.EMBED_FORMS)
    assert {f[1] for f in G.EMBED_FORMS} == {0, 1, 5} and any(f[2] and 0 in f[2] and 1 in f[2] and f[1] in f[2] for f in G.EMBED_FORMS)
    A = G.ACCUM_FORMS
    assert {a[0] for a in A} == {0, 1, 3} and {(a[0], a[1]) for a in A} >= {(1, False), (1, True), (3, False), (3, True)}
    assert any(a[2] for a in A) and any(a[4] for a in A) and any(a[5] and not a[6] for a in A) and any(a[6] and not a[5] for a in A)
    assert any(a[3] for a in A)
    assert G.ROWPREP_D == [4, 64, 1020, 1024, 1028, 4096] and G.ROWPREP_M == [1, 3, 257]


# ---------------------------------------------------------------------------------------------------- mutants
DRAW_MUTANTS = ["tie_desc", "strict_kth", "p_ge", "keep_plus", "keep_minus", "thr_total", "u_local"]


@pytest.mark.parametrize("mut", DRAW_MUTANTS)
def test_draw_mutant_is_refused(mut):
    """At least one family (a (k, p, T) setting, or a tie case) puts at least 5 % of its draws outside the accepted sets."""
    best, where = 0.0, None
    groups = [(f"k,p,T={G.KPT[i]}", fam) for i, fam in enumerate(G.SAMPLER_FAMILIES)] + [(c["name"], [c]) for c in G.TIE_CASES]
    for name, fam in groups:
        out = n = 0
        for c in fam:
            _, ref = _exp(c)
            _, m = _exp(c, mut=mut)
            for e, em in zip(ref, m):
                n += 1
                out += em["mirror"] not in e["accept"]
        if out / n > best:
            best, where = out / n, name
    print(f"[mutant] {mut}: {100 * best:.1f} % of the draws of {where} are refused")
    assert best >= 0.05, (mut, best)


@pytest.mark.parametrize("mut", ["inv_at_j0", "lt_last"])
def test_mask_mutant_is_refused(mut):
    diff = 0
    for c in ALL_CASES[::2]:
        _, ref = _exp(c)
        _, m = _exp(c, mut=mut)
        diff += sum(int((e["ml"].view(np.uint32) != em["ml"].view(np.uint32)).sum()) for e, em in zip(ref, m))
    print(f"[mutant] {mut}: {diff} masked logits differ")
    assert diff > 0


def test_embedding_mutants_are_refused():
    seq, ln, Lc = R.build_token_rows("cpu/emb", 64, 97, 12)
    tb = R.tables("cpu/emb", 97, 64, 12)
    ge = order = 0
    for b in range(64):
        for t in range(int(ln[b])):
            ref, ext = R.embed_rows_ref(tb, seq, int(Lc[b]), 96, b, t)
            ge += R.embed_rows_ref(tb, seq, int(Lc[b]), 96, b, t, mut="ge")[1] != ext
            order += int((R.embed_rows_ref(tb, seq, int(Lc[b]), 96, b, t, mut="order")[0].view(np.uint32) != ref.view(np.uint32)).sum())
    print(f"[mutant] extra index with >=: {ge} indices differ; another summation order: {order} elements differ")
    assert ge > 0 and order > 0


@pytest.mark.parametrize("D", G.ROWPREP_D)
def test_unbiased_variance_exceeds_the_layernorm_bound_tenfold(D):
    rng = np.random.RandomState(D)
    x = R.ln_rows(rng, 8, D)
    g, be = (1 + 0.1 * rng.randn(D)).astype(np.float32), (0.1 * rng.randn(D)).astype(np.float32)
    ref, bound = R.rowln_ref(x, g, be)
    mut, _ = R.rowln_ref(x, g, be, mut="unbiased")
    # an independent float32 LayerNorm sits inside the bound
    x32 = x.astype(np.float32)
    m32 = x32.mean(1, keepdims=True, dtype=np.float32)
    v32 = ((x32 - m32) ** 2).mean(1, keepdims=True, dtype=np.float32)
    f32 = (x32 - m32) / np.sqrt(v32 + np.float32(1e-5)) * g + be
    own = float((np.abs(f32.astype(np.float64) - ref) / bound).max())
    r = float((np.abs(mut - ref) / bound)[[0, 1, 2, 4, 5, 6]].max())          # the constant rows have xhat = 0 under either variance
    print(f"[ratio] rowprep LN D={D}: a float32 numpy LayerNorm {own:.3g}, unbiased variance {r:.3g}")
    assert own <= 1.0 and r >= 10.0


def test_compaction_reference_is_a_stable_partition():
    for B in G.COMPACT_B:
        for pat in G.COMPACT_PATTERNS:
            alen = R.alen_pattern(pat, B, 16)
            Bpad = (B + 15) // 16 * 16
            slot_of, row_of, slot_len, nlive = R.compact_ref(alen, Bpad)
            live = np.nonzero(alen >= 0)[0]
            assert nlive == len(live) and list(row_of[:nlive]) == list(live) and list(row_of[nlive:B]) == list(np.nonzero(alen < 0)[0])
            assert (row_of[B:] == -1).all() and (slot_len[nlive:] == -1).all() and list(slot_len[:nlive]) == list(alen[live])
            assert all(slot_of[b] == (list(live).index(b) if alen[b] >= 0 else -1) for b in range(B))


# ---------------------------------------------------------------------------------------------------- the bracket
def test_running_sums_stay_inside_the_monotone_bracket():
    """Exps perturbed anywhere inside [e_lo, e_hi] and summed sequentially in f32 stay between the two bracketing cumsums; numpy's
    own f32 exp is such a perturbation."""
    rng = np.random.RandomState(0)
    for n, sc in ((4097, 3.0), (512, 1.0), (4352, 0.01), (100, 10.0)):
        for trial in range(4):
            xs = np.sort((rng.randn(n) * sc).astype(np.float32))[::-1].copy()
            lo, hi = R.exp_bracket(xs)
            cs_lo, cs_hi = np.cumsum(lo, dtype=np.float32), np.cumsum(hi, dtype=np.float32)
            assert (lo <= hi).all() and (cs_lo <= cs_hi).all() and lo[0] == hi[0] == 1.0
            e32 = np.exp((xs - xs[0]).astype(np.float32)).astype(np.float32)
            assert (lo <= e32).all() and (e32 <= hi).all()
            for e in (e32, lo + (hi - lo) * rng.rand(n).astype(np.float32), np.where(rng.rand(n) < 0.5, lo, hi)):
                e = np.clip(e.astype(np.float32), lo, hi)
                cs = np.cumsum(e, dtype=np.float32)
                assert (cs_lo <= cs).all() and (cs <= cs_hi).all()
            acc = np.float32(0)                                          # np.cumsum adds one after the other, as the kernel does
            for i in range(64):
                acc = np.float32(acc + e32[i])
                assert acc == np.cumsum(e32, dtype=np.float32)[i]
