"""The decode step's sampler, embedding and row kernels of csrc/gpt.hip (and ar_n_extra_kernel of csrc/tokens.hip) against
tests/sampler_ref.py, every launch through the C ABI and every written buffer between sentinel bands:

* sample_kernel through sfmi_gpt_sample_f32 / _live_f32 / _rows_f32 / sfmi_gpt_mask_logits_f32: the masks, the slab sum, the candidate
  set and order (both sort paths, C = 1, ties at the k-th value, more than 512 candidates), the draw as a member of the accepted set
  of [DRAW], the log-probability under [LOGP], history, forcing, the greedy row, the seed by value and in device memory, micro-batches,
  the staged and unstaged position column, both embedding tails, ended rows and packed chains.
* rowprep_kernel through sfmi_gpt_embed_f32 and sfmi_gpt_rowprep_f32: the embedding and the residual sum in bits, the LayerNorm under
  [RLN]; embed_packed_kernel in both layouts; sfmi_ar_n_extra_i32 on the same rows; compact_rows_kernel; sfmi_set_len_i32.
* every SFMI_EINVAL refusal of these launchers, by return value.

The case tables below are plain data: tests/test_sampler_ref_cpu.py imports them, asserts the conditions [DRAW] puts on them and runs
the seeded mutants over them.

Measured on one MI355X (pytest -s; largest error / bound over all launches of a family, printed as `[ratio] ...` lines): sampler
log-probability 0.21 .. 0.33 over the twelve (top_k, top_p, T) families, 0.18 .. 0.24 over the tie cases (0.005 on all-equal rows),
0.32 with history and forcing; rowprep LayerNorm 0.11 .. 0.19 over D = 4 .. 4096 (rows of |mean| / std = 30: at most 0.14, constant rows
0.18).  Share of draws with more than one accepted token (`[share] ...` lines): 0 of 272 .. 320 in ten families, 3 of 320 (0.94 %) at
(0, 0.8, 1.3) and 1 of 272 (0.37 %) at (V + 5, 0.9, 1.3); the kernel's token was a member every time.  Rows over 512 candidates in the
tie cases: 6, 19, 8, 57 and 61 of 64, truncated in rank order and bit-identical over two launches.  The file takes 3.2 s."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import sampler_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu
SENT = 0x7FC0DEAD          # NaN bit pattern of every "must stay untouched" float
CSENT = 0x5A5A5A5A         # the same for ints
GUARD = 1024               # guard-band elements on either side of every buffer a kernel writes
EINVAL = -1

# ---------------------------------------------------------------------------------------------------- case tables (plain data)
# (top_k, top_p, T); top_k = -n stands for V + n.  Sort paths: top_k in 1 .. 512 takes the rank sort, 0 / 513 / V + 5 the bitonic network.
KPT = [(100, 0.4, 1.0), (300, 0.9, 1.0), (50, 0.0, 0.7), (0, 0.8, 1.3), (0, 0.0, 1.0), (512, 0.0, 1.0), (512, 0.95, 1.0), (513, 0.0, 1.0),
       (1, 0.0, 1.0), (2, 1.0, 4.0), (511, 1e-9, 1.0), (-5, 0.9, 1.3)]
VS = [(1, 1), (2, 4), (255, 256), (256, 256), (257, 264), (4097, 4128), (4352, 4352)]        # (V, ldv)
LOGITS = ["n3", "n1", "n001"]


def _family(i):
    """The launches of KPT[i]: the product vocabulary twice, every other vocabulary / slab count / tuple in rotation."""
    kpt = KPT[i]
    va, vb = VS[i % 7], VS[(i + 3) % 7]
    return [
        dict(name=f"k{i}/a", V=4097, ldv=4128, S=1 + i % 3, tup=0, kpt=kpt, logits=LOGITS[i % 3], so=(0, 3)[i % 2], comp=1),
        dict(name=f"k{i}/b", V=va[0], ldv=va[1], S=1 + (i + 1) % 3, tup=1, kpt=kpt, logits="n3", B=64 if va[0] > 2 else 16),
        dict(name=f"k{i}/c", V=vb[0], ldv=vb[1], S=1 + (i + 2) % 3, tup=0, kpt=kpt, logits="n1", so=(3, 0)[i % 2], comp=i % 2, inv=int(i % 4 != 3),
             B=64 if vb[0] > 2 else 16),
        dict(name=f"k{i}/d", V=4097, ldv=4128, S=1, tup=0, kpt=kpt, logits="n3", comp=(i + 1) % 2, kinds=("mid", "j0", "mid", "mid"),
             row_offset=7, rows_total=64 + 7 + 9),
        dict(name=f"k{i}/e", V=4352, ldv=4352, S=1, tup=1, kpt=kpt, logits=LOGITS[(i + 1) % 3], kinds=("cur",)),
    ]


SAMPLER_FAMILIES = [[R.case_defaults(c) for c in _family(i)] for i in range(len(KPT))]

# ties: logits are multiples of 0.5 (every 8th row all equal); each launch runs twice and must repeat in bits
TIE_CASES = [R.case_defaults(c) for c in [
    dict(name="tie/flat100", V=4097, ldv=4128, S=2, kpt=(100, 0.0, 1.0), logits="tieflat", kinds=("j0", "mid")),       # k < C <= 512
    dict(name="tie/flat300p", V=4097, ldv=4128, S=1, kpt=(300, 0.9, 1.0), logits="tieflat", kinds=("j0", "mid")),
    dict(name="tie/n3_100", V=4097, ldv=4128, S=3, kpt=(100, 0.4, 1.0), logits="tie3", kinds=("j0", "mid")),
    dict(name="tie/over512", V=4097, ldv=4128, S=1, kpt=(512, 0.0, 1.0), logits="tieflat", kinds=("j0", "mid")),       # C > 512: truncation
    dict(name="tie/over511p", V=4352, ldv=4352, S=1, kpt=(511, 0.95, 1.0), logits="tieflat", kinds=("j0", "mid")),
    dict(name="tie/big0", V=4097, ldv=4128, S=1, kpt=(0, 0.0, 1.0), logits="tie3", kinds=("j0", "mid")),               # bitonic path
    dict(name="tie/big513p", V=257, ldv=264, S=2, kpt=(513, 0.8, 1.3), logits="tieflat", kinds=("j0", "mid")),
    dict(name="tie/tup1", V=4097, ldv=4128, S=1, tup=1, kpt=(100, 0.0, 0.7), logits="tieflat"),
    # equal logits, 512 candidates: the softmax cumsum is (i + 1) / 512 exactly and meets top_p = 0.75 exactly at i = 383 (`>` keeps going)
    dict(name="tie/eq_p", V=512, ldv=512, S=1, kpt=(512, 0.75, 1.0), logits="tieeq", kinds=("j0",), B=32),
    dict(name="tie/eq_p_big", V=512, ldv=512, S=1, kpt=(0, 0.75, 1.3), logits="tieeq", kinds=("j0",), B=32),
]]

OPT_CASE = R.case_defaults(dict(name="opt", V=4097, ldv=4128, S=2, kpt=(100, 0.4, 1.0), logits="n3", so=0, comp=1, B=16))
OPT_CASE1 = R.case_defaults(dict(name="opt1", V=4097, ldv=4128, S=1, tup=1, kpt=(100, 0.4, 1.0), logits="n3", B=16))
MB_CASE = R.case_defaults(dict(name="mb", V=4097, ldv=4128, S=1, kpt=(300, 0.0, 1.3), logits="n1", B=8, greedy0=1))
TAIL_D = [16, 192, 1024]
TAIL_CASES = {D: [R.case_defaults(dict(name=f"tail{D}/{t}", V=V, ldv=V + 7, S=1, tup=t, kpt=(100, 0.4, 1.0), logits="n3", B=20))
                  for t in (0, 1)] for D, V in zip(TAIL_D, (4097, 300, 257))}
LIVE_CASES = [R.case_defaults(dict(name=f"live/{t}", V=300, ldv=304, S=1, tup=t, kpt=(50, 0.9, 1.0), logits="n3", B=24,
                                   kinds=("mid", "end") if t == 0 else ("cur", "curend", "cur"))) for t in (0, 1)]

ROWPREP_D = [4, 64, 1020, 1024, 1028, 4096]
ROWPREP_M = [1, 3, 257]
# mode 0 (embedding): (form, P, nval per row or None, explicit extra, extra_out)
EMBED_FORMS = [("decode", 0, None, False, True), ("rect", 1, (0, 1), False, True), ("rect", 5, (0, 1, 5), False, False),
               ("rect", 5, None, True, True), ("packed", 5, None, False, True), ("packed1", 5, None, False, False)]
# mode 1 (accumulate): (S or 0 for part == NULL, bias, Eadd, P, alias, xn, resid_out)
ACCUM_FORMS = [(0, False, False, 0, False, True, True), (1, False, False, 0, True, True, True), (1, True, False, 0, False, True, True),
               (3, False, False, 0, False, True, True), (3, True, True, 0, True, True, True), (3, True, False, 0, False, True, False),
               (1, False, True, 0, False, False, True), (3, True, True, 4, True, True, True)]
EMBED_PACKED_D = [16, 1024]
COMPACT_B = [1, 16, 17, 96, 255, 256]
COMPACT_PATTERNS = ["all", "none", "alt", "last", "random"]
COMPACT_D = [16, 1024]
SETLEN_B = [1, 63, 64, 65]
SETLEN_DELTA = [-1, 0, 2]


# ---------------------------------------------------------------------------------------------------- helpers
def _L():
    from shapeformer_amd import _lib as L
    return L


class Band:
    """A device buffer between two sentinel bands; .t is the payload view."""

    def __init__(self, dev, init=None, n=None, dtype=torch.float32):
        if init is not None:
            init = torch.as_tensor(np.ascontiguousarray(init)) if isinstance(init, np.ndarray) else init
            n, dtype = init.numel(), init.dtype
        self.n, self.isf = n, dtype == torch.float32
        self.full = torch.full((n + 2 * GUARD,), SENT if self.isf else CSENT, dtype=torch.int32, device=dev)
        self.t = self.full[GUARD:GUARD + n].view(dtype)
        if init is not None:
            self.t.copy_(init.reshape(-1).to(dev))

    def ptr(self):
        return self.t.data_ptr()

    def np(self, shape=None):
        assert bool((self.full[:GUARD] == (SENT if self.isf else CSENT)).all()) and \
            bool((self.full[GUARD + self.n:] == (SENT if self.isf else CSENT)).all()), "guard band written"
        a = self.t.cpu().numpy()
        return a.reshape(shape) if shape is not None else a


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _is_sent(a):
    return _bits(a) == SENT


def _sub(c, inp, lo, hi):
    """rows lo .. hi-1 of a case as a micro-batch of the same global batch"""
    c2 = dict(c, B=hi - lo, row_offset=c["row_offset"] + lo, rows_total=c["rows_total"])
    i2 = dict(part=np.ascontiguousarray(inp["part"][:, lo:hi]), seq=inp["seq"][lo:hi].copy(), len=inp["len"][lo:hi].copy(),
              Lc=inp["Lc"][lo:hi].copy(), kinds=inp["kinds"][lo:hi])
    return c2, i2


def _run(dev, c, inp, entry="plain", logp=True, hist=False, force=None, advance=1, D=0, tb=None, resid=None, seed_dev=False,
         alen=None, skip=1, slot_of=None, part=None, nslots=None):
    """One sampler launch.  resid: (rows, D) row-major initial residual (packed here).  Returns the buffers as numpy."""
    L = _L()
    lib = L.lib()
    B, V, ms = c["B"], c["V"], c["max_steps"]
    k = R.eff_k(c["kpt"][0], V)
    d = {}
    bpart = Band(dev, init=inp["part"] if part is None else part)
    bseq, blen = Band(dev, init=inp["seq"]), Band(dev, init=inp["len"])
    bLc = torch.from_numpy(inp["Lc"]).to(dev)
    blogp = Band(dev, n=B * ms * 2) if logp else None
    bhist = Band(dev, n=B * ms * V) if hist else None
    dforce = torch.from_numpy(np.ascontiguousarray(force, np.int32)).to(dev) if force is not None else None
    bres = bstage = None
    tbd = [None] * 4
    if D:
        rows = resid.shape[0]
        bres = Band(dev, init=R.pack(torch.from_numpy(np.ascontiguousarray(resid)), (rows + 15) // 16 * 16))
        tbd = [torch.from_numpy(t).to(dev) for t in tb[:4]]
        if entry == "rows":
            bstage = Band(dev, n=B * D)
    dseed = torch.tensor([c["seed"]], dtype=torch.int64).to(torch.int32).to(dev) if seed_dev else None
    balen = Band(dev, init=np.ascontiguousarray(alen, np.int32)) if alen is not None else None
    dslot = torch.from_numpy(np.ascontiguousarray(slot_of, np.int32)).to(dev) if slot_of is not None else None
    p = L.ptr
    seed_val = 0xDEADBEEF if seed_dev else c["seed"]
    common = [D, c["S"], B, V, c["ldv"], c["Lmax"], c["tup"], c["end0"], c["end1"], k, float(c["kpt"][1]), float(c["kpt"][2]), c["greedy0"]]
    tailargs = [seed_val, p(dseed), advance, c["row_offset"], c["rows_total"], c["so"]]
    if entry == "rows":
        rc = lib.sfmi_gpt_sample_rows_f32(bpart.ptr(), bseq.ptr(), blen.ptr(), p(bLc), blogp.ptr() if logp else None, bres.ptr(), bstage.ptr(),
                                          *[p(t) for t in tbd], *common, c["comp"], ms, *tailargs, balen.ptr(), p(dslot), L.stream_ptr())
    else:
        head = [bpart.ptr(), bseq.ptr(), blen.ptr(), p(bLc), blogp.ptr() if logp else None, bhist.ptr() if hist else None, p(dforce),
                bres.ptr() if D else None, *[p(t) for t in tbd], *common, c["inv"], c["comp"], ms, *tailargs]
        if entry == "live":
            rc = lib.sfmi_gpt_sample_live_f32(*head, balen.ptr() if balen else None, skip, L.stream_ptr())
        else:
            rc = lib.sfmi_gpt_sample_f32(*head, L.stream_ptr())
    L.check(rc, "sample " + c["name"])
    torch.cuda.synchronize()
    d["seq"], d["len"] = bseq.np(inp["seq"].shape), blen.np()
    assert _same_bits(bpart.np(), (inp["part"] if part is None else part).reshape(-1)), "logits written"
    if logp:
        d["logp"] = blogp.np((B, ms, 2))
    if hist:
        d["hist"] = bhist.np((B, ms, V))
    if D:
        rows = resid.shape[0]
        d["resid"] = R.unpack(torch.from_numpy(bres.np()), rows, D).numpy()
        if bstage is not None:
            d["stage"] = bstage.np((B, D))
    if balen is not None:
        d["alen"] = balen.np()
    return d


def _check(c, inp, exp, out, advance=1, force=None, stats=None, hist=False, ended=None):
    """Everything a sampler launch owes its row: the token (a member of the accepted set), seq otherwise untouched, len, the
    log-probability slot under [LOGP] (bits +0.0f where the token is the only finite logit), the history slot in bits, every other
    slot still the sentinel.  Returns the largest logp error / bound."""
    B, tup, ms = c["B"], c["tup"], c["max_steps"]
    worst = 0.0
    want_seq = inp["seq"].copy()
    for b in range(B):
        e, Lb = exp[b], int(inp["len"][b])
        tok = int(out["seq"][b, Lb, tup])
        j_in = 0 <= e["j"] < ms
        if ended is not None and ended[b]:
            assert tok == (c["end1"] if tup else c["end0"]), (c["name"], b, tok)
            ref, bound, only = 0.0, 0.0, True
        else:
            if force is not None:         # forcing makes the row greedy; beyond the forced steps the arg-max itself is written
                assert tok == (int(force[b, e["j"], tup]) if j_in else int(np.argmax(e["ml"]))), (c["name"], b)
            else:
                assert tok in e["accept"], (c["name"], b, tok, e["accept"], e["keeps"], e["C"])
                if stats is not None:
                    stats["draws"] += 1
                    stats["multi"] += int(len(e["accept"]) > 1)
            ref, bound = R.logp_ref(e["ml"], tok)
            only = np.isfinite(e["ml"]).sum() == 1 and np.isfinite(e["ml"][tok])
        want_seq[b, Lb, tup] = tok
        assert int(out["len"][b]) == Lb + (1 if advance else 0), (c["name"], b)
        if "logp" in out:
            lp = out["logp"][b]
            mask = np.ones((ms, 2), bool)
            if j_in:
                mask[e["j"], tup] = False
                got = lp[e["j"], tup]
                if only:
                    assert _bits(got) == 0, (c["name"], b, got)
                elif ref == -np.inf:
                    assert got == -np.inf, (c["name"], b, got)
                else:
                    r = abs(float(got) - ref) / bound
                    worst = max(worst, r)
                    assert r <= 1.0, (c["name"], b, float(got), ref, bound)
            assert _is_sent(lp[mask]).all(), (c["name"], b, "logp slot of another step written")
        if hist:
            h = out["hist"][b]
            for s in range(ms):
                if j_in and s == e["j"]:
                    assert _same_bits(h[s], e["ml"]), (c["name"], b, "history")
                else:
                    assert _is_sent(h[s]).all(), (c["name"], b, s, "history slot of another step written")
    assert np.array_equal(out["seq"], want_seq), (c["name"], "seq written beyond the token")
    return worst


def _report(what, ratio):
    print(f"[ratio] {what}: {ratio:.3g}")


# ---------------------------------------------------------------------------------------------------- sampler: the (k, p, T) table
@pytest.mark.parametrize("fi", range(len(KPT)))
def test_sampler_family(dev, fi):
    """Every launch of one (top_k, top_p, T) family: tokens inside the accepted set, log-probabilities under [LOGP], nothing else written."""
    stats, worst = dict(draws=0, multi=0), 0.0
    for c in SAMPLER_FAMILIES[fi]:
        inp = R.build_sampler_inputs(c)
        exp = R.sampler_expect(c, inp)
        out = _run(dev, c, inp)
        worst = max(worst, _check(c, inp, exp, out, stats=stats))
    _report(f"sampler logp k,p,T={KPT[fi]}", worst)
    print(f"[share] sampler k,p,T={KPT[fi]}: {stats['multi']} of {stats['draws']} draws have more than one accepted token "
          f"({100.0 * stats['multi'] / max(stats['draws'], 1):.2f} %)")


@pytest.mark.parametrize("ci", range(len(TIE_CASES)))
def test_sampler_ties_repeat_in_bits_and_follow_the_rank_order(dev, ci):
    """Ties at the k-th value, inside the order, all-equal rows and more than 512 candidates: the token is a member of the accepted
    set of the rank-ordered (and, beyond 512, rank-truncated) candidates, and a second launch gives the same bits."""
    c = TIE_CASES[ci]
    inp = R.build_sampler_inputs(c)
    exp = R.sampler_expect(c, inp)
    a = _run(dev, c, inp)
    b = _run(dev, c, inp)
    worst = _check(c, inp, exp, a)
    assert np.array_equal(a["seq"], b["seq"]) and _same_bits(a["logp"], b["logp"]) and np.array_equal(a["len"], b["len"])
    _report(f"sampler logp {c['name']}", worst)
    print(f"[ties] {c['name']}: candidates {min(e['C'] for e in exp)} .. {max(e['C'] for e in exp)}, rows over 512: {sum(e['over'] for e in exp)}")


def test_sampler_history_forcing_advance_and_seed(dev):
    """hist is written at step j only and equals the mask in bits; a forced token is written and its log-probability taken under the
    mask (-inf where it is masked); advance = 0 leaves len; the seed in device memory gives the bits of the seed by value."""
    for c in (OPT_CASE, OPT_CASE1):
        inp = R.build_sampler_inputs(c)
        exp = R.sampler_expect(c, inp)
        base = _run(dev, c, inp, hist=True)
        w = _check(c, inp, exp, base, hist=True)
        noadv = _run(dev, c, inp, advance=0)
        _check(c, inp, exp, noadv, advance=0)
        sd = _run(dev, c, inp, seed_dev=True)
        assert np.array_equal(sd["seq"], base["seq"]) and _same_bits(sd["logp"], base["logp"]) and np.array_equal(noadv["seq"], base["seq"])
        rng = np.random.RandomState(5)
        force = rng.randint(0, c["V"], (c["B"], c["max_steps"], 2)).astype(np.int32)
        force[::3, :, c["tup"]] = c["end0"]           # tuple 0: never masked by mask_invalid
        fo = _run(dev, c, inp, force=force, hist=True)
        w = max(w, _check(c, inp, exp, fo, force=force, hist=True))
        masked = sum(1 for b in range(c["B"]) if 0 <= exp[b]["j"] < c["max_steps"]
                     and not np.isfinite(exp[b]["ml"][force[b, exp[b]["j"], c["tup"]]]))
        assert masked > 0 or c["tup"] == 1
        _report(f"sampler logp {c['name']} (history, forcing)", w)


def test_sampler_greedy_row_and_micro_batches(dev):
    """Row 0 of the first micro-batch is greedy and no other row is; rows 0..2 and 3..7 as two micro-batches of 8 give one launch's bits."""
    c = MB_CASE
    inp = R.build_sampler_inputs(c)
    exp = R.sampler_expect(c, inp)
    assert exp[0]["greedy"] and not any(e["greedy"] for e in exp[1:])
    one = _run(dev, c, inp)
    _check(c, inp, exp, one)
    seqs, lps = [], []
    for lo, hi in ((0, 3), (3, 8)):
        c2, i2 = _sub(c, inp, lo, hi)
        o = _run(dev, c2, i2)
        _check(c2, i2, exp[lo:hi], o)
        seqs.append(o["seq"]); lps.append(o["logp"])
    assert np.array_equal(np.concatenate(seqs), one["seq"]) and _same_bits(np.concatenate(lps), one["logp"])
    # the same rows without the greedy flag: row 0 draws like every other row
    c3 = dict(c, greedy0=0)
    exp3 = R.sampler_expect(c3, inp)
    _check(c3, inp, exp3, _run(dev, c3, inp))
    assert len(exp3[0]["accept"]) == 1 and exp3[0]["accept"][0] != exp[0]["accept"][0], "row 0 must tell the greedy token from the drawn one"


def test_sampler_staged_and_unstaged_positions_agree(dev):
    """Lmax 1040 (position column staged in LDS) and 1041 (read from memory): same bits."""
    outs = []
    for c in (OPT_CASE, OPT_CASE1):
        for Lmax in (R.SMP_NPOS, R.SMP_NPOS + 1):
            c2 = dict(c, Lmax=Lmax)
            inp = R.build_sampler_inputs(c2)
            exp = R.sampler_expect(c2, inp)
            o = _run(dev, c2, inp)
            _check(c2, inp, exp, o)
            outs.append((o["seq"][:, :64], o["logp"]))
        assert np.array_equal(outs[-1][0], outs[-2][0]) and _same_bits(outs[-1][1], outs[-2][1])


# ---------------------------------------------------------------------------------------------------- sampler: tails, ended rows, packed chains
def _tail_expect(c, inp, tb, resid, toks, rows=None):
    """the residual after the tail, row-major: tuple 0 adds E0[token]; tuple 1 writes the completed token's embedding"""
    want = resid.copy()
    for b in range(c["B"]) if rows is None else rows:
        Lb, lc = int(inp["len"][b]), int(inp["Lc"][b])
        if c["tup"] == 0:
            want[b] = (resid[b] + tb[0][toks[b]]).astype(np.float32)
        else:
            pos = int(inp["seq"][b, Lb, 0])
            ext = int(R.ar_n_extra(inp["seq"][b, :lc, 0], np.array([pos]), c["end0"])[0])
            want[b] = R.emb_ref(tb[0], tb[1], tb[2], tb[3][Lb - lc], pos, toks[b], ext)
    return want


@pytest.mark.parametrize("D", TAIL_D)
def test_sampler_tails(dev, D):
    """Tuple 0: resid[pk_off(row)] += E0[token]; tuple 1: the completed token's embedding; other rows and the bands untouched."""
    for c in TAIL_CASES[D]:
        inp = R.build_sampler_inputs(c)
        exp = R.sampler_expect(c, inp)
        tb = R.tables(c["name"], c["V"], D, c["Lmax"])
        B = c["B"]
        resid = np.random.RandomState(D).randn(32, D).astype(np.float32)            # rows 20 .. 31 belong to nobody
        out = _run(dev, c, inp, D=D, tb=tb, resid=resid)
        _check(c, inp, exp, out)
        toks = [int(out["seq"][b, inp["len"][b], c["tup"]]) for b in range(B)]
        assert _same_bits(out["resid"], _tail_expect(c, inp, tb, resid, toks)), c["name"]


@pytest.mark.parametrize("tup", [0, 1])
def test_sample_live_ended_rows(dev, tup):
    """sfmi_gpt_sample_live_f32: a row with alen < 0 carries NaN logits and still gets the forced token, log-probability bits 0, len + 1
    and (tuple 1) a zeroed residual; a row that completes an end0 token at tuple 1 gets alen = -1, every other row len; with a
    history, forcing or mask_invalid = 0 the skip is disarmed and alen follows len."""
    c = LIVE_CASES[tup]
    D = 64
    inp = R.build_sampler_inputs(c)
    exp = R.sampler_expect(c, inp)
    tb = R.tables(c["name"], c["V"], D, c["Lmax"])
    B = c["B"]
    ended = np.zeros(B, bool)
    ended[2::5] = True
    alen = np.where(ended, -1, inp["len"]).astype(np.int32)
    part = inp["part"].copy()
    part[:, ended] = np.nan
    resid = np.random.RandomState(3).randn(32, D).astype(np.float32)
    out = _run(dev, c, inp, entry="live", D=D, tb=tb, resid=resid, alen=alen, part=part)
    _check(c, inp, exp, out, ended=ended)
    toks = [int(out["seq"][b, inp["len"][b], tup]) for b in range(B)]
    want = _tail_expect(c, inp, tb, resid, toks, rows=[b for b in range(B) if not ended[b]])
    if tup == 1:
        want[:B][ended] = 0.0
    assert _same_bits(out["resid"], want)
    for b in range(B):
        if ended[b]:
            assert out["alen"][b] == -1
        else:
            ends = tup == 1 and int(inp["seq"][b, inp["len"][b], 0]) == c["end0"]
            assert out["alen"][b] == (-1 if ends else inp["len"][b] + 1), (b, out["alen"][b])
    if tup == 1:
        assert any(out["alen"][b] == -1 and not ended[b] for b in range(B))
    # the plain entry gives the live rows' bits
    plain = _run(dev, c, inp)
    live = ~ended
    assert np.array_equal(plain["seq"][live], out["seq"][live]) and _same_bits(plain["logp"][live], out["logp"][live])
    # advance = 0 leaves alen alone
    na = _run(dev, c, inp, entry="live", alen=alen, part=part, advance=0)
    assert np.array_equal(na["alen"], alen)
    # disarmed: finite logits everywhere, every row is sampled and alen == len afterwards
    rng = np.random.RandomState(9)
    force = rng.randint(0, c["V"], (B, c["max_steps"], 2)).astype(np.int32)
    for kw, c2 in ((dict(hist=True), c), (dict(force=force), c), (dict(), dict(c, inv=0)), (dict(skip=0), c)):
        exp2 = exp if c2 is c else R.sampler_expect(c2, inp)
        o = _run(dev, c2, inp, entry="live", alen=alen, **kw)
        _check(c2, inp, exp2, o, force=kw.get("force"), hist=bool(kw.get("hist")))
        assert np.array_equal(o["alen"], inp["len"] + 1), kw


@pytest.mark.parametrize("tup", [0, 1])
def test_sample_rows_packed_chain(dev, tup):
    """sfmi_gpt_sample_rows_f32 with a non-identity slot map: logits and the tuple-0 residual at the slot, the tuple-1 embedding to
    stage[row]; seq, len, alen and logp keyed by row and bit-equal to the _live launch on the unpermuted rows."""
    c = LIVE_CASES[tup]
    D = 64
    inp = R.build_sampler_inputs(c)
    exp = R.sampler_expect(c, inp)
    tb = R.tables(c["name"], c["V"], D, c["Lmax"])
    B = c["B"]
    ended = np.zeros(B, bool)
    ended[[0, 3, 4, 11, 23]] = True
    alen = np.where(ended, -1, inp["len"]).astype(np.int32)
    slot_of, row_of, _, nlive = R.compact_ref(alen, 32)
    assert not np.array_equal(slot_of[~ended], np.arange(B)[~ended]) and (slot_of == -1).sum() == ended.sum()
    part = inp["part"].copy()
    part[:, ended] = np.nan
    part_slots = np.full_like(part, np.nan)
    part_slots[:, slot_of[~ended]] = part[:, ~ended]
    resid = np.random.RandomState(4).randn(32, D).astype(np.float32)                # by slot
    out = _run(dev, c, inp, entry="rows", D=D, tb=tb, resid=resid, alen=alen, part=part_slots, slot_of=slot_of)
    _check(c, inp, exp, out, ended=ended)
    resid_rows = np.zeros_like(resid)
    resid_rows[:B][~ended] = resid[slot_of[~ended]]
    live = _run(dev, c, inp, entry="live", D=D, tb=tb, resid=resid_rows, alen=alen, part=part)
    assert np.array_equal(out["seq"], live["seq"]) and _same_bits(out["logp"], live["logp"])
    assert np.array_equal(out["len"], live["len"]) and np.array_equal(out["alen"], live["alen"])
    toks = [int(out["seq"][b, inp["len"][b], tup]) for b in range(B)]
    if tup == 0:
        want = resid.copy()
        for b in np.nonzero(~ended)[0]:
            want[slot_of[b]] = (resid[slot_of[b]] + tb[0][toks[b]]).astype(np.float32)
        assert _same_bits(out["resid"], want)
        assert _is_sent(out["stage"]).all()
    else:
        assert _same_bits(out["resid"], resid), "a packed chain's tuple-1 tail writes the staging buffer only"
        rows = [b for b in range(B) if not ended[b]]
        want = _tail_expect(c, inp, tb, np.zeros((B, D), np.float32), toks, rows=rows)
        assert _same_bits(out["stage"][~ended], want[~ended])
        assert _is_sent(out["stage"][ended]).all()


@pytest.mark.parametrize("tup", [0, 1])
def test_mask_logits_equals_history_and_reference(dev, tup):
    """sfmi_gpt_mask_logits_f32: bit-equal to the reference (and so to the sampler's history); seq and len untouched."""
    L = _L()
    for c in ([OPT_CASE, SAMPLER_FAMILIES[2][2], SAMPLER_FAMILIES[3][2]] if tup == 0 else [OPT_CASE1, SAMPLER_FAMILIES[1][1]]):
        c = dict(c, so=0, S=1)
        inp = R.build_sampler_inputs(c)
        exp = R.sampler_expect(c, inp)
        B, V = c["B"], c["V"]
        bseq, blen, bout = Band(dev, init=inp["seq"]), Band(dev, init=inp["len"]), Band(dev, n=B * V)
        dpart, dLc = torch.from_numpy(inp["part"][0]).to(dev), torch.from_numpy(inp["Lc"]).to(dev)
        L.check(L.lib().sfmi_gpt_mask_logits_f32(L.ptr(dpart), bseq.ptr(), blen.ptr(), L.ptr(dLc), bout.ptr(), B, V, c["ldv"], c["Lmax"], tup,
                                                 c["end0"], c["end1"], c["inv"], c["comp"], L.stream_ptr()), "mask_logits")
        torch.cuda.synchronize()
        assert _same_bits(bout.np((B, V)), np.stack([e["ml"] for e in exp])), c["name"]
        assert np.array_equal(bseq.np(inp["seq"].shape), inp["seq"]) and np.array_equal(blen.np(), inp["len"])
        h = _run(dev, c, inp, hist=True)
        for b in range(B):
            if 0 <= exp[b]["j"] < c["max_steps"]:
                assert _same_bits(h["hist"][b, exp[b]["j"]], bout.np((B, V))[b])


# ---------------------------------------------------------------------------------------------------- rowprep
def _embed_launch(dev, tb, seq, ln, Lc, D, Lmax, end0, B, P, nval, extra, want_extra, rowoff, M, xn=True, resid=True):
    L = _L()
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tbd = [d(t) for t in tb]
    rng = np.random.RandomState(D + M)
    gam, bet = (1 + 0.1 * rng.randn(D)).astype(np.float32), (0.1 * rng.randn(D)).astype(np.float32)
    bres, bxn = (Band(dev, n=M * D) if resid else None), (Band(dev, n=M * D) if xn else None)
    bex = Band(dev, n=M, dtype=torch.int32) if want_extra else None
    keep = [d(seq), d(ln), d(Lc), d(nval), d(extra), d(gam), d(bet), d(rowoff)]
    L.check(L.lib().sfmi_gpt_embed_f32(*[L.ptr(t) for t in tbd], *[L.ptr(t) for t in keep[:5]], bex.ptr() if bex else None,
                                       bres.ptr() if bres else None, bxn.ptr() if bxn else None, L.ptr(keep[5]), L.ptr(keep[6]), B, P, D, Lmax,
                                       end0, L.ptr(keep[7]), M if rowoff is not None else 0, L.stream_ptr()), "embed")
    torch.cuda.synchronize()
    return (bres.np((M, D)) if bres else None, bxn.np((M, D)) if bxn else None, bex.np() if bex else None, gam, bet)


def _embed_case(D, form, P, nvals, explicit, Mwant):
    """-> seq, len, Lc, nval, extra, rowoff, B, M, Lmax, V, rows [(b, t)]"""
    V, Lmax = 97, 12
    if form == "decode":
        B = Mwant
    elif form == "rect":
        B = max(1, -(-Mwant // P))
    elif form == "packed1":
        B = 1
    else:
        B = max(2, Mwant // 3)
    seq, ln, Lc = R.build_token_rows(f"embed/{D}/{form}/{P}/{Mwant}", B, V, Lmax)
    nval = None if nvals is None else np.array([nvals[b % len(nvals)] for b in range(B)], np.int32)
    rowoff = None
    M = B * P if P else B
    if form.startswith("packed"):
        cnt = np.array([1 if (b % 3 == 1 or form == "packed1") else 1 + (b * 7) % P for b in range(B)], np.int32)     # ragged, one-row sequences
        cnt = np.minimum(cnt, ln)
        rowoff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        M = int(rowoff[-1])
        nval = cnt.copy()
    extra = None
    if explicit:
        extra = np.random.RandomState(D).randint(0, V, (B, Lmax)).astype(np.int32)
    rows = R.rowprep_rows(P, B, nval, Lc, rowoff, M)
    if not P:
        rows = [(b, int(ln[b]) - 1) for b in range(B)]
    return seq, ln, Lc, nval, extra, rowoff, B, M, Lmax, V, rows


@pytest.mark.parametrize("D", ROWPREP_D)
def test_rowprep_embedding(dev, D):
    """rowprep_kernel mode 0 through sfmi_gpt_embed_f32: every form of EMBED_FORMS at M of ROWPREP_M; the embedding and the extra
    index in bits, the LayerNorm under [RLN], a launch with only xn and one with only resid_out."""
    worst = 0.0
    for fi, (form, P, nvals, explicit, want_extra) in enumerate(EMBED_FORMS):
        for Mwant in ROWPREP_M:
            if Mwant == 257 and (D > 1028 or fi % 2):
                Mwant = 40                                               # the many-block launch once per form pair and width class
            seq, ln, Lc, nval, extra, rowoff, B, M, Lmax, V, rows = _embed_case(D, form, P, nvals, explicit, Mwant)
            tb = R.tables(f"embed/{D}", V, D, Lmax)
            only = (fi + Mwant) % 3            # 0: both outputs, 1: xn only, 2: resid_out only
            res, xn, ex, gam, bet = _embed_launch(dev, tb, seq, ln, Lc, D, Lmax, V - 1, B, P, nval, extra, want_extra, rowoff, M,
                                                  xn=only != 2, resid=only != 1)
            want = np.zeros((M, D), np.float32)
            wex = np.zeros(M, np.int32)
            for m, (b, t) in enumerate(rows):
                want[m], wex[m] = R.embed_rows_ref(tb, seq, int(Lc[b]), V - 1, b, t, extra)
            if res is not None:
                assert _same_bits(res, want), (D, form, P, Mwant)
            if ex is not None:
                assert np.array_equal(ex, wex), (D, form, P, Mwant)
            if xn is not None:
                ref, bound = R.rowln_ref(want, gam, bet)
                r = float((np.abs(xn.astype(np.float64) - ref) / bound).max())
                worst = max(worst, r)
                assert r <= 1.0, (D, form, P, Mwant, r)
    _report(f"rowprep LN (embedding, D={D})", worst)


@pytest.mark.parametrize("D", ROWPREP_D)
def test_rowprep_accumulate(dev, D):
    """rowprep_kernel mode 1 through sfmi_gpt_rowprep_f32: resid + sum of slabs + bias + Eadd[next position] in bits, resid_out
    aliasing resid_in, the LayerNorm under [RLN] on rows of |mean| / std 0, 3, 30 and a constant row."""
    L = _L()
    worst, kinds = 0.0, [0.0] * 4
    for fi, (S, bias, eadd, P, alias, want_xn, want_res) in enumerate(ACCUM_FORMS):
        for M in ROWPREP_M:
            if M == 257 and (D > 1028 or fi % 2):
                M = 40
            if P:
                M = -(-M // P) * P
            B = M // P if P else M
            rng = np.random.RandomState(D * 31 + fi * 7 + M)
            V, Lmax = 50, 10
            x = R.ln_rows(rng, M, D)
            part = (rng.randn(S, M, D) * 0.01).astype(np.float32) if S else None
            bv = (rng.randn(D) * 0.01).astype(np.float32) if bias else None
            E = (rng.randn(V, D) * 0.01).astype(np.float32) if eadd else None
            seq = rng.randint(0, V, (B, Lmax, 2)).astype(np.int32)
            ln = rng.randint(1, Lmax - 1, B).astype(np.int32)
            nval = rng.randint(0, P + 1, B).astype(np.int32) if P else None
            gam, bet = (1 + 0.1 * rng.randn(D)).astype(np.float32), (0.1 * rng.randn(D)).astype(np.float32)
            d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            bin_ = Band(dev, init=x)
            bres = bin_ if alias else (Band(dev, n=M * D) if want_res else None)
            bxn = Band(dev, n=M * D) if want_xn else None
            keep = [d(part), d(bv), d(E), d(seq), d(ln), d(nval), d(gam), d(bet)]
            L.check(L.lib().sfmi_gpt_rowprep_f32(bin_.ptr(), *[L.ptr(t) for t in keep[:5]], None, L.ptr(keep[5]), bres.ptr() if bres else None,
                                                 bxn.ptr() if bxn else None, L.ptr(keep[6]), L.ptr(keep[7]), max(S, 1), M, P, D, Lmax, None, B,
                                                 L.stream_ptr()), "rowprep")
            torch.cuda.synchronize()
            rows = R.rowprep_rows(P, B, nval, np.zeros(B, np.int32), None, M) if P else [(b, int(ln[b]) - 1) for b in range(B)]
            erow = np.stack([E[seq[b, t + 1, 0]] for b, t in rows]) if eadd else None
            want = R.accum_ref(x, part, bv, erow)
            if bres is not None:
                assert _same_bits(bres.np((M, D)), want), (D, fi, M)
            if not alias:
                assert _same_bits(bin_.np((M, D)), x), "resid_in written"
            if bxn is not None:
                ref, bound = R.rowln_ref(want, gam, bet)
                rr = np.abs(bxn.np((M, D)).astype(np.float64) - ref) / bound
                for kq in range(4):
                    if rr[kq::4].size:
                        kinds[kq] = max(kinds[kq], float(rr[kq::4].max()))
                worst = max(worst, float(rr.max()))
                assert rr.max() <= 1.0, (D, fi, M, float(rr.max()))
    _report(f"rowprep LN (accumulate, D={D})", worst)
    print(f"[ratio] rowprep LN D={D} by |mean|/std 0, 3, 30, constant: " + ", ".join(f"{k:.3g}" for k in kinds))


@pytest.mark.parametrize("D", EMBED_PACKED_D)
def test_embed_packed_rows_and_ar_n_extra(dev, D):
    """embed_packed_kernel in both layouts against the rows of rowprep mode 0 at P = 0 (bit-equal to the reference, so to each other);
    sfmi_ar_n_extra_i32 on the same rows equals rowprep's extra_out; Lz = 0."""
    L = _L()
    lib = L.lib()
    B, V, Lmax = 37, 97, 12
    seq, ln, Lc = R.build_token_rows(f"embp/{D}", B, V, Lmax)
    tb = R.tables(f"embp/{D}", V, D, Lmax)
    end0 = V - 1
    want = np.stack([R.embed_rows_ref(tb, seq, int(Lc[b]), end0, b, int(ln[b]) - 1)[0] for b in range(B)])
    wex = np.array([R.embed_rows_ref(tb, seq, int(Lc[b]), end0, b, int(ln[b]) - 1)[1] for b in range(B)])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tbd, dseq, dlen, dLc = [d(t) for t in tb], d(seq), d(ln), d(Lc)
    Bp = 48
    bpk, brm = Band(dev, n=Bp * D), Band(dev, n=B * D)
    L.check(lib.sfmi_gpt_embed_packed_f32(*[L.ptr(t) for t in tbd], L.ptr(dseq), L.ptr(dlen), L.ptr(dLc), bpk.ptr(), B, D, Lmax, end0,
                                          L.stream_ptr()), "embed_packed")
    L.check(lib.sfmi_gpt_embed_rows_f32(*[L.ptr(t) for t in tbd], L.ptr(dseq), L.ptr(dlen), L.ptr(dLc), brm.ptr(), B, D, Lmax, end0,
                                        L.stream_ptr()), "embed_rows")
    torch.cuda.synchronize()
    pk = R.unpack(torch.from_numpy(bpk.np()), Bp, D).numpy()
    assert _same_bits(pk[:B], want) and _same_bits(brm.np((B, D)), want)
    assert _is_sent(pk[B:]).all(), "rows beyond B written"
    res, _, ex, _, _ = _embed_launch(dev, tb, seq, ln, Lc, D, Lmax, end0, B, 0, None, None, True, None, B, xn=False)
    assert _same_bits(res, want) and np.array_equal(ex, wex)
    # the dense form of the rule: every token of every row (conditions of one length per launch), then conditions alone (Lz = 0)
    for lc in sorted(set(Lc.tolist())):
        rows = np.nonzero(Lc == lc)[0]
        Lz = int((ln[rows] - lc).max())
        cpos = np.ascontiguousarray(seq[rows, :lc, 0])
        zpos = np.full((len(rows), max(Lz, 1)), end0, np.int32)
        for i, b in enumerate(rows):
            zpos[i, :ln[b] - lc] = seq[b, lc:ln[b], 0]
        for lz in sorted({Lz, 0}):
            bex = Band(dev, n=len(rows) * (lc + lz), dtype=torch.int32)
            dc, dz = d(cpos), (d(zpos[:, :lz]) if lz else None)
            L.check(lib.sfmi_ar_n_extra_i32(L.ptr(dc), L.ptr(dz), bex.ptr(), len(rows), lc, lz, end0, L.stream_ptr()), "ar_n_extra")
            torch.cuda.synchronize()
            got = bex.np((len(rows), lc + lz))
            wantx = np.concatenate([cpos, np.stack([R.ar_n_extra(cpos[i], zpos[i, :lz], end0) for i in range(len(rows))])], 1)
            assert np.array_equal(got, wantx), (lc, lz)
            for i, b in enumerate(rows):                 # the decode row of rowprep / embed_packed is one of these entries
                if ln[b] - 1 < lc + lz:
                    assert got[i, ln[b] - 1] == wex[b]


# ---------------------------------------------------------------------------------------------------- compaction, set_len
@pytest.mark.parametrize("D", COMPACT_D)
def test_compact_rows(dev, D):
    """compact_rows_kernel: the slot map is exact, padding slots are -1, live slots hold their stage rows in bits, ended slots are
    zero, rows of the residual beyond Bpad and the bands are untouched."""
    L = _L()
    lib = L.lib()
    for B in COMPACT_B:
        Bpad = int(lib.sfmi_decode_gemm_padded_rows(B))
        assert Bpad >= B and Bpad % 16 == 0
        for pat in COMPACT_PATTERNS:
            alen = R.alen_pattern(pat, B, D)
            stage = np.random.RandomState(B).randn(B, D).astype(np.float32)
            balen = Band(dev, init=alen)
            bso, bro, bsl, bnl = (Band(dev, n=n, dtype=torch.int32) for n in (B, Bpad, Bpad, 1))
            bst, bres = Band(dev, init=stage), Band(dev, n=(Bpad + 16) * D)
            L.check(lib.sfmi_gpt_compact_rows_f32(balen.ptr(), bso.ptr(), bro.ptr(), bnl.ptr(), bsl.ptr(), bst.ptr(), bres.ptr(), B, Bpad, D,
                                                  L.stream_ptr()), "compact_rows")
            torch.cuda.synchronize()
            slot_of, row_of, slot_len, nlive = R.compact_ref(alen, Bpad)
            assert np.array_equal(bso.np(), slot_of) and np.array_equal(bro.np(), row_of), (B, pat)
            assert np.array_equal(bsl.np(), slot_len) and int(bnl.np()[0]) == nlive, (B, pat)
            assert np.array_equal(balen.np(), alen) and _same_bits(bst.np((B, D)), stage)
            res = R.unpack(torch.from_numpy(bres.np()), Bpad + 16, D).numpy()
            want = np.zeros((B, D), np.float32)
            live = alen >= 0
            want[slot_of[live]] = stage[live]
            assert _same_bits(res[:B], want), (B, pat)
            assert _is_sent(res[B:]).all(), (B, pat, "slots beyond B written")


def test_set_len(dev):
    L = _L()
    for B in SETLEN_B:
        for delta in SETLEN_DELTA:
            src = np.arange(B, dtype=np.int32) * 3 - 5
            bl, bs = Band(dev, n=B, dtype=torch.int32), Band(dev, init=src)
            L.check(L.lib().sfmi_set_len_i32(bl.ptr(), bs.ptr(), B, delta, L.stream_ptr()), "set_len")
            torch.cuda.synchronize()
            assert np.array_equal(bl.np(), src + delta) and np.array_equal(bs.np(), src)


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    """Every SFMI_EINVAL check of these launchers, by return value: each call below is refused before anything is launched (the
    launchers check first and launch last), and no refused value would be valid for the kernel."""
    L = _L()
    lib = L.lib()
    buf = torch.zeros(1 << 16, device=dev)
    ibuf = torch.zeros(1 << 12, dtype=torch.int32, device=dev)
    p, q = buf.data_ptr(), ibuf.data_ptr()
    st = L.stream_ptr()

    def sample(**kw):
        a = dict(part=p, seq=q, len=q, Lc=q, logp=None, hist=None, force=None, resid=None, E0=None, E1=None, Ex=None, pe=None, D=0, S=1, B=4,
                 V=64, ldv=64, Lmax=16, tup=0, end0=63, end1=63, k=10, tp=0.5, T=1.0, g0=0, inv=1, comp=0, ms=4, seed=1, sd=None, adv=1,
                 ro=0, rt=4, so=0)
        a.update(kw)
        return lib.sfmi_gpt_sample_f32(*a.values(), st)

    bad = [dict(part=None), dict(seq=None), dict(len=None), dict(Lc=None), dict(V=4353, ldv=4353), dict(T=0.0), dict(T=-1.0), dict(rt=3),
           dict(ro=1), dict(so=-1), dict(V=0), dict(V=-1), dict(ldv=63), dict(S=0), dict(B=0), dict(B=-2), dict(tup=2), dict(tup=-1),
           dict(Lmax=0), dict(ro=-1, rt=4), dict(logp=p, ms=0), dict(hist=p, ms=0),
           dict(resid=p, D=64), dict(resid=p, E0=p, D=24), dict(resid=p, E0=p, D=0), dict(resid=p, E0=p, D=20),
           dict(resid=p, E0=p, D=64, tup=1), dict(resid=p, E0=p, E1=p, D=64, tup=1), dict(resid=p, E0=p, E1=p, Ex=p, D=64, tup=1)]
    for kw in bad:
        assert sample(**kw) == EINVAL, kw

    def rows(**kw):
        a = dict(part=p, seq=q, len=q, Lc=q, logp=None, resid=p, stage=p, E0=p, E1=p, Ex=p, pe=p, D=64, S=1, B=4, V=64, ldv=64, Lmax=16,
                 tup=0, end0=63, end1=63, k=10, tp=0.5, T=1.0, g0=0, comp=0, ms=4, seed=1, sd=None, adv=1, ro=0, rt=4, so=0, alen=q, slot=q)
        a.update(kw)
        return lib.sfmi_gpt_sample_rows_f32(*a.values(), st)

    for kw in [dict(slot=None), dict(alen=None), dict(resid=None), dict(stage=None), dict(D=24), dict(B=0), dict(V=0)]:
        assert rows(**kw) == EINVAL, kw

    def mask(**kw):
        a = dict(lg=p, seq=q, len=q, Lc=q, out=p, B=4, V=64, ldv=64, Lmax=16, tup=0, end0=63, end1=63, inv=1, comp=0)
        a.update(kw)
        return lib.sfmi_gpt_mask_logits_f32(*a.values(), st)

    for kw in [dict(lg=None), dict(seq=None), dict(len=None), dict(Lc=None), dict(out=None), dict(B=0), dict(V=0), dict(V=4353, ldv=4353),
               dict(ldv=63), dict(tup=2), dict(tup=-1)]:
        assert mask(**kw) == EINVAL, kw

    def embed(**kw):
        a = dict(E0=p, E1=p, Ex=p, pe=p, cpe=p, seq=q, len=q, Lc=q, nval=None, extra=None, eo=None, ro=p, xn=None, g=None, b=None, B=2, P=0,
                 D=64, Lmax=8, end0=9, rowoff=None, Mp=0)
        a.update(kw)
        return lib.sfmi_gpt_embed_f32(*a.values(), st)

    for kw in [dict(E0=None), dict(E1=None), dict(Ex=None), dict(pe=None), dict(cpe=None), dict(seq=None), dict(len=None), dict(Lc=None),
               dict(D=6), dict(D=4100), dict(rowoff=q, P=0, Mp=2), dict(rowoff=q, P=2, Mp=0)]:
        assert embed(**kw) == EINVAL, kw

    def rowprep(**kw):
        a = dict(ri=p, part=None, bias=None, Eadd=None, seq=None, len=None, Lc=None, nval=None, ro=p, xn=None, g=None, b=None, S=1, M=2, P=0,
                 D=64, Lmax=8, rowoff=None, B=2)
        a.update(kw)
        return lib.sfmi_gpt_rowprep_f32(*a.values(), st)

    for kw in [dict(ri=None), dict(D=6), dict(D=4100), dict(Eadd=p), dict(Eadd=p, seq=q), dict(Eadd=p, len=q), dict(rowoff=q, B=0)]:
        assert rowprep(**kw) == EINVAL, kw

    def embp(fn, **kw):
        a = dict(E0=p, E1=p, Ex=p, pe=p, cpe=p, seq=q, len=q, Lc=q, out=p, B=2, D=64, Lmax=8, end0=9)
        a.update(kw)
        return fn(*a.values(), st)

    for fn in (lib.sfmi_gpt_embed_packed_f32, lib.sfmi_gpt_embed_rows_f32):
        for kw in [dict(E0=None), dict(E1=None), dict(Ex=None), dict(pe=None), dict(cpe=None), dict(seq=None), dict(len=None), dict(Lc=None),
                   dict(out=None), dict(D=24)]:
            assert embp(fn, **kw) == EINVAL, kw

    def compact(**kw):
        a = dict(alen=q, so=q, ro=q, nl=q, sl=q, stage=p, resid=p, B=4, Bpad=16, D=64)
        a.update(kw)
        return lib.sfmi_gpt_compact_rows_f32(*a.values(), st)

    for kw in [dict(alen=None), dict(so=None), dict(ro=None), dict(nl=None), dict(sl=None), dict(stage=None), dict(resid=None), dict(B=0),
               dict(B=257, Bpad=272), dict(Bpad=3), dict(B=1, Bpad=258), dict(D=24)]:
        assert compact(**kw) == EINVAL, kw

    assert lib.sfmi_set_len_i32(None, q, 4, 0, st) == EINVAL and lib.sfmi_set_len_i32(q, None, 4, 0, st) == EINVAL
    for a in [(None, q, q, 2, 2, 1, 9), (q, q, None, 2, 2, 1, 9), (q, q, q, 0, 2, 1, 9), (q, q, q, 2, 0, 1, 9), (q, q, q, 2, 2, -1, 9),
              (q, None, q, 2, 2, 1, 9)]:
        assert lib.sfmi_ar_n_extra_i32(*a, st) == EINVAL, a
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and int(ibuf.abs().sum()) == 0
