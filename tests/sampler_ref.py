"""References of the decode step's sampler, embedding and row kernels of csrc/gpt.hip (sample_kernel, rowprep_kernel, embed_packed_kernel,
compact_rows_kernel, set_len_kernel) and of ar_n_extra_kernel (csrc/tokens.hip), the bounds their tests assert, and the builders of the
test inputs.  The case tables themselves are plain data at the top of tests/test_sampler_kernels_gpu.py.

What is exact (compared in bits)
  Masking (representers.py:120-155) is a function of integers and copies: mask_ref, one restatement with the kernel's per-row len / Lc and
  step_offset (tests/test_sampler_ref_cpu.py holds it against oracle.tokens_oracle.sampling_masker).  The slab sum is ((p0 + p1) + p2) in
  f32.  The keys are fl(lg * fl(1 / T)): one multiply, nothing to contract with.  The candidate set is {x > -inf and key(x) >= the k-th
  largest key}, the order value descending then index ascending; with 0 < top_k <= 512 and more than 512 candidates (ties at the k-th
  key) the kernel keeps the first 512 of that order (sampler section) and so does `candidates`.  Embeddings are three f32 adds
  in a fixed order, ((E0[pos] + E1[val]) + Ex[ext]) + pe[t]; the AR_N extra index (representers.py:188-196, 432-442) is `ar_n_extra`, one
  rule for its four device copies.  The compaction is a stable partition of alen >= 0.

The draw: a set, not a tolerance                                                                                                   [DRAW]
  The running sums are sequential f32 adds (mirrored exactly), __expf is not correctly rounded.  f32 rounding is monotone, so a
  sequential f32 sum is monotone in every addend.  With d_i = fl(x_i - x_0) of the sorted candidates and e_i = exp(d_i) in float64,
      e_lo_i = rounddown_f32(e_i (1 - r_i)),  e_hi_i = roundup_f32(e_i (1 + r_i)),  r_i = E_EXP (1 + |d_i|) U       (train_ref.py: E_EXP)
  bracket the kernel's exps (d_i = 0: __expf(0) = exp2(0) = 1 exactly, the bracket is [1, 1]), the f32 cumsums of e_lo and e_hi bracket
  its running sums, fl(e_lo / tot_hi) and fl(e_hi / tot_lo) bracket the top-p quotients - the f32 division is correctly rounded, hence
  monotone: the library is built without -ffast-math and without -fno-hip-fp32-correctly-rounded-divide-sqrt (build.py FLAGS, asserted by
  tests/test_sampler_ref_cpu.py; train_ref.py measured 1.0000 U), draw_set(widen_div=True) widens them by one ulp each way for a build
  that is not - and their sequential cumsums give a range [keep_lo, keep_hi] of kept prefixes.  For
  every keep of that range the threshold fl(u cs[keep-1]) lies in [fl(u cs_lo[keep-1]), fl(u cs_hi[keep-1])], and the first index whose
  running sum exceeds it in [first i: cs_hi_i > thr_lo, first i: cs_lo_i > thr_hi] (the last kept index where there is none).  The
  accepted set is the union of those rank intervals; the kernel's token must be a member.  Conditions on the inputs, asserted for the
  reference alone by tests/test_sampler_ref_cpu.py: per (top_k, top_p, T) family at most 4 % of the draws have more than one accepted
  token, no set has more than 8, and the f32 oracle's draw (TO.sample_filtered on TO.filter_sampling_logits) is a member.

Log-probability                                                                                                                     [LOGP]
  logp = lg[c] - (gmax + __logf(sum_v __expf(lg_v - gmax))) against the float64 log-softmax of the masked logits.  x_v = lg_v - gmax
  rounds once, p_v = __expf(x_v):  r_v = U |x_v| + E_EXP (1 + |x_v|) U.  A thread adds ceil(V / 256) terms, the wave butterfly 6 levels,
  the four waves (a + b) + (c + d) two more:  e_t = sum_v p_v r_v / tot + gamma(ceil(V / 256) + 8) + V TINY, relative to tot in [1, V].
      |d logp| <= e_t + E_LOG U log tot + U |gmax + log tot| + U |logp|
  A row whose only finite logit is the chosen one: exp(0) = 1, sum = 1, log 1 = 0, x - x = +0.0f exactly.  A masked forced token: -inf.

LayerNorm of rowprep_kernel (two-pass, biased variance, eps 1e-5f)                                                                   [RLN]
  A thread owns nq = ceil(D / 1024) float4s: (x0 + x1) + (x2 + x3) is two levels, the thread's running sum nq more, the wave butterfly 6,
  red[0] + red[1] + red[2] + red[3] three:  ns = nq + 11, the division by D one more.  With E|.| the row mean of absolute values:
      |d mean| = dm <= gamma(ns + 1) E|x|
      var_f = mean (x - mean_f)^2 = var + (mean_f - mean)^2 exactly; difference, square, sum, division, + eps:
      |d var| <= dm^2 + gamma(ns + 4) (var + dm^2);   e = |d var| / (var + eps);   e_r = e / (2 (1 - e)^1.5) + (1 + E_RSQRT) U
      |d xhat| = dxh <= rstd (1 + e_r) (dm + U |x - mean|) + |xhat| (e_r + U)
      out = xhat g + b:  |d out| <= |g| dxh + U |xhat g| + U |out|
  The input x of mode 1 is itself an f32 sum in a fixed order, x = (resid + (((p0 + p1) + p2) + bias)) + Eadd[row]: mirrored in f32 and
  compared in bits (resid_out); the float64 LayerNorm starts from that f32 x.  Unbiased variance moves rstd by 1 / (2 D) relative: 1.2e-4
  at D = 4096 against a bound of ~1e-6."""
from __future__ import annotations

import zlib

import numpy as np

from decode_ref import pack, unpack, pk_off        # noqa: F401  (re-exported for the tests)
from train_ref import U, E_EXP, E_LOG, E_RSQRT, TINY, gamma, hash_unit_idx

F32 = np.float32
NEG = F32(-np.inf)
SMP_MAXC, SMP_NPOS, VMAX = 512, 1040, 4352         # csrc/gpt.hip
LN_EPS32 = float(np.float32(1e-5))


# ---------------------------------------------------------------------------------------------------- masking, keys, candidates
def slab_sum(part):
    """(S, B, ld) -> (B, ld): ((p0 + p1) + p2) in f32."""
    part = np.asarray(part, F32)
    x = part[0].copy()
    for s in range(1, part.shape[0]):
        x = (x + part[s]).astype(F32)
    return x


def mask_ref(x, pos, L, lc, tup, end0, end1, inv=1, comp=0, so=0, mut=None):
    """sampling_masker for one row: x (V,) f32 logits, pos = seq[b, :, 0], L = len[b] complete tokens (tuple 1: pos[L] just drawn).
    mut: 'inv_at_j0' / 'lt_last' (mutants)."""
    x = np.array(x, F32, copy=True)
    v = np.arange(x.size)
    if tup == 1:
        if int(pos[L]) == end0:
            x[:] = NEG
            x[end1] = F32(1.0)
        return x
    j, last = L - lc - so, int(pos[L - 1])
    if inv and (j > 0 or mut == "inv_at_j0"):
        m = (v < last) if mut == "lt_last" else (v <= last)
        x[m & (v != end0)] = NEG
    if comp:
        cond = np.asarray(pos[:lc])
        i = int(np.searchsorted(cond, last, side="right"))
        nxt = int(cond[i]) if i < lc else end0 + 1
        x[v > nxt] = NEG
    return x


def fkey(x):
    """fkey_u: order-preserving u32 key of an f32; -0.0 takes the key of +0.0, so the keys order exactly as the floats compare."""
    u = np.ascontiguousarray(np.asarray(x, F32) + F32(0.0), F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def scaled(lg, T):
    return (np.asarray(lg, F32) * (F32(1.0) / F32(T))).astype(F32)


def eff_k(top_k, V):
    """the case tables write V + n as -n"""
    return V - top_k if top_k < 0 else top_k


def candidates(x, top_k, mut=None):
    """x (V,) scaled masked logits -> (indices in rank order, overflow).  mut: 'tie_desc', 'strict_kth'."""
    V = x.size
    big = top_k <= 0 or top_k > SMP_MAXC
    k = min(top_k, V) if top_k > 0 else V
    key = fkey(x)
    kth = np.sort(key)[::-1][k - 1]
    sel = np.nonzero((x > NEG) & (key >= kth))[0]
    order = np.lexsort((-sel if mut == "tie_desc" else sel, -x[sel]))
    idx = sel[order]
    if mut == "strict_kth":
        idx = idx[:k]
    over = (not big) and idx.size > SMP_MAXC
    return (idx[:SMP_MAXC] if over else idx), bool(over)


# ---------------------------------------------------------------------------------------------------- the draw
def _down(a):
    y = np.asarray(a, np.float64).astype(F32)
    return np.where(y.astype(np.float64) > a, np.nextafter(y, NEG), y).astype(F32)


def _up(a):
    y = np.asarray(a, np.float64).astype(F32)
    return np.where(y.astype(np.float64) < a, np.nextafter(y, F32(np.inf)), y).astype(F32)


def exp_bracket(xs):
    """sorted candidate values -> (e_lo, e_hi) f32 of [DRAW]."""
    d = (xs - xs[0]).astype(F32).astype(np.float64)
    e = np.exp(d)
    r = E_EXP * (1.0 + np.abs(d)) * U
    lo, hi = _down(e * (1.0 - r)), _up(e * (1.0 + r) + TINY)
    lo = np.where(lo < F32(2.0 ** -125), F32(0), lo)            # results below the normal range may be flushed
    one = d == 0.0
    lo[one], hi[one] = F32(1), F32(1)
    return lo.astype(F32), hi.astype(F32)


def _first_above(cs, thr, keep):
    return min(int(np.searchsorted(cs[:keep], thr, side="right")), keep - 1)


def draw_set(xs, top_p, u, widen_div=False):
    """(sorted ranks the kernel may draw, (keep_lo, keep_hi)) of [DRAW]."""
    C = xs.size
    e_lo, e_hi = exp_bracket(xs)
    cs_lo, cs_hi = np.cumsum(e_lo, dtype=F32), np.cumsum(e_hi, dtype=F32)
    p, u = F32(top_p), F32(u)
    keep_lo = keep_hi = C
    if p > 0:
        q_hi, q_lo = (e_hi / cs_lo[-1]).astype(F32), (e_lo / cs_hi[-1]).astype(F32)
        if widen_div:
            q_hi, q_lo = np.nextafter(q_hi, F32(np.inf)), np.maximum(np.nextafter(q_lo, NEG), F32(0))
        keep_lo = int(np.searchsorted(np.cumsum(q_hi, dtype=F32)[:C - 1], p, side="right")) + 1
        keep_hi = int(np.searchsorted(np.cumsum(q_lo, dtype=F32)[:C - 1], p, side="right")) + 1
    ranks = set()
    for keep in range(keep_lo, keep_hi + 1):
        i0 = _first_above(cs_hi, F32(u * cs_lo[keep - 1]), keep)
        i1 = _first_above(cs_lo, F32(u * cs_hi[keep - 1]), keep)
        ranks.update(range(i0, i1 + 1))
    return sorted(ranks), (keep_lo, keep_hi)


def mirror_draw(xs, top_p, u, mut=None):
    """The kernel's serial tail in f32 with numpy's f32 exp in place of __expf -> rank.  mut: 'p_ge', 'keep_plus', 'keep_minus',
    'thr_total' (mutants)."""
    C = xs.size
    e = np.exp((xs - xs[0]).astype(F32)).astype(F32)
    cs = np.cumsum(e, dtype=F32)
    keep = C
    if F32(top_p) > 0:
        cum = np.cumsum((e / cs[-1]).astype(F32), dtype=F32)[:C - 1]
        keep = int(np.searchsorted(cum, F32(top_p), side="left" if mut == "p_ge" else "right")) + 1
    if mut == "keep_plus":
        keep = min(keep + 1, C)
    if mut == "keep_minus":
        keep = max(keep - 1, 1)
    thr = F32(F32(u) * (cs[-1] if mut == "thr_total" else cs[keep - 1]))
    return _first_above(cs, thr, keep)


def uniform(seed, j, tup, rows_total, grow):
    return F32(hash_unit_idx(seed, np.array([(j * 2 + tup) * rows_total + grow]))[0])


def logp_ref(ml, choice):
    """masked logits (V,) f32, the written token -> (float64 log-softmax at the token, [LOGP] bound); (-inf, 0) for a masked token."""
    z = np.asarray(ml, np.float64)
    if not np.isfinite(z[choice]):
        return -np.inf, 0.0
    gmax = z.max()
    x = z[np.isfinite(z)] - gmax
    p = np.exp(x)
    tot = p.sum()
    r = U * np.abs(x) + E_EXP * (1.0 + np.abs(x)) * U
    V = z.size
    e_t = float((p * r).sum() / tot + gamma(-(-V // 256) + 8) + V * TINY)
    lt = np.log(tot)
    ref = z[choice] - (gmax + lt)
    return float(ref), float(e_t + E_LOG * U * lt + U * abs(gmax + lt) + U * abs(ref))


# ---------------------------------------------------------------------------------------------------- sampler inputs and expectation
KINDS0 = ("j0", "mid", "end", "few", "late", "mid", "nocond", "mid")      # tuple 0 row states, rotating over the rows
KINDS1 = ("cur", "curend", "cur", "late")                                 # tuple 1


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def case_defaults(c):
    d = dict(S=1, tup=0, B=64, logits="n3", so=0, inv=1, comp=1, Lmax=64, max_steps=4, greedy0=0, row_offset=0, seed=0x1234ABCD)
    d.update(c)
    d.setdefault("ldv", d["V"])
    d.setdefault("rows_total", d["B"] + d["row_offset"])
    d.setdefault("kinds", KINDS1 if d["tup"] else KINDS0)
    d["end0"] = d["end1"] = d["V"] - 1
    return d


def _logits(rng, kind, B, V):
    if kind in ("n3", "n1", "n001"):
        return (rng.randn(B, V) * {"n3": 3.0, "n1": 1.0, "n001": 0.01}[kind]).astype(F32)
    sc = {"tie3": 3.0, "tieflat": 0.6, "tieeq": 0.0}[kind]      # multiples of 0.5; every 8th row (from row 5) all equal; tieeq: every row
    x = (np.round(rng.randn(B, V) * sc * 2.0) / 2.0).astype(F32)
    x[5::8] = F32(1.5)
    if kind == "tieeq":
        x[:] = F32(-2.5)
    return x


def build_sampler_inputs(c):
    """c: a case dict (case_defaults applied) -> part (S, B, ldv) with NaN in the columns V .. ldv-1, seq (B, Lmax, 2) with 0x5A5A5A5A
    wherever the row holds no token, len, Lc."""
    rng = _rng(c["name"])
    V, ldv, S, B, Lmax, so, tup, end0 = c["V"], c["ldv"], c["S"], c["B"], c["Lmax"], c["so"], c["tup"], c["end0"]
    x = _logits(rng, c["logits"], B, V)
    part = np.full((S, B, ldv), np.nan, F32)
    rest = x.copy()
    for s in range(1, S):
        if c["logits"].startswith("tie"):
            p = (np.round(rng.randn(B, V) * 2.0) / 2.0).astype(F32)
            rest = (rest - p).astype(F32)                       # exact: multiples of 0.5 of small magnitude
        else:
            p = (rng.randn(B, V) * 0.5).astype(F32)
        part[s, :, :V] = p
    part[0, :, :V] = rest
    seq = np.full((B, Lmax, 2), 0x5A5A5A5A, np.int32)
    ln, Lc, kinds = np.zeros(B, np.int32), np.zeros(B, np.int32), []
    for b in range(B):
        kind = c["kinds"][b % len(c["kinds"])]
        kinds.append(kind)
        ncond = min(int(rng.randint(0, 4)), V - 1)
        cond = sorted(rng.choice(V - 1, ncond, replace=False).tolist()) if ncond else []
        if not (kind == "nocond" and cond):
            cond = cond + [end0]
        lc = len(cond)
        g = {"j0": so, "mid": so + 1 + int(rng.randint(0, 2)), "end": so + 1, "few": so + 1, "nocond": so + 1,
             "late": so + c["max_steps"] + int(rng.randint(0, 2)), "cur": so + int(rng.randint(0, 3)), "curend": so + 1}[kind]
        last = {"end": end0, "few": max(0, V - 2 - int(rng.randint(0, 10))), "nocond": min(max(cond) + 1 + int(rng.randint(0, 5)), V - 1)
                }.get(kind, int(rng.randint(0, max(1, V // 2))))
        gen = sorted(int(rng.randint(0, last + 1)) for _ in range(max(g - 1, 0))) + ([last] if g else [])
        L = lc + g
        assert L + 1 < Lmax
        seq[b, :lc, 0], seq[b, lc:L, 0] = cond, gen
        seq[b, :L, 1] = rng.randint(0, V, L)
        if tup == 1:
            seq[b, L, 0] = end0 if kind == "curend" else int(rng.randint(0, max(1, V - 1)))
        ln[b], Lc[b] = L, lc
    return dict(part=part, seq=seq, len=ln, Lc=Lc, kinds=kinds)


def sampler_expect(c, inp, mut=None, oracle=False):
    """Per row: dict(j, ml (masked logits), C, over, greedy, accept (token ids), mirror (the f32 mirror's token), keeps, oracle)."""
    V, B, tup, so = c["V"], c["B"], c["tup"], c["so"]
    k, p, T = c["kpt"]
    k = eff_k(k, V)
    x_all = slab_sum(inp["part"])[:, :V]
    rows = []
    for b in range(B):
        L, lc = int(inp["len"][b]), int(inp["Lc"][b])
        j, grow = L - lc - so, c["row_offset"] + b
        mmut = mut if mut in ("inv_at_j0", "lt_last") else None
        ml = mask_ref(x_all[b], inp["seq"][b, :, 0], L, lc, tup, c["end0"], c["end1"], c["inv"], c["comp"], so, mmut)
        greedy = bool((c["greedy0"] and grow == 0) or k == 1)
        row = dict(j=j, ml=ml, greedy=greedy, over=False, C=1, keeps=(1, 1), oracle=None)
        if greedy:
            row["accept"] = np.array([int(np.argmax(ml))])
            row["mirror"] = int(np.argmax(ml))
        else:
            xs_all = scaled(ml, T)
            idx, over = candidates(xs_all, k, mut)
            xs = xs_all[idx]
            u = uniform(c["seed"], j, tup, c["rows_total"], b if mut == "u_local" else grow)
            ranks, keeps = draw_set(xs, p, u)
            row.update(accept=idx[ranks], mirror=int(idx[mirror_draw(xs, p, u, mut)]), C=int(idx.size), over=over, keeps=keeps, u=u)
            if oracle:
                from oracle import tokens_oracle as TO
                row["oracle"] = TO.sample_filtered(TO.filter_sampling_logits(ml, k, float(p), float(T)), u)
        rows.append(row)
    return rows


# ---------------------------------------------------------------------------------------------------- embeddings
def ar_n_extra(cond_pos, pos, end0, mut=None):
    """get_next_cond (representers.py:432-442) for one row: the first condition position > pos (the last one where there is none);
    an end token keeps end0.  cond_pos ascending.  mut: 'ge' (mutant)."""
    cond, pos = np.asarray(cond_pos), np.asarray(pos)
    i = np.minimum(np.searchsorted(cond, pos, side="left" if mut == "ge" else "right"), cond.size - 1)
    out = cond[i].copy()
    out[pos == end0] = end0
    return out


def token_extra(pos_row, t, lc, end0, mut=None):
    """the extra index of the token at t of a row (representers.py:188-196): a condition token's own position, else ar_n_extra."""
    if t < lc:
        return int(pos_row[t])
    return int(ar_n_extra(pos_row[:lc], np.array([pos_row[t]]), end0, mut)[0])


def emb_ref(E0, E1, Ex, pe, pos, val, ext, mut=None):
    """((E0[pos] + E1[val]) + Ex[ext]) + pe in f32 (mingpt.py:285).  mut: 'order' (mutant: E0 + (E1 + (Ex + pe)))."""
    a, b, c, d = (np.asarray(t, F32) for t in (E0[pos], E1[val], Ex[ext], pe))
    if mut == "order":
        return (a + (b + (c + d).astype(F32)).astype(F32)).astype(F32)
    return (((a + b).astype(F32) + c).astype(F32) + d).astype(F32)


def build_token_rows(name, B, V, Lmax, nmax=6):
    """Rows of tokens for the embedding kernels: conditions (ascending, ending with the end token) of 1 .. 4 tokens, 0 .. nmax generated
    tokens among them end tokens, positions beyond every condition position but the end token, and repeats of condition positions."""
    rng = _rng(name)
    end0 = V - 1
    seq = np.zeros((B, Lmax, 2), np.int32)
    ln, Lc = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        ncond = min(int(rng.randint(0, 4)), V - 1)
        cond = sorted(rng.choice(V - 1, ncond, replace=False).tolist()) + [end0]
        g = b % (nmax + 1)
        gen = []
        for i in range(g):
            r = (b + i) % 4
            gen.append(end0 if r == 0 else (cond[i % len(cond)] if r == 1 else (max(cond[:-1] + [0]) + 1 if r == 2 else int(rng.randint(0, V)))))
        gen = [min(x, end0) for x in gen]
        L = len(cond) + g
        assert L <= Lmax
        seq[b, :L, 0] = cond + gen
        seq[b, :L, 1] = rng.randint(0, V, L)
        ln[b], Lc[b] = L, len(cond)
    return seq, ln, Lc


def tables(name, V, D, Lmax):
    rng = _rng(name + "/tables")
    return tuple((rng.randn(n, D)).astype(F32) for n in (V, V, V, Lmax, Lmax))      # E0, E1, Ex, pos_emb, cond_pos_emb


def embed_rows_ref(tb, seq, lc, end0, b, t, extra=None, mut=None):
    """The embedding of token t of row b and its extra index."""
    E0, E1, Ex, pe, cpe = tb
    pos, val = int(seq[b, t, 0]), int(seq[b, t, 1])
    ext = int(extra[b, t]) if extra is not None else token_extra(seq[b, :, 0], t, lc, end0, "ge" if mut == "ge" else None)
    row = cpe[t] if t < lc else pe[t - lc]
    return emb_ref(E0, E1, Ex, row, pos, val, ext, mut if mut == "order" else None), ext


# ---------------------------------------------------------------------------------------------------- rowprep
def rowprep_rows(P, B, nval, Lc, rowoff=None, M=None):
    """(b, t) of every row m of a rowprep launch: decode form (P == 0: t is the caller's len - 1, returned as -1), the (B, P) rectangle,
    or packed ragged rows; t is clamped to max(nval - 1, 0) (nval NULL: Lc - 1)."""
    out = []
    if P and rowoff is not None:
        for m in range(M):
            b = int(np.searchsorted(rowoff, m, side="right")) - 1
            out.append((b, m - int(rowoff[b])))
    elif P:
        out = [(m // P, m % P) for m in range(B * P)]
    else:
        return [(b, -1) for b in range(B)]
    res = []
    for b, t in out:
        tmax = max((int(nval[b]) if nval is not None else int(Lc[b]) - 1) - 1, 0)
        res.append((b, min(t, tmax)))
    return res


def accum_ref(resid, part=None, bias=None, eadd=None):
    """mode 1's x in f32, in the kernel's order."""
    x = np.asarray(resid, F32)
    if part is not None:
        p = np.asarray(part[0], F32)
        for s in range(1, len(part)):
            p = (p + part[s]).astype(F32)
        if bias is not None:
            p = (p + np.asarray(bias, F32)).astype(F32)
        x = (x + p).astype(F32)
    if eadd is not None:
        x = (x + np.asarray(eadd, F32)).astype(F32)
    return x


def rowln_ref(x, g, be, mut=None):
    """x (M, D) f32 -> (float64 LayerNorm, [RLN] bound).  mut: 'unbiased' (mutant)."""
    x, g, be = (np.asarray(a, np.float64) for a in (x, g, be))
    D = x.shape[1]
    ns = -(-D // 1024) + 11
    mean = x.mean(1, keepdims=True)
    xc = x - mean
    var = (xc * xc).mean(1, keepdims=True)
    if mut == "unbiased":
        var = var * D / (D - 1)
    rstd = 1.0 / np.sqrt(var + LN_EPS32)
    xhat = xc * rstd
    out = xhat * g + be
    dm = gamma(ns + 1) * np.abs(x).mean(1, keepdims=True)
    dvar = dm * dm + gamma(ns + 4) * (var + dm * dm)
    e = dvar / (var + LN_EPS32)
    e_r = e / (2.0 * (1.0 - e) ** 1.5) + (1.0 + E_RSQRT) * U
    dxh = rstd * (1.0 + e_r) * (dm + U * np.abs(xc)) + np.abs(xhat) * (e_r + U)
    return out, np.abs(g) * dxh + U * np.abs(xhat * g) + U * np.abs(out) + TINY


def ln_rows(rng, M, D):
    """rows of |mean| / std 0, 3, 30 and a constant row, rotating."""
    x = rng.randn(M, D).astype(F32)
    x[1::4] += F32(3.0)
    x[2::4] += F32(30.0)
    x[3::4] = F32(0.3)
    return x


# ---------------------------------------------------------------------------------------------------- compaction
def compact_ref(alen, Bpad):
    """stable partition of alen >= 0 -> slot_of (B), row_of (Bpad), slot_len (Bpad), nlive."""
    alen = np.asarray(alen)
    B = alen.size
    live = alen >= 0
    nlive = int(live.sum())
    slot = np.where(live, np.cumsum(live) - 1, nlive + np.cumsum(~live) - 1)
    row_of, slot_len = np.full(Bpad, -1, np.int32), np.full(Bpad, -1, np.int32)
    row_of[slot] = np.arange(B)
    slot_len[slot[live]] = alen[live]
    return np.where(live, slot, -1).astype(np.int32), row_of, slot_len, nlive


def alen_pattern(kind, B, seed=0):
    a = np.arange(B, dtype=np.int32) + 3
    if kind == "none":
        a[:] = -1
    elif kind == "alt":
        a[1::2] = -1
    elif kind == "last":
        a[:-1] = -1
    elif kind == "random":
        a[np.random.RandomState(seed + B).rand(B) < 0.5] = -1
    return a
