"""CPU companion of tests/train_ref.py (no GPU): the mirrors of the launch rules against the source text of csrc/train.hip, the case
tables of tests/test_train_kernels_gpu.py against the mirrors (every form is reached), and the teeth of the bounds: for each operation an
fp32 numpy emulation in the kernel's summation arrangement stays inside the bound at every case of the GPU tables, and every listed mutant
of it lands outside a TENFOLD-wider bound (or fails the bit-exact gate where that is the check the mutant is meant for)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import train_ref as R                    # noqa: E402
import test_train_kernels_gpu as T       # noqa: E402  (plain data and CPU input builders; nothing there touches a GPU at import)

f32 = np.float32
_qk, _pv, _tq = R._qk, R._pv, R._tq
TEETH = 10.0


def _src():
    return open(os.path.join(ROOT, "shapeformer_amd", "csrc", "train.hip")).read()


def _body(src, head):
    """the brace-matched body of the function whose definition starts with `head`"""
    i = src.index(head)
    j = src.index("{", i)
    depth, k = 0, j
    while True:
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[j:k + 1]
        k += 1


# ---------------------------------------------------------------------------------------------------- mirrors against the source
def test_colsum_slices_mirror_is_the_source_rule():
    b = _body(_src(), "int sfmi_colsum_slices(int M, int N)")
    assert re.search(r"cb = \(N \+ 63\) / 64", b)
    assert int(re.search(r"rs = \((\d+) \+ cb - 1\) / cb", b).group(1)) == R.COLSUM_TARGET_BLOCKS
    assert int(re.search(r"if \(rs > (\d+)\) rs = (\d+)", b).group(1)) == R.COLSUM_MAX_SLICES == int(re.search(r"if \(rs > (\d+)\) rs = (\d+)", b).group(2))
    assert int(re.search(r"if \(rs > M / (\d+)\) rs = M / (\d+)", b).group(1)) == R.COLSUM_MIN_ROWS
    assert "return rs < 1 ? 1 : rs" in b
    assert R.colsum_slices(2050, 64) == 128 and R.colsum_slices(15, 64) == 1 and R.colsum_slices(3000, 4096) == 32 and R.colsum_slices(33, 64) == 2


def test_col_reduce_slices_mirror_is_the_source_rule():
    b = _body(_src(), "int sfmi_col_reduce_slices(int M)")
    m = re.search(r"return M <= (\d+) \? 1 : \(M \+ (\d+)\) / (\d+) > (\d+) \? (\d+) : \(M \+ (\d+)\) / (\d+);", b)
    a = [int(v) for v in m.groups()]
    assert a == [R.CR_DIRECT_ROWS, R.CR_ROWS_PER_SLICE - 1, R.CR_ROWS_PER_SLICE, R.CR_MAX_SLICES, R.CR_MAX_SLICES, R.CR_ROWS_PER_SLICE - 1, R.CR_ROWS_PER_SLICE]
    assert [R.col_reduce_slices(M) for M in T.CR_M] == [1, 1, 1, 1, 1, 3, 4, 16]


def test_layernorm_rows_dispatch_mirror_is_the_source_rule():
    b = _body(_src(), "int sfmi_layernorm_bwd_rows_drop_sd_f32(")
    inst = sorted((int(d), int(ne)) for d, ne in re.findall(r"if \(D == (\d+)\) hipLaunchKernelGGL\(ln_bwd_rows_wave_kernel<(\d+)>", b))
    assert [d for d, _ in inst] == sorted(R.LN_WAVE_WIDTHS) and all(d == 64 * ne for d, ne in inst)
    assert len(re.findall(r"ln_bwd_rows_kernel,", b)) == 1 and b.index("ln_bwd_rows_kernel,") > b.index("ln_bwd_rows_wave_kernel<2>")
    # the argument check of the fallback path stands before the first launch
    assert b.index("% 4) return SFMI_EINVAL") < b.index("hipLaunchKernelGGL")
    assert [R.ln_rows_form(D) for D in T.LN_D_WAVE] == ["wave"] * 4 and [R.ln_rows_form(D) for D in T.LN_D_BLOCK] == ["block"] * 4


def test_attention_launch_mirrors_are_the_source_rules():
    src = _src()
    b = _body(src, "static void attn_bwd_fused_launch(")
    m = re.search(r"if \(\(long long\)B \* H \* 2 \* nqb <= (\d+) && nqb > 1\)", b)
    assert int(m.group(1)) == R.ATTN_BWD_SMALL_WG and "nqb = (L + 63) / 64" in b
    assert re.findall(r"attn_bwd_fused_kernel<(\d), (\d)>", b) == [("2", "2"), ("4", "1")]
    b = _body(src, "int sfmi_attn_train_fwd_small_sd_f32(")
    assert int(re.search(r"if \(\(long long\)B \* H \* \(\(L \+ 63\) / 64\) > (\d+)\) return SFMI_EINVAL", b).group(1)) == R.ATTN_FWD_SMALL_WG


def test_argument_checks_stand_in_the_source_before_the_launch():
    src = _src()
    for head, conds in (("int sfmi_transpose_f32(", ["ldin < C"]), ("int sfmi_colsum_f32(", ["ld < N"]), ("int sfmi_colsum_ws_f32(", ["ld < N"]),
                        ("int sfmi_col_reduce_f32(", ["ld[i] < N[i]"]), ("int sfmi_ce_fwd_bwd_f32(", ["V <= 0", "ld < V", "L <= 0", "t0 < 0"]),
                        ("int sfmi_attn_bwd_f32(", ["B <= 0", "L <= 0", "H <= 0"])):
        b = _body(src, head)
        for c in conds:
            assert c in b and b.index(c) < b.index("hipLaunchKernelGGL"), (head, c)


def test_the_gpu_tables_reach_every_form():
    assert {R.colsum_slices(M, N) for M, N in T.COLSUM_WS_CASES} >= {1, 2, 6, 32, 128}
    M, N = 2050, 64                                            # the last slices own no rows
    RS = R.colsum_slices(M, N)
    assert RS == 128 and -(-M // RS) == 17 and 17 * (RS - 1) > M
    assert {R.col_reduce_slices(M) for M in T.CR_M} == {1, 3, 4, 16} and set(k for _, _, k in T.CR_JOBS) == {0, 1}
    assert any(ld > N for N, ld, _ in T.CR_JOBS[:3]) and {N for N, _, _ in T.CR_JOBS} == {4, 60, 64, 68, 1024, 3072}
    assert {R.ln_rows_form(D) for D in T.LN_D_WAVE + T.LN_D_BLOCK} == {"wave", "block"} and set(T.LN_D_WAVE) == set(R.LN_WAVE_WIDTHS)
    assert {R.attn_bwd_form(*c) for c in T.ATTN_CASES} == {(2, 2), (4, 1)}
    assert {R.attn_fwd_small(*c) for c in T.ATTN_CASES} == {True, False}
    assert {(L + 63) // 64 for _, L, _ in T.ATTN_CASES} == {1, 2, 3}
    # AdamW: both paths of adamw_multi_kernel, by its alignment rule
    vec = [T.adam_chunk_is_vector("aligned", t, o, n) for t, o, n in zip(*T.adam_chunks("vector"))]
    assert any(vec) and not all(vec)
    assert not any(T.adam_chunk_is_vector("aligned", t, o, n) for t, o, n in zip(*T.adam_chunks("scalar")) if n % 4)
    off = {t: T.adam_chunk_is_vector("offset", t, o, n) for t, o, n in zip(*T.adam_chunks("vector"))}
    assert not off[1] and not off[3] and off[2] and off[4]
    assert any(f % 4 for f in T.ADAM_FOFF["offset"])
    for kind in ("vector", "scalar"):                          # a partition of every tensor
        cov = [np.zeros(n, int) for n in T.ADAM_LENS]
        for t, o, n in zip(*T.adam_chunks(kind)):
            cov[t][o:o + n] += 1
        assert all((c == 1).all() for c in cov)
    assert set(T.adam_chunks("scalar")[2]) >= {1, 3, 255, 1025}


# ---------------------------------------------------------------------------------------------------- fp32 emulations
def _serial(rows):
    """f32 sum of the rows of a (R, N) array one after the other, from 0"""
    s = np.zeros(rows.shape[1:], f32)
    for r in rows:
        s = s + r
    return s


def _tree4(p):
    return (p[0] + p[1]) + (p[2] + p[3])


def emu_colsum(kind, a, prev=None, g=None, mutant=None):
    """colsum_kernel / colsum_part + finish / col_reduce_kernel in f32.  a (M, N) f32 terms; g: the kind-1 dgamma terms (then returns
    (out, out2) = (dgamma, dbeta)); prev (or (prev, prev2)): what accumulate adds to."""
    M, N = a.shape
    lanes = 4 if kind in ("plain", "ws") else 16
    RS = 1 if kind == "plain" else R.colsum_slices(M, N) if kind == "ws" else R.col_reduce_slices(M)
    rows_per = -(-M // RS)

    def reduce(t):
        parts = []
        for s in range(RS):
            m0, m1 = s * rows_per, min(M, (s + 1) * rows_per)
            lane = [_serial(t[m0 + l:m1:lanes]) if m0 + l < m1 else np.zeros(N, f32) for l in range(lanes)]
            if mutant == "lane":
                lane[1] = np.zeros(N, f32)
            parts.append(_tree4(lane) if lanes == 4 else _serial(np.stack(lane)))
        if mutant == "slice":
            parts = parts[:-1] if RS > 1 else parts
            k = max(i for i in range(RS) if i * rows_per < M)                 # the last slice that owns rows
            parts = [p for i, p in enumerate(parts) if i != k] if RS > 1 else parts
        return _serial(np.stack(parts)) if kind != "plain" else parts[0]
    out = reduce(a)
    if g is None:
        return out if prev is None or mutant == "accumulate" else (prev + out).astype(f32)
    o1, o2 = reduce(g), out
    if mutant == "swap":
        o1, o2 = o2, o1
    if prev is not None and mutant != "accumulate":
        o1, o2 = (prev[0] + o1).astype(f32), (prev[1] + o2).astype(f32)
    return o1, o2


def _butterfly(v):
    """wave_sum over the last axis (64 lanes): the xor-32 .. xor-1 butterfly in f32; every lane ends with the sum"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _row_sum(t, form):
    """a row sum of t (M, D) f32 as ln_bwd_rows_wave_kernel / ln_bwd_rows_kernel forms it"""
    M, D = t.shape
    if form == "wave":
        lane = _serial(np.moveaxis(t.reshape(M, D // 64, 64), 1, 0))
        return _butterfly(lane)
    pad = -(-D // 256) * 256
    tp = np.zeros((M, pad), f32)
    tp[:, :D] = t
    thr = _serial(np.moveaxis(tp.reshape(M, pad // 256, 256), 1, 0))           # (M, 256): thread tid adds c = tid, tid + 256, ...
    w = _butterfly(thr.reshape(M, 4, 64))
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def emu_ln_rows(dy, x, gam, dres, form, mutant=None):
    dy, x, gam = (np.asarray(a, f32) for a in (dy, x, gam))
    M, D = x.shape
    Df = f32(D)
    mean = (_row_sum(x, form) / Df)[:, None]
    d = x - mean
    var = _row_sum(d * d, form) / Df
    with np.errstate(divide="ignore", invalid="ignore"):          # the "no eps" mutant divides by zero on a constant row
        rstd = (f32(1) / np.sqrt((var if mutant == "no eps" else var + f32(1e-5)).astype(np.float64))).astype(f32)[:, None]
        xh = d * rstd
    g = dy * gam
    ma, mb = (_row_sum(g, form) / Df)[:, None], (_row_sum(g * xh, form) / Df)[:, None]
    v = rstd * (g - ma - (f32(0) if mutant == "xhat mb" else xh * mb))
    if dres is not None and mutant != "dres":
        v = v + np.asarray(dres, f32)
    st = np.concatenate([mean, rstd], 1)
    return v.astype(f32), (st[:, ::-1].copy() if mutant == "stats swapped" else st)


def emu_ce(z, tg, V, L, t0, scale, mutant=None):
    z = np.asarray(z, f32)
    M, ld = z.shape
    dl = np.full((M, ld), np.nan, f32)
    loss = np.zeros(M, f32)
    for m in range(M):
        if m % L < t0 and mutant != "inactive":
            dl[m] = 0
            continue
        row = z[m, :V]
        mx = row.max()
        e = np.exp((row - mx).astype(f32)).astype(f32)
        pad = -(-V // 256) * 256
        ep = np.zeros(pad, f32)
        ep[:V] = e
        thr = _serial(ep.reshape(pad // 256, 256))
        w = _butterfly(thr.reshape(4, 64))
        tot = (w[0] + w[1]) + (w[2] + w[3])
        oh = np.zeros(V, f32)
        k = int(tg[m]) + (1 if mutant == "onehot" else 0)
        if k < V:
            oh[k] = 1
        gr = e / tot - oh
        dl[m, :V] = gr if mutant == "scale" else gr * f32(scale)
        if mutant != "pad":
            dl[m, V:] = 0
        loss[m] = mx + np.log(tot).astype(f32) - row[int(tg[m])]
    return loss, dl


def emu_adamw(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, mutant=None):
    p, g, m, v = (np.asarray(a, f32) for a in (p, g, m, v))
    lr, b1, b2, eps, wd, bc1, bc2 = (f32(a) for a in (lr, b1, b2, eps, wd, bc1, bc2))
    if mutant == "no bias correction":
        bc1 = bc2 = f32(1)
    if mutant == "decay":
        wd = f32(0.01)
    if mutant == "launch lr":
        lr = f32(123.0)
    decay, sb2, step = f32(1) - lr * wd, np.sqrt(bc2), lr / bc1
    mi = b1 * m + (f32(1) - b1) * g
    vi = b2 * v + (f32(1) - b2) * g * g
    den = np.sqrt(vi + eps) / sb2 if mutant == "eps in sqrt" else np.sqrt(vi) / sb2 + eps
    return (p * decay - step * (mi / den)).astype(f32), mi.astype(f32), vi.astype(f32)


def emu_attention(qkv, dy, B, L, H, mask, mutant=None):
    """attn_train_fwd_kernel + attn_delta_kernel + attn_bwd_fused_kernel in f32 numpy: 64-key blocks, online softmax, recompute backward."""
    D = 64 * H
    x = np.asarray(qkv, f32)
    hd = lambda a: a.reshape(B, L, H, 64).transpose(0, 2, 1, 3)
    q, k, v, do = hd(x[:, :D]), hd(x[:, D:2 * D]), hd(x[:, 2 * D:]), hd(np.asarray(dy, f32))
    mk = np.ones((B, H, L, L), f32) if mask is None else np.asarray(mask, f32)
    live = np.tril(np.ones((L, L), bool))
    qs = q * f32(0.125)
    s = _qk(qs, k).astype(f32)
    mrun = np.full((B, H, L, 1), -np.inf, f32)
    lrun = np.zeros((B, H, L, 1), f32)
    o = np.zeros((B, H, L, 64), f32)
    for k0 in range(0, L, 64):
        sb = np.where(live[:, k0:k0 + 64], s[..., k0:k0 + 64], -np.inf).astype(f32)
        mnew = np.maximum(mrun, sb.max(-1, keepdims=True))
        ms = np.where(np.isinf(mnew), f32(0), mnew)
        corr = np.exp(mrun - ms).astype(f32)
        pe = np.exp(sb - ms).astype(f32)
        lrun = lrun * corr + pe.sum(-1, keepdims=True, dtype=f32)
        o = o * corr + _pv(pe * mk[..., k0:k0 + 64], v[:, :, k0:k0 + 64]).astype(f32)
        mrun = mnew
    y = (o * (f32(1) / lrun)).astype(f32)
    lse = (mrun + np.log(lrun).astype(f32))[..., 0]
    delta = np.zeros_like(lse[..., None]) if mutant == "delta" else (y * do).sum(-1, keepdims=True, dtype=f32)
    lv = np.ones((L, L), bool) if mutant == "diagonal mask" else live
    if mutant == "diagonal mask":                     # only the diagonal 64-blocks lose their mask: later blocks are never visited
        lv = live | (np.arange(L)[:, None] // 64 == np.arange(L)[None, :] // 64)
    P = np.where(lv, np.exp(s - lse[..., None]), 0).astype(f32)
    dP = _qk(do, v).astype(f32)
    dS = (P * (dP * mk - delta)).astype(f32)
    dSq = dS.copy()
    if mutant == "key block":
        dSq[..., :64] = 0                             # dQ: the first key block is never added
    dq = _pv(dSq, k).astype(f32) * f32(0.125)
    dk = _tq(dS, qs).astype(f32)
    dv = _tq(P * mk, do).astype(f32)
    un = lambda a: a.transpose(0, 2, 1, 3).reshape(B * L, D)
    return un(y), lse, delta[..., 0], np.concatenate([un(dq), un(dk), un(dv)], 1)


# ---------------------------------------------------------------------------------------------------- teeth: column sums
def _cr_terms(M, N, seed):
    g = T._gen(seed)
    a, x = torch.randn(M, N, generator=g).numpy(), (torch.randn(M, N, generator=g) + 3).numpy()
    st = np.stack([torch.randn(M, generator=g).numpy() + 3, torch.rand(M, generator=g).numpy() + 0.5], 1).astype(f32)
    gt = ((a * (x - st[:, :1])).astype(f32) * st[:, 1:2]).astype(f32)
    return a, x, st, gt


def test_column_sum_emulations_inside_and_mutants_outside():
    worst = 0.0
    cases = [("plain", M, N) for M in T.COLSUM_M for N in T.COLSUM_N] + [("ws", M, N) for M, N in T.COLSUM_WS_CASES] \
        + [("col_reduce", M, N) for M in T.CR_M for N in (64, 68)]
    for kind, M, N in cases:
        a, x, st, gt = _cr_terms(M, N, M * 7 + N)
        prev = torch.randn(N, generator=T._gen(1)).numpy()
        n = R.colsum_depth(kind, M, N)
        for pv in (None, prev):
            s, b = R.colsum_ref(a, n, pv)
            r = R.ratio(emu_colsum(kind, a, pv), s, b)
            worst = max(worst, r)
            assert r <= 1.0, (kind, M, N)
        s, b = R.colsum_ref(a, n, prev)
        RS = 1 if kind == "plain" else R.colsum_slices(M, N) if kind == "ws" else R.col_reduce_slices(M)
        if -(-M // RS) >= 2:
            assert R.ratio(emu_colsum(kind, a, prev, mutant="lane"), s, b) > TEETH, (kind, M, N, "lane")
        if RS > 1:
            assert R.ratio(emu_colsum(kind, a, prev, mutant="slice"), s, b) > TEETH, (kind, M, N, "slice")
        assert R.ratio(emu_colsum(kind, a, prev, mutant="accumulate"), s, b) > TEETH, (kind, M, N, "accumulate")
        if kind == "col_reduce":
            sg, bg = R.colsum_ref(R.ln_param_terms(a, x, st), n + 3, prev)
            o1, o2 = emu_colsum(kind, a, (prev, prev), g=gt)
            assert R.ratio(o1, sg, bg) <= 1.0 and R.ratio(o2, s, b) <= 1.0, (M, "kind 1")
            o1, o2 = emu_colsum(kind, a, (prev, prev), g=gt, mutant="swap")
            assert R.ratio(o1, sg, bg) > TEETH and R.ratio(o2, s, b) > TEETH, (M, "swap")
    print(f"column sums: emulation worst error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------- teeth: GELU
def test_gelu_emulation_inside():
    for n in T.GELU_N:
        x, dy = T._gelu_x(n, n).numpy(), torch.randn(n, generator=T._gen(n + 1)).numpy()
        er = R._erf(x.astype(np.float64) * float(f32(0.70710678118654752))).astype(f32)
        y, b = R.gelu_ref(x)
        assert R.ratio((f32(0.5) * x * (f32(1) + er)).astype(f32), y, b) <= 1.0
        gp = f32(0.5) * (f32(1) + er) + x * f32(R.K_PDF) * np.exp((f32(-0.5) * x * x).astype(f32)).astype(f32)
        dx, bd = R.gelu_bwd_ref(dy, x)
        assert R.ratio((dy * gp).astype(f32), dx, bd) <= 1.0
        assert R.ratio((dy * (gp - f32(0.5) * (f32(1) + er))).astype(f32), dx, bd) > TEETH or n == 1      # the Phi term dropped


# ---------------------------------------------------------------------------------------------------- teeth: LayerNorm
@pytest.mark.parametrize("D", T.LN_D_WAVE + T.LN_D_BLOCK)
def test_layernorm_emulation_inside_and_mutants_outside(D):
    form, ns = R.ln_rows_form(D), R.ln_sum_depth(D)
    for M in T.LN_M:
        x, dy, gam, dres = (t.numpy() for t in T.ln_inputs(M, D, M * 10000 + D))
        for res in (dres, None):
            ref = R.ln_bwd_rows_ref(dy, x, gam, res, ns)
            dx, st = emu_ln_rows(dy, x, gam, res, form)
            assert R.ratio(dx, ref["dx"], ref["b_dx"]) <= 1.0 and R.ratio(st, ref["stats"], ref["b_stats"]) <= 1.0, (M, D)
        ref = R.ln_bwd_rows_ref(dy, x, gam, dres, ns)
        wide = lambda got, key: R.ratio(got, ref[key], ref["b_" + key])
        assert wide(emu_ln_rows(dy, x, gam, dres, form, "stats swapped")[1], "stats") > TEETH, (M, D)
        assert wide(emu_ln_rows(dy, x, gam, dres, form, "xhat mb")[0], "dx") > TEETH, (M, D)
        assert wide(emu_ln_rows(dy, x, gam, dres, form, "dres")[0], "dx") > TEETH, (M, D)
        if M >= 3:                                                  # the constant row
            dxm, stm = emu_ln_rows(dy, x, gam, dres, form, "no eps")
            assert max(R.ratio(stm[1], ref["stats"][1], ref["b_stats"][1]), R.ratio(dxm[1], ref["dx"][1], ref["b_dx"][1])) > TEETH, (M, D)


def test_layernorm_three_launch_emulation_inside():
    """sfmi_layernorm_bwd_f32: the block form at every width, parameter sums through the two-stage column sum"""
    for M, D in T.LN_FULL_CASES[:2] + [(2100, 192)]:
        x, dy, gam, dres = (t.numpy() for t in T.ln_inputs(M, D, M + D))
        ref = R.ln_bwd_rows_ref(dy, x, gam, dres, -(-D // 256) + 8)
        dx, st = emu_ln_rows(dy, x, gam, dres, "block")
        assert R.ratio(dx, ref["dx"], ref["b_dx"]) <= 1.0 and R.ratio(st, ref["stats"], ref["b_stats"]) <= 1.0
        g0 = torch.randn(D, generator=T._gen(1)).numpy()
        terms = ((dy * (x - st[:, :1])).astype(f32) * st[:, 1:2]).astype(f32)
        n = R.colsum_depth("ws", M, D)
        s, b = R.colsum_ref(R.ln_param_terms(dy, x, st), n + 3, g0)
        assert R.ratio(emu_colsum("ws", terms, g0), s, b) <= 1.0


# ---------------------------------------------------------------------------------------------------- teeth: cross entropy
def _ce_inputs(V, ld, L, B):
    M = B * L
    g = T._gen(V * 1000 + L * 10 + B)
    z = torch.randn(M, ld, generator=g) * 3
    z[M // 2, :V] = torch.where(torch.rand(V, generator=g) < 0.5, 80.0, -80.0)
    tg = torch.randint(0, V, (M,), generator=g)
    tg[0], tg[-1] = 0, V - 1
    return z.numpy(), tg.numpy(), 1.0 / (M + 1)


@pytest.mark.parametrize("V,ld", T.CE_VLD)
def test_cross_entropy_emulation_inside_and_mutants_outside(V, ld):
    for L in T.CE_L:
        for B in T.CE_B:
            z, tg, scale = _ce_inputs(V, ld, L, B)
            for t0 in sorted({0, L - 1}):
                ref = R.ce_ref(z, tg, V, L, t0, scale)
                loss, dl = emu_ce(z, tg, V, L, t0, scale)
                assert R.ratio(loss, ref["loss"], ref["b_loss"]) <= 1.0 and R.ratio(dl, ref["dlogits"], ref["b_dl"]) <= 1.0, (V, L, B, t0)
                # (V = 1: softmax - onehot is exactly 0, so an omitted scale or a row that should have been zeroed changes nothing there;
                #  ld = V: there are no pad columns)
                for mutant in ("onehot",) + (("pad",) if ld > V else ()) + (("scale",) if V > 1 else ()) + (("inactive",) if t0 > 0 and V > 1 else ()):
                    _, dm = emu_ce(z, tg, V, L, t0, scale, mutant)
                    assert R.ratio(dm, ref["dlogits"], ref["b_dl"]) > TEETH, (V, L, B, t0, mutant)


# ---------------------------------------------------------------------------------------------------- teeth: scatter, dropout
@pytest.mark.parametrize("D", T.SCATTER_D)
def test_scatter_references_and_mutants(D):
    rows = T.SCATTER_ROWS
    g = T._gen(D)
    for idx in (np.full(2048, 7), np.concatenate([[0, rows - 1, 0], torch.randint(0, rows, (496,), generator=g).numpy()])):
        for sc in T.SCATTER_SCALES:
            dx = (torch.randn(len(idx), D, generator=g) * sc).numpy()
            exact = R.scatter_fixed_ref(dx, idx, rows)
            s, b = R.scatter_ref(dx, idx, rows)
            assert R.ratio(exact, s, b) <= 1.0
            # truncation instead of round-to-nearest: the BIT-EXACT gate sees it (it stays inside twice the float64 bound).  At scale 1
            # an f32 of magnitude >= 2^-9 times 2^32 is an integer already: the mutant only moves the rare smaller values by < 2^-32 and
            # the final rounding to f32 hides that - it is observable (and asserted) at the two smaller scales
            tr = R.scatter_fixed_ref(dx, idx, rows, trunc=True)
            assert sc > 1e-4 or not np.array_equal(tr.view(np.int32), exact.view(np.int32))
            assert R.ratio(tr, s, b) <= 2.0 + 1e-9
            # one duplicate row lost: the float64 gate sees it wherever the values are above the fixed-point quantum; the bit-exact gate always
            lost = R.scatter_fixed_ref(dx[1:], idx[1:], rows)
            assert not np.array_equal(lost.view(np.int32), exact.view(np.int32))
            if sc >= 1e-4:
                assert R.ratio(lost, s, b) > TEETH, (D, sc)


def test_dropout_mask_arithmetic_and_mutants():
    from shapeformer_amd import weights as W
    key = "dropout-k7-L0.attn"
    seed = W._fnv1a32(key)
    assert np.array_equal(R.hash_unit_idx(seed, np.arange(5000)), W.hash_unit(key, 5000))          # weights.hash_unit's arithmetic
    x = torch.randn(4096, generator=T._gen(1)).numpy()
    for p in (0.1, 0.9):
        good = x * R.dropout_mul(seed, np.arange(4096), p)
        assert not np.array_equal(good, x * R.dropout_mul(seed, np.arange(4096) + 1, p))           # index off by one
        assert not np.array_equal(good, x * (R.dropout_mul(seed, np.arange(4096), p) != 0))        # inv_keep omitted
        assert np.array_equal(good == 0, R.hash_unit_idx(seed, np.arange(4096)) < f32(p))
    assert np.array_equal(x * R.dropout_mul(seed, np.arange(4096), 0.0), x)
    m = R.attn_mask(seed, 2, 3, 5, 0.5)
    assert m[1, 2, 3, 4] == R.dropout_mul(seed, np.array([((1 * 3 + 2) * 5 + 3) * 5 + 4]), 0.5)[0]
    assert not np.array_equal(m, R.attn_mask(seed, 2, 3, 5, 0.5, swap=True))


# ---------------------------------------------------------------------------------------------------- teeth: AdamW
@pytest.mark.parametrize("step", T.ADAM_STEPS)
def test_adamw_emulation_inside_and_mutants_outside(step):
    hp = T.ADAM_HP
    g = T._gen(step)
    bc = (f32(1) - f32(np.float64(f32(hp["b1"])) ** step), f32(1) - f32(np.float64(f32(hp["b2"])) ** step))
    ref_bc, bb = R.bias_corrections_ref(hp["b1"], hp["b2"], step)
    assert (np.abs(np.array(bc, np.float64) - ref_bc) <= bb).all()
    caught = {m: 0.0 for m in ("no bias correction", "decay", "eps in sqrt", "launch lr")}
    for n, wd, sc in zip(T.ADAM_LENS, T.ADAM_WD, T.ADAM_GSCALE):
        p, gr = torch.randn(n, generator=g).numpy(), (torch.randn(n, generator=g) * sc).numpy()
        m = (torch.randn(n, generator=g) * 0.1).numpy() if step > 1 and sc else np.zeros(n, f32)
        v = (torch.rand(n, generator=g) * 0.01).numpy() if step > 1 and sc else np.zeros(n, f32)
        args = (p, gr, m, v, hp["lr"], hp["b1"], hp["b2"], hp["eps"], wd, bc[0], bc[1])
        ref = R.adamw_ref(*args)
        got = emu_adamw(*args)
        for name, a in zip("pmv", got):
            assert R.ratio(a, ref[name], ref["b_" + name]) <= 1.0, (step, n, name)
        assert np.isfinite(got[0]).all()
        for mu in caught:
            if mu == "decay" and wd != 0:
                continue
            caught[mu] = max(caught[mu], R.ratio(emu_adamw(*args, mutant=mu)[0], ref["p"], ref["b_p"]))
    assert caught["decay"] > TEETH and caught["launch lr"] > TEETH, caught
    if step <= 2:                                                    # 1 - 0.9^1000 and 1 - 0.95^1000 are exactly 1 in f32: nothing to drop there
        assert caught["no bias correction"] > TEETH, caught
    if step == 1:                                                    # v = 0 before the step: sqrt(v' + eps) is far from sqrt(v') + eps
        assert caught["eps in sqrt"] > TEETH, caught


# ---------------------------------------------------------------------------------------------------- teeth: attention
@pytest.mark.parametrize("B,L,H", T.ATTN_CASES)
def test_attention_emulation_inside_and_mutants_outside(B, L, H):
    D = 64 * H
    g = T._gen(B * 1000 + L * 10 + H)
    qkv, dy = torch.randn(B * L, 3 * D, generator=g).numpy(), torch.randn(B * L, D, generator=g).numpy()
    for p in T.ATTN_P:
        seed = 0x51ED270B + L
        mask = R.attn_mask(seed, B, H, L, p) if p else None
        fw = R.attn_fwd_ref(qkv, B, L, H, mask)
        bw = R.attn_bwd_ref(fw, dy, B, L, H)
        y, lse, delta, dqkv = emu_attention(qkv, dy, B, L, H, mask)
        assert R.ratio(y, fw["y"], fw["b_y"]) <= 1.0 and R.ratio(lse, fw["lse"], fw["b_lse"]) <= 1.0, (B, L, H, p)
        dref, dbound = R.delta_ref(y, dy, B, L, H)
        assert R.ratio(delta, dref, dbound) <= 1.0 and R.ratio(delta, bw["delta"], bw["b_delta"]) <= 1.0
        assert R.ratio(dqkv, bw["dqkv"], bw["b_dqkv"]) <= 1.0, (B, L, H, p)
        if B > 1 and L > 64:
            continue                                  # the mutants at this length run in the B = 1 case: the emulation has no launch forms
        wide = lambda mu, mk=mask: R.ratio(emu_attention(qkv, dy, B, L, H, mk, mu)[3], bw["dqkv"], bw["b_dqkv"])
        if L > 1:
            assert wide("delta") > TEETH and wide("diagonal mask") > TEETH, (B, L, H, p)
        if L > 64:
            assert wide("key block") > TEETH, (B, L, H, p)
        if p and L > 1:
            sw = R.attn_mask(seed, B, H, L, p, swap=True)
            ys, _, _, ds = emu_attention(qkv, dy, B, L, H, sw)
            assert R.ratio(ys, fw["y"], fw["b_y"]) > TEETH and R.ratio(ds, bw["dqkv"], bw["b_dqkv"]) > TEETH, (B, L, H, "mask swapped")
