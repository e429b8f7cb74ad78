"""CondTupleGPT.TILE_BUDGET on the device: the decode loop replays, block by block, step graphs shaped for the row tiles a lagging
read of the chain's live count still needs - and seq / len / logp stay bit for bit what the full-form loop and the CPU oracle give.
Cases, tiny model and helpers of tests/test_compact_live_gpu.py / tests/skip_ended_ref.py (24 steps, stop_early off).

`python tests/test_tile_budget_gpu.py chains2x96` runs the two-chain case in a process of its own (the test starts it under a time
limit, as the packed chain's own test does) and prints one JSON line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import skip_ended_ref as R                  # noqa: E402
import test_compact_live_gpu as C           # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1


def _over(g, case):
    sts = [g._states[k] for k in sorted(g._states) if k >= 100] if case == "chains2x96" else [g._state]
    return [int(st["over"]) for st in sts]


def _run(g, case, budget, every=8, **kw):
    g.TILE_BUDGET, g.TILE_BUDGET_EVERY = budget, every
    g.last_budget_log = None
    out, sts, Lc = C._run(g, case, True, **kw)
    return out, sts, Lc, _over(g, case), g.last_budget_log


def _check_loop(g, case, ref_run=None):
    """TILE_BUDGET on (blocks of 1 and of 8 steps) against off and against the oracle's tokens; guard word, split-K tickets, the map of
    the last step, the budget log."""
    kinds, _ = C.CASES[case]
    B = len(kinds)
    off, _, Lc, over_off, log_off = ref_run or _run(g, case, False)
    assert not any(over_off) and all(len(l) == 0 for l in log_off)
    ref = C.oracle_tokens(case)
    fe = R.first_end_step(ref)
    sems = {}
    for every in (1, 8):
        on, sts, _, over, logs = _run(g, case, True, every)
        sems[every] = g.last_sem
        for k in ("seq", "len", "alen"):
            assert torch.equal(on[k], off[k]), (every, k)
        assert torch.equal(on["logp"].view(torch.int32), off["logp"].view(torch.int32)), every
        seq, ln = on["seq"].cpu().numpy(), on["len"].cpu().numpy()
        assert np.array_equal(ln, Lc + R.STEPS)
        tok = np.stack([seq[b, Lc[b]:Lc[b] + R.STEPS] for b in range(B)])
        assert np.array_equal(tok, ref), f"every {every}: {int((tok != ref).any(-1).sum())} tokens differ from the oracle"
        assert over == [0] * len(sts), (every, over)
        alen = on["alen"].cpu().numpy()
        lo = 0
        assert len(logs) == len(sts)
        for st, log in zip(sts, logs):
            assert int(st["cnt"].abs().max()) == 0, every
            n = st["slot_of"].shape[0]
            slot_of, row_of, nlive = C._stable_compaction(alen[lo:lo + n])
            assert np.array_equal(st["slot_of"].cpu().numpy(), slot_of)
            assert np.array_equal(st["row_of"].cpu().numpy()[:n], row_of) and (st["row_of"].cpu().numpy()[n:] == -1).all()
            assert int(st["nlive"]) == nlive
            # live rows at the head of every step of this chain, from the oracle's first-end steps; no block's budget is below any of its steps
            nlive_steps = np.array([int((fe[lo:lo + n] >= j).sum()) for j in range(R.STEPS)])
            full = (n + 15) // 16
            assert len(log) == -(-R.STEPS // every) and log[:2] == [full] * min(2, len(log))
            for j, T in enumerate(log):
                need = -(-int(nlive_steps[j * every:(j + 1) * every].max()) // 16)
                assert need <= T <= full, (every, j, T, need)
                if j >= 2:      # exactly the tiles of the count the host was sent two blocks earlier
                    assert T == max(1, -(-int(nlive_steps[(j - 1) * every - 1]) // 16)), (every, j, T)
            lo += n
    return dict(nlive_steps=np.array([int((fe >= j).sum()) for j in range(R.STEPS)]), logs=logs, sems=sems, first_end=fe)


def test_scatter96_replays_every_budget(dev):
    g = C._gpt(dev)
    f = _check_loop(g, "scatter96")
    assert f["nlive_steps"][-1] == 24
    _, _, _, _, logs = _run(g, "scatter96", True, 1)
    assert set(logs[0]) == {6, 5, 4, 3, 2}, logs[0]
    # the small budgets have graphs of their own (no aliasing configured): six distinct graphs were replayed from
    by_budget = g._graphs[0][2]
    assert sorted(by_budget) == [1, 2, 3, 4, 5, 6]
    forms = g.TILE_BUDGET_FORMS
    assert forms is not None or len({id(v) for v in by_budget.values()}) == 6


def test_one_live96(dev):
    f = _check_loop(C._gpt(dev), "one_live96")
    assert f["nlive_steps"][-1] == 1


def test_fill16_and_spill17(dev):
    g = C._gpt(dev)
    assert _check_loop(g, "fill16")["nlive_steps"][-1] == 16
    _, _, _, _, logs = _run(g, "fill16", True, 1)
    assert logs[0][-1] == 1
    assert _check_loop(g, "spill17")["nlive_steps"][-1] == 17
    _, _, _, _, logs = _run(g, "spill17", True, 1)
    assert logs[0][-1] == 2


def test_all_end32_stays_at_one_tile(dev):
    g = C._gpt(dev)
    f = _check_loop(g, "all_end32")
    assert f["nlive_steps"][-1] == 0
    _, _, _, _, logs = _run(g, "all_end32", True, 1)
    assert logs[0][-1] == 1 and min(logs[0]) == 1      # nlive = 0: there is no empty form


def _chains_main():
    g = C._gpt(torch.device("cuda:0"))
    f = _check_loop(g, "chains2x96")
    print(json.dumps(dict(ok=True, sems=f["sems"], logs=f["logs"])))


def test_two_chains_turnstile_keeps_turning(dev):
    """2 chains x 96 rows, one attention lane, chain 0 all early: every budget form keeps its gate and attention launch per layer, so
    the turnstile counts are those of the full form.  Own process, under a time limit."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chains2x96"], capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["ok"]
    for every, sem in out["sems"].items():
        tickets, finished, timeouts = sem[:3]
        assert timeouts == 0 and tickets == finished == 2 * 3 * R.STEPS, (every, sem)
    assert len(out["logs"]) == 2 and all(len(l) == 3 for l in out["logs"])      # blocks of 8: three budgets per chain


def test_unarmed_runs_use_the_full_graph_only(dev):
    """Logits history, teacher forcing and mask_invalid off: no budget graph exists, nothing is logged, results are those with the
    knob off."""
    g = C._gpt(dev)
    ref = R.oracle_tokens("rows50")
    B = len(C.CASES["rows50"][0])
    for kw in (dict(return_logits=True), dict(force_tokens=ref), dict(mask_invalid=False)):
        off, _, _, _, _ = _run(g, "rows50", False, **kw)
        got, sts, _, over, logs = _run(g, "rows50", True, 1, **kw)
        assert torch.equal(got["seq"], off["seq"]) and torch.equal(got["len"], off["len"]), kw.keys()
        assert torch.equal(got["logp"].view(torch.int32), off["logp"].view(torch.int32)), kw.keys()
        assert over == [0] and (logs is None or all(len(l) == 0 for l in logs)), kw.keys()
        assert int(sts[0]["nlive"]) == B
        cached = g._graphs.get(0)
        if cached is not None and "force_tokens" not in kw:
            assert sorted(cached[2]) == [(B + 15) // 16], kw.keys()


# ---------------------------------------------------------------------------------------------------------------------------------
# sfmi_decode_gemm_tiles_f32 alone: a 96-row chain at every budget; the smallest shapes that reach each launch path
GEMM_SHAPES = [  # N, K, S, ln, resid, row-major ldo (0: fragment-packed)
    pytest.param(48, 1024, 1, 1, False, 0, id="ln_fold_odd_tiles_un8"),
    pytest.param(32, 4096, 4, 0, True, 0, id="resid_splitk"),
    pytest.param(33, 1024, 1, 1, False, 36, id="logits_row_major"),
    pytest.param(32, 2048, 1, 0, False, 0, id="kslice2048_nw_pinned"),
]


def _gemm_setup(dev, N, K, S, ln, res, ldo):
    from shapeformer_amd import _lib as L
    M = 96
    Np = (N + 15) // 16 * 16
    gen = torch.Generator().manual_seed(1000 * N + K)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    w, bias, x = rnd(N, K) * K ** -0.5, rnd(N), rnd(M * K)
    gamma, beta = (1 + 0.1 * rnd(K), 0.1 * rnd(K)) if ln else (None, None)
    ld = ldo if ldo else N
    resid = rnd(M * ld) if res else None
    wp, c1, c2 = torch.empty(Np * K, device=dev), torch.empty(Np, device=dev), torch.empty(Np, device=dev)
    L.check(L.lib().sfmi_ln_fold_pack_f32(L.ptr(w), L.ptr(gamma), L.ptr(beta), L.ptr(bias), L.ptr(wp), L.ptr(c1), L.ptr(c2), N, K,
                                          L.stream_ptr()), "sfmi_ln_fold_pack_f32")
    slab = torch.empty(int(L.lib().sfmi_decode_gemm_slab_floats(M, N, S)), device=dev)
    cnt = torch.zeros(M // 16 * (Np // 16 + 1), device=dev, dtype=torch.int32)
    sl, ct = (L.ptr(slab), L.ptr(cnt)) if S > 1 else (None, None)
    nl = torch.zeros(1, device=dev, dtype=torch.int32)
    head = (L.ptr(x), L.ptr(wp), L.ptr(c1) if ln else None, L.ptr(c2), L.ptr(resid))
    tail = (N, K, ld, ln, 0, 0 if ldo else 1, S, sl, ct, L.ptr(nl), 1, L.stream_ptr())
    keep = (w, bias, x, gamma, beta, resid, wp, c1, c2, slab)
    return M, ld, nl, cnt, head, tail, keep


def _rows(t, M, N, ldo):
    return t.view(M, ldo) if ldo else C._unpack(t, M, N)


@pytest.mark.parametrize("N,K,S,ln,res,ldo", GEMM_SHAPES)
def test_decode_gemm_tiles_matches_the_96_row_launch(dev, N, K, S, ln, res, ldo):
    from shapeformer_amd import _lib as L
    lib = L.lib()
    M, ld, nl, cnt, head, tail, keep = _gemm_setup(dev, N, K, S, ln, res, ldo)
    SENT = 12345.0
    nl.fill_(M)
    full = torch.full((M * ld,), SENT, device=dev)
    L.check(lib.sfmi_decode_gemm_rows_f32(*head, L.ptr(full), M, *tail), "sfmi_decode_gemm_rows_f32")
    full = _rows(full, M, N, ldo)
    assert bool(torch.isfinite(full[:, :N]).all()) and not bool((full[:, :N] == SENT).any())
    for tiles in range(1, 7):
        for nlive in (0, 1, 16 * tiles - 15, 16 * tiles):
            nl.fill_(nlive)
            out = torch.full((M * ld,), SENT, device=dev)
            L.check(lib.sfmi_decode_gemm_tiles_f32(*head, L.ptr(out), M, tiles, *tail), "sfmi_decode_gemm_tiles_f32")
            out = _rows(out, M, N, ldo)
            assert torch.equal(out[:nlive, :N].view(torch.int32), full[:nlive, :N].view(torch.int32)), (tiles, nlive)
            assert bool((out[16 * tiles:] == SENT).all()), (tiles, nlive)
            assert int(cnt.abs().max()) == 0, (tiles, nlive)


def test_decode_gemm_tiles_refusals(dev):
    from shapeformer_amd import _lib as L
    lib = L.lib()
    M, ld, nl, cnt, head, tail, keep = _gemm_setup(dev, 32, 1024, 1, 0, False, 0)
    out = torch.zeros(M * ld, device=dev)
    call = lambda form_rows, tiles, tail_=tail: lib.sfmi_decode_gemm_tiles_f32(*head, L.ptr(out), form_rows, tiles, *tail_)
    assert call(96, 1) == 0 and call(96, 6) == 0
    assert call(96, 0) == EINVAL and call(96, -1) == EINVAL
    assert call(96, 7) == EINVAL                      # 16 * tiles beyond the padded rows of the chain
    assert call(17, 2) == 0 and call(17, 3) == EINVAL  # 17 rows pad to two tiles
    assert call(0, 1) == EINVAL and call(193, 1) == EINVAL
    no_nlive = tail[:9] + (None,) + tail[10:]
    assert call(96, 1, no_nlive) == EINVAL
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# the guard word of the compaction at a budget
def test_compaction_guard_word(dev):
    from shapeformer_amd import _lib as L
    lib = L.lib()
    B, D = 32, 64
    Bpad = int(lib.sfmi_decode_gemm_padded_rows(B))
    i32 = lambda n, v=0: torch.full((n,), v, device=dev, dtype=torch.int32)
    stage = torch.randn(B, D, generator=torch.Generator().manual_seed(3)).to(dev)

    def run(nlive, budget, plain=False):
        alen = i32(B, -1)
        alen[torch.arange(0, 2 * nlive, 2, device=dev)[:nlive] if nlive <= B // 2 else torch.arange(nlive, device=dev)] = 5
        slot_of, row_of, nl, slot_len, over = i32(B), i32(Bpad), i32(1), i32(Bpad), i32(1)
        resid = torch.zeros(Bpad * D, device=dev)
        a = (L.ptr(alen), L.ptr(slot_of), L.ptr(row_of), L.ptr(nl), L.ptr(slot_len), L.ptr(stage), L.ptr(resid), B, Bpad, D)
        if plain:
            L.check(lib.sfmi_gpt_compact_rows_f32(*a, L.stream_ptr()), "sfmi_gpt_compact_rows_f32")
        else:
            L.check(lib.sfmi_gpt_compact_rows_budget_f32(*a, budget, L.ptr(over), L.stream_ptr()), "sfmi_gpt_compact_rows_budget_f32")
        return int(over), int(nl), slot_of.cpu(), row_of.cpu(), slot_len.cpu(), resid.cpu()

    assert run(17, 1)[:2] == (1, 17)
    assert run(16, 1)[:2] == (0, 16)
    assert run(17, 2)[:2] == (0, 17) and run(32, 2)[:2] == (0, 32) and run(0, 1)[:2] == (0, 0)
    # everything else the launch writes is what the plain entry point writes
    got, want = run(17, 1), run(17, 0, plain=True)
    for a_, b_ in zip(got[1:], want[1:]):
        assert (torch.equal(a_, b_) if torch.is_tensor(a_) else a_ == b_)
    # refusals: no guard word, no budget, a budget beyond the padded rows
    alen, so, ro, nl, sl_, over = i32(B), i32(B), i32(Bpad), i32(1), i32(Bpad), i32(1)
    resid = torch.zeros(Bpad * D, device=dev)
    a = (L.ptr(alen), L.ptr(so), L.ptr(ro), L.ptr(nl), L.ptr(sl_), L.ptr(stage), L.ptr(resid), B, Bpad, D)
    assert lib.sfmi_gpt_compact_rows_budget_f32(*a, 1, None, L.stream_ptr()) == EINVAL
    assert lib.sfmi_gpt_compact_rows_budget_f32(*a, 0, L.ptr(over), L.stream_ptr()) == EINVAL
    assert lib.sfmi_gpt_compact_rows_budget_f32(*a, Bpad // 16 + 1, L.ptr(over), L.stream_ptr()) == EINVAL
    assert lib.sfmi_gpt_compact_rows_budget_f32(*a, Bpad // 16, L.ptr(over), L.stream_ptr()) == 0
    torch.cuda.synchronize()


def test_guard_raises_at_the_next_prepare(dev):
    """A guard word left set by a run is reported, and cleared, when the slot is prepared again."""
    from shapeformer_amd import _lib as L
    g = C._gpt(dev)
    _run(g, "fill16", True, 8)
    g._state["over"].fill_(1)
    with pytest.raises(L.SfmiError):
        _run(g, "fill16", True, 8)
    _run(g, "fill16", True, 8)      # cleared: the slot is usable again


if __name__ == "__main__":
    assert sys.argv[1:] == ["chains2x96"]
    _chains_main()
