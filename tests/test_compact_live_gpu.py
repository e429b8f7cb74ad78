"""CondTupleGPT.COMPACT_LIVE on the device: at the head of every decode step the chain's live rows are packed into the slots
0 .. nlive-1 of the activation buffers and the decode GEMMs run only the row tiles that hold a live slot - and seq / len / logp stay
bit for bit what they are with the rows in place, with SKIP_ENDED off, and what the CPU oracle draws.  Tiny model, conditions and
helpers of tests/skip_ended_ref.py (24 steps, "E" rows end early, "L" rows stay live), stop_early off.

`python tests/test_compact_live_gpu.py chains2x96` runs the two-chain case in a process of its own (the test starts it under a time
limit: a chain whose launches do nothing must keep releasing the attention turnstile) and prints one JSON line."""
import functools
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

import skip_ended_ref as R      # noqa: E402

pytestmark = pytest.mark.gpu
KEEP = ("seq", "len", "logp", "alen", "resid", "qkv", "y", "h", "logit", "cnt", "slot_of", "row_of", "nlive", "emb")

# (kinds of the rows, seed); the oracle was run on these beforehand: every "E" row ends by step 18, every "L" row never (asserted below)
CASES = {
    "scatter96": ("E" * 48 + "EL" * 24, 11),      # live count 96, 93, 90, 84, 70, 62, 56, 40, 38, ... 24: every tile and the group boundary
    "live_first96": ("L" * 40 + "E" * 56, 25),    # identity map for the survivors; a half-filled last tile in group 0, group 1 empty
    "one_live96": ("E" * 95 + "L", 21),           # one live row moves from row 95 to slot 0
    "fill16": ("EL" * 16, 22),                    # live count settles at exactly 16 ...
    "spill17": ("EL" * 16 + "L", 23),             # ... and at 17: ceil(nlive / 16)
    "all_end32": ("E" * 32, 24),                  # nlive reaches 0: every GEMM workgroup and attention item leaves
    "shared16": R.CASES["shared16"],              # sample(shared_prefix=True): the condition is read from cache row 0
    "chains2x96": ("E" * 96 + "LE" * 48, 26),     # chain 0 runs empty while chain 1 goes on
    "rows50": R.CASES["rows50"],                  # the unarmed runs
}


@functools.lru_cache(maxsize=None)
def oracle_tokens(case):
    """As skip_ended_ref.oracle_tokens, for the cases of this file: (B, STEPS, 2) tokens of oracle.gpt_oracle.sample_indices; rows of
    one kind go through the oracle as one batch, the greedy row is global row 0."""
    from oracle import gpt_oracle as GO
    kinds, seed = CASES[case]
    B = len(kinds)
    _, sd_t, cfg = R.model()
    c, Lc = R.conditions(kinds)
    u = GO.uniforms(seed, R.STEPS, B)
    out = np.zeros((B, R.STEPS, 2), np.int64)
    for k in "EL":
        rows = [b for b in range(B) if kinds[b] == k]
        if not rows:
            continue
        cb = torch.from_numpy(c[rows][:, :Lc[rows[0]]])
        tok, _, _ = GO.sample_indices(sd_t, cfg, cb, R.STEPS, u[:, :, rows], use_cache=True, stop_early=False,
                                      best_in_first=(rows[0] == 0), return_logits=False)
        out[rows] = tok
    return out


def _gpt(dev):
    from shapeformer_amd.gpt import CondTupleGPT
    return CondTupleGPT(R.model()[0], device=dev, **R.KW)


def _run(g, case, compact, skip=True, **kw):
    kinds, seed = CASES[case]
    c, Lc = R.conditions(kinds)
    g.SKIP_ENDED, g.COMPACT_LIVE = skip, compact
    args = dict(max_steps=R.STEPS, seed=seed, stop_early=False)
    args.update(kw)
    if case == "chains2x96":
        g.ATTN_LANES = 1
        r = g.sample_microbatched(torch.from_numpy(c), torch.from_numpy(Lc), n_micro=2, **args)
    else:
        r = g.sample(torch.from_numpy(c), torch.from_numpy(Lc), to_host=False, shared_prefix=(case == "shared16"), **args)
    torch.cuda.synchronize()
    sts = [r["state"]] if "alen" in r["state"] else [g._states[k] for k in sorted(g._states) if k >= 100]
    sts = [{k: st[k].clone() for k in KEEP} for st in sts]      # (the next run reuses the buffers)
    g.last_sem = g._sem.cpu().tolist()      # the turnstile words are re-armed by every multi-chain run
    return {k: torch.cat([st[k] for st in sts], 0) for k in ("seq", "len", "logp", "alen")}, sts, Lc


def _stable_compaction(alen):
    """(slot_of, row_of, nlive) of one chain's alen: live rows first, ended rows behind them, both in ascending row order."""
    live = alen >= 0
    rows = np.arange(len(alen))
    slot_of = np.where(live, np.cumsum(live) - 1, -1)
    return slot_of, np.concatenate([rows[live], rows[~live]]), int(live.sum())


def _check_case(g, case):
    """COMPACT_LIVE on against off, against SKIP_ENDED off, against the oracle's tokens; alen, finite state, split-K tickets, the map."""
    kinds, _ = CASES[case]
    B = len(kinds)
    on, sts, Lc = _run(g, case, True)
    sem_on = g.last_sem
    for what, other in (("COMPACT_LIVE off", _run(g, case, False)[0]), ("SKIP_ENDED off", _run(g, case, False, skip=False)[0])):
        for k in ("seq", "len"):
            assert torch.equal(on[k], other[k]), (what, k)
        assert torch.equal(on["logp"].view(torch.int32), other["logp"].view(torch.int32)), what      # bit patterns: +0.0 and -0.0 differ
    seq, ln = on["seq"].cpu().numpy(), on["len"].cpu().numpy()
    assert np.array_equal(ln, Lc + R.STEPS)
    tok = np.stack([seq[b, Lc[b]:Lc[b] + R.STEPS] for b in range(B)])
    ref = oracle_tokens(case)
    assert np.array_equal(tok, ref), f"{int((tok != ref).any(-1).sum())} tokens differ from the oracle"
    # the preconditions of the case, asserted on the oracle's tokens: every early row has ended with steps to spare, every live row never
    fe = R.first_end_step(ref)
    early = np.array([k == "E" for k in kinds])
    assert (not early.any() or fe[early].max() <= R.STEPS - 4) and (fe[~early] == R.STEPS).all()
    ended = seq[np.arange(B), ln - 1, 0] == R.END[0]
    assert np.array_equal(ended, early)
    alen = on["alen"].cpu().numpy()
    assert np.array_equal(alen, np.where(ended, -1, ln))
    lo = 0
    for st in sts:
        for k in ("resid", "qkv", "y", "h"):
            assert bool(torch.isfinite(st[k]).all()), k
        assert bool(torch.isfinite(st["logit"][:, :g.V]).all())      # (the padding columns of the logits rows are never written)
        assert int(st["cnt"].abs().max()) == 0                       # split-K tickets: every tile that ran re-armed its word, no other was touched
        # the map of the last step (no row ends in the last four steps, so it is the compaction of the final alen)
        n = st["slot_of"].shape[0]
        slot_of, row_of, nlive = _stable_compaction(alen[lo:lo + n])
        assert np.array_equal(st["slot_of"].cpu().numpy(), slot_of)
        assert np.array_equal(st["row_of"].cpu().numpy()[:n], row_of) and (st["row_of"].cpu().numpy()[n:] == -1).all()
        assert int(st["nlive"]) == nlive
        lo += n
    # live rows at the head of every step (a row that ends at step s is live through step s)
    nlive_steps = np.array([int((fe >= j).sum()) for j in range(R.STEPS)])
    return dict(first_end=fe, early=early, sem=sem_on, nlive_steps=nlive_steps)


def test_scatter96_crosses_every_tile_boundary(dev):
    """The product's launch form (two row groups of three tiles).  The live count falls from 96 to 24 through every tile count; the 24
    survivors sit at odd rows of the second group and end in slots 0-23."""
    f = _check_case(_gpt(dev), "scatter96")
    tiles = set(((f["nlive_steps"] + 15) // 16).tolist())
    assert tiles == {6, 5, 4, 3, 2} and f["nlive_steps"][-1] == 24
    assert f["early"][:48].all() and f["early"][48::2].all() and not f["early"][49::2].any()


def test_live_first96_identity_map(dev):
    f = _check_case(_gpt(dev), "live_first96")
    assert f["nlive_steps"][-1] == 40


def test_one_live96_row_95_in_slot_0(dev):
    f = _check_case(_gpt(dev), "one_live96")
    assert f["nlive_steps"][-1] == 1


def test_fill16_and_spill17(dev):
    g = _gpt(dev)
    assert _check_case(g, "fill16")["nlive_steps"][-1] == 16
    assert _check_case(g, "spill17")["nlive_steps"][-1] == 17


def test_all_end32_runs_empty(dev):
    f = _check_case(_gpt(dev), "all_end32")
    # the oracle's last row ends at step 17: the chain is empty at the head of steps 18 .. 23
    assert f["first_end"].max() == 17 and np.array_equal(np.flatnonzero(f["nlive_steps"] == 0), np.arange(18, R.STEPS))


def test_shared_prefix_16_rows(dev):
    """The shared-prefix attention instance: the condition comes from cache row 0 whether or not row 0 still holds a slot."""
    f = _check_case(_gpt(dev), "shared16")
    assert len(set(f["first_end"].tolist())) >= 4      # the copies end at different steps: the map changes while the condition is read


def test_unarmed_runs_keep_the_identity_map(dev):
    """Logits history, teacher forcing and mask_invalid off: rows are neither skipped nor packed.  Same seq / logp bits as with
    COMPACT_LIVE off (and, where mask_invalid is on, the oracle's tokens), and no launch of the packed path ran: the staging buffer,
    which only the packed chain's embedding and stage-1 sampler tail write, keeps a sentinel."""
    g = _gpt(dev)
    ref = R.oracle_tokens("rows50")
    B = len(CASES["rows50"][0])
    SENT = -7.25
    for kw in (dict(return_logits=True), dict(force_tokens=ref), dict(mask_invalid=False)):
        off, _, Lc = _run(g, "rows50", False, **kw)
        g._state["emb"].fill_(SENT)      # (the next run of the same shape reuses the chain state)
        got, sts, _ = _run(g, "rows50", True, **kw)
        assert torch.equal(got["seq"], off["seq"]) and torch.equal(got["len"], off["len"]), kw.keys()
        assert torch.equal(got["logp"].view(torch.int32), off["logp"].view(torch.int32)), kw.keys()
        if kw.get("mask_invalid", True):
            seq = got["seq"].cpu().numpy()
            assert np.array_equal(np.stack([seq[b, Lc[b]:Lc[b] + R.STEPS] for b in range(B)]), ref), kw.keys()
        assert torch.equal(got["alen"], got["len"]), kw.keys()
        st = sts[0]
        assert bool((st["emb"] == SENT).all()), kw.keys()
        assert int(st["nlive"]) == B
        assert np.array_equal(st["slot_of"].cpu().numpy(), np.arange(B))
        assert np.array_equal(st["row_of"].cpu().numpy()[:B], np.arange(B))


def _chains_main():
    g = _gpt(torch.device("cuda:0"))
    f = _check_case(g, "chains2x96")
    print(json.dumps(dict(ok=True, sem=f["sem"], chain0_all_ended_at=int(f["first_end"][:96].max()))))


def test_two_chains_turnstile_keeps_turning(dev):
    """2 chains x 96 rows, one attention lane; chain 0 is all early: once nlive is 0 its launches do nothing and must still release
    the turnstile for chain 1.  Own process, under a time limit sized to seconds."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chains2x96"], capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    tickets, finished, timeouts = out["sem"][:3]
    assert out["ok"] and timeouts == 0 and tickets == finished
    assert tickets == 2 * 3 * R.STEPS      # the turnstile was on in the COMPACT_LIVE run: 2 chains x 3 layers x 24 steps gated launches


# ---------------------------------------------------------------------------------------------------------------------------------
# sfmi_decode_gemm_rows_f32 alone, at the product's shapes: the rows of the live tiles have sfmi_decode_gemm_f32's bits, the others
# are not written
def _unpack(t, M, N):
    """fragment-packed [M/16][N/16][64][4] (csrc/gpt.hip pk_off) -> (M, N)"""
    return t.view(M // 16, N // 16, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(M, N)


@pytest.mark.parametrize("N,K,ln,act,res,S", [(3072, 1024, 1, 0, False, 1), (1024, 1024, 0, 0, True, 1),
                                              (4096, 1024, 1, 1, False, 1), (1024, 4096, 0, 0, True, 4)],
                         ids=["qkv_ln", "proj_resid", "fc1_ln_gelu", "fc2_splitk"])
def test_decode_gemm_rows_matches_full_launch(dev, N, K, ln, act, res, S):
    from shapeformer_amd import _lib as L
    from shapeformer_amd.gpt import CondTupleGPT
    S = CondTupleGPT.S_FC2 if S > 1 else 1
    M = 96
    gen = torch.Generator().manual_seed(N + K)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)
    w, bias, x = rnd(N, K) * K ** -0.5, rnd(N), rnd(M * K)
    gamma, beta = (1 + 0.1 * rnd(K), 0.1 * rnd(K)) if ln else (None, None)
    resid = rnd(M * N) if res else None
    wp, c1, c2 = torch.empty(N * K, device=dev), torch.empty(N, device=dev), torch.empty(N, device=dev)
    L.check(L.lib().sfmi_ln_fold_pack_f32(L.ptr(w), L.ptr(gamma), L.ptr(beta), L.ptr(bias), L.ptr(wp), L.ptr(c1), L.ptr(c2), N, K,
                                          L.stream_ptr()), "sfmi_ln_fold_pack_f32")
    slab = torch.empty(int(L.lib().sfmi_decode_gemm_slab_floats(M, N, S)), device=dev)
    cnt = torch.zeros(M // 16 * (N // 16), device=dev, dtype=torch.int32)
    sl, ct = (L.ptr(slab), L.ptr(cnt)) if S > 1 else (None, None)
    c1p = L.ptr(c1) if ln else None
    full = torch.empty(M * N, device=dev)
    L.check(L.lib().sfmi_decode_gemm_f32(L.ptr(x), L.ptr(wp), c1p, L.ptr(c2), L.ptr(resid), L.ptr(full), M, N, K, N, ln, act, 1, S,
                                         sl, ct, L.stream_ptr()), "sfmi_decode_gemm_f32")
    full = _unpack(full, M, N)
    assert bool(torch.isfinite(full).all())
    nl = torch.zeros(1, device=dev, dtype=torch.int32)
    SENT = 12345.0
    for nlive in (0, 1, 16, 17, 48, 49, 96):
        nl.fill_(nlive)
        out = torch.full((M * N,), SENT, device=dev)
        L.check(L.lib().sfmi_decode_gemm_rows_f32(L.ptr(x), L.ptr(wp), c1p, L.ptr(c2), L.ptr(resid), L.ptr(out), M, N, K, N, ln, act, 1,
                                                  S, sl, ct, L.ptr(nl), 1, L.stream_ptr()), "sfmi_decode_gemm_rows_f32")
        out = _unpack(out, M, N)
        run = (nlive + 15) // 16 * 16
        assert torch.equal(out[:nlive].view(torch.int32), full[:nlive].view(torch.int32)), nlive
        assert bool((out[run:] == SENT).all()), nlive
        assert int(cnt.abs().max()) == 0, nlive


if __name__ == "__main__":
    assert sys.argv[1:] == ["chains2x96"]
    _chains_main()
