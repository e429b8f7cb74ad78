"""CondTupleGPT.SKIP_ENDED on the device: rows that have ended are no longer streamed by the decode attention, sampled from logits or
(whole row groups) multiplied by the decode GEMMs - and seq / len / logp stay bit for bit what they were, and what the CPU oracle
draws.  Tiny model of tests/test_gpt_gpu.py, 24 steps, stop_early off; conditions and oracle tokens: tests/skip_ended_ref.py.

`python tests/test_skip_ended_gpu.py chains2x96` runs the two-chain case in a process of its own (the test starts it under a time
limit: a chain whose attention launches do nothing must keep releasing the attention turnstile) and prints one JSON line."""
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
KEEP = ("seq", "len", "logp", "alen", "resid", "qkv", "y", "h", "logit")


def _gpt(dev):
    from shapeformer_amd.gpt import CondTupleGPT
    return CondTupleGPT(R.model()[0], device=dev, **R.KW)


def _states(g, r):
    """The chain states behind a `to_host=False` result, cloned (the next run reuses the buffers)."""
    sts = [r["state"]] if "alen" in r["state"] else [g._states[k] for k in sorted(g._states) if k >= 100]
    return [{k: st[k].clone() for k in KEEP} for st in sts]


def _run(g, case, skip, **kw):
    kinds, seed = R.CASES[case]
    c, Lc = R.conditions(kinds)
    g.SKIP_ENDED = skip
    args = dict(max_steps=R.STEPS, seed=seed, stop_early=False)
    args.update(kw)
    if case == "chains2x96":
        g.ATTN_LANES = 1
        r = g.sample_microbatched(torch.from_numpy(c), torch.from_numpy(Lc), n_micro=2, **args)
    else:
        r = g.sample(torch.from_numpy(c), torch.from_numpy(Lc), to_host=False, shared_prefix=(case == "shared16"), **args)
    torch.cuda.synchronize()
    sts = _states(g, r)
    g.last_sem = g._sem.cpu().tolist()      # the turnstile words are re-armed by every multi-chain run
    return {k: torch.cat([st[k] for st in sts], 0) for k in ("seq", "len", "logp", "alen")}, sts, Lc


def _check_case(g, case):
    """SKIP_ENDED on against off, the oracle's tokens, finite chain state, alen.  Returns figures of the run."""
    kinds, _ = R.CASES[case]
    B = len(kinds)
    on, sts, Lc = _run(g, case, True)
    sem_on = g.last_sem
    off, _, _ = _run(g, case, False)
    for k in ("seq", "len"):
        assert torch.equal(on[k], off[k]), k
    assert torch.equal(on["logp"].view(torch.int32), off["logp"].view(torch.int32))      # bit patterns: +0.0 and -0.0 differ
    assert torch.equal(off["alen"], off["len"])                                             # not armed: alen follows len
    seq, ln = on["seq"].cpu().numpy(), on["len"].cpu().numpy()
    assert np.array_equal(ln, Lc + R.STEPS)
    tok = np.stack([seq[b, Lc[b]:Lc[b] + R.STEPS] for b in range(B)])
    ref = R.oracle_tokens(case)
    assert np.array_equal(tok, ref), f"{int((tok != ref).any(-1).sum())} tokens differ from the oracle"
    # the preconditions of the case, asserted on the result: every early row has ended with steps to spare, every live row never
    fe = R.first_end_step(tok)
    early = np.array([k == "E" for k in kinds])
    assert fe[early].max() <= R.STEPS - 4 and (fe[~early] == R.STEPS).all()
    ended = seq[np.arange(B), ln - 1, 0] == R.END[0]
    assert np.array_equal(ended, early)
    alen = on["alen"].cpu().numpy()
    assert np.array_equal(alen, np.where(ended, -1, ln))
    for st in sts:
        for k in ("resid", "qkv", "y", "h"):
            assert bool(torch.isfinite(st[k]).all()), k
        assert bool(torch.isfinite(st["logit"][:, :g.V]).all())      # (the padding columns of the logits rows are never written)
    return dict(first_end=fe, early=early, sem=sem_on)


def test_rows96_one_chain(dev):
    """The product's launch form: two GEMM row groups of three tiles.  Group 0 (rows 0-47) dies completely, group 1 holds mixed tiles."""
    f = _check_case(_gpt(dev), "rows96")
    assert f["early"][:48].all() and f["early"][48::2].all() and not f["early"][49::2].any()


def test_rows50_ragged_tile(dev):
    _check_case(_gpt(dev), "rows50")


def test_shared_prefix_16_rows(dev):
    """The shared-prefix attention instance; the copies of one early condition end at different steps through their uniforms."""
    f = _check_case(_gpt(dev), "shared16")
    assert len(set(f["first_end"].tolist())) >= 4


def test_unarmed_runs_leave_alen_equal_len(dev):
    """Logits history, teacher forcing and mask_invalid off: ended rows are not skipped, alen follows len."""
    g = _gpt(dev)
    ref = R.oracle_tokens("rows50")
    for kw in (dict(return_logits=True), dict(force_tokens=ref), dict(mask_invalid=False)):
        got, _, _ = _run(g, "rows50", True, **kw)
        assert torch.equal(got["alen"], got["len"]), kw.keys()
        assert int(got["alen"].min()) > 0


def _chains_main():
    g = _gpt(torch.device("cuda:0"))
    f = _check_case(g, "chains2x96")
    print(json.dumps(dict(ok=True, sem=f["sem"], chain0_all_ended_at=int(f["first_end"][:96].max()))))


def test_two_chains_turnstile_keeps_turning(dev):
    """2 chains x 96 rows, one attention lane; chain 0 is all early: from step 17 on its attention launches stream nothing and must
    still release the turnstile for chain 1.  Own process, under a time limit sized to seconds."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "chains2x96"], capture_output=True, text=True, timeout=180, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    tickets, finished, timeouts = out["sem"][:3]
    assert out["ok"] and timeouts == 0 and tickets == finished
    assert tickets == 2 * 3 * R.STEPS      # the turnstile was on in the SKIP_ENDED run: 2 chains x 3 layers x 24 steps gated launches


if __name__ == "__main__":
    assert sys.argv[1:] == ["chains2x96"]
    _chains_main()
