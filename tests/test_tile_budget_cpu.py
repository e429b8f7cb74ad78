"""CondTupleGPT.TILE_BUDGET without a GPU: the policy that turns lagging live counts into row-tile budgets
(shapeformer_amd.gpt.tile_budget_policy), the precondition it rests on - a chain's live count never grows - asserted on the CPU
oracle's tokens for every case tests/test_tile_budget_gpu.py runs, and the ladder that arms it (shapeformer_amd.gpt.decode_level)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import skip_ended_ref as R                       # noqa: E402
import test_compact_live_gpu as C                # noqa: E402  (the cases and their cached oracle tokens; nothing there touches a GPU on import)
from shapeformer_amd.gpt import decode_level, tile_budget_policy      # noqa: E402

LOOP_CASES = ("scatter96", "one_live96", "fill16", "spill17", "all_end32", "chains2x96")


def _budgets(full, nlive_steps, every):
    """The budgets per block a loop of len(nlive_steps) steps takes: after block i's last step the host is sent the live count at the
    head of that step; block j is chosen from what blocks <= j - 2 sent."""
    nblocks = -(-len(nlive_steps) // every)
    sent = [int(nlive_steps[min((i + 1) * every, len(nlive_steps)) - 1]) for i in range(nblocks)]
    return [tile_budget_policy(full, sent[:max(j - 1, 0)], j) for j in range(nblocks)]


def _sequences():
    rng = np.random.default_rng(5)
    seqs = [np.full(40, 96), np.zeros(40, np.int64), np.arange(96, 0, -1), np.array([96] * 5 + [17] * 5 + [16] * 5 + [1] * 5 + [0] * 5),
            np.array([33, 32, 32, 31, 17, 16, 15, 1, 0, 0, 0, 0])]
    for _ in range(20):
        seqs.append(np.sort(rng.integers(0, 97, int(rng.integers(1, 70))))[::-1])
    return seqs


@pytest.mark.parametrize("every", [1, 3, 8, 16])
def test_budget_covers_every_later_step(every):
    """On a non-increasing live count no block's budget is below ceil(n / 16) of any of its own or any later step."""
    for nl in _sequences():
        assert (np.diff(nl) <= 0).all()
        full = 6
        bud = _budgets(full, nl, every)
        assert len(bud) == -(-len(nl) // every)
        for j, T in enumerate(bud):
            assert 1 <= T <= full
            assert T >= -(-int(nl[j * every:].max()) // 16), (nl.tolist(), every, j, T)


def test_full_budget_until_two_blocks_were_observed():
    """Blocks 0 and 1 run at the full budget whatever has been sent (block 1 may not even look at block 0's count: the host has not
    waited for it); block 2 is the first to follow block 0's count."""
    for full in (1, 2, 6, 12):
        assert tile_budget_policy(full, [], 0) == full
        assert tile_budget_policy(full, [], 1) == full
        assert tile_budget_policy(full, [0], 1) == full
        assert tile_budget_policy(full, [0, 0], 1) == full
    assert tile_budget_policy(6, [33], 2) == 3
    assert tile_budget_policy(6, [33, 1], 2) == 3          # block 1's count is not used for block 2
    assert tile_budget_policy(6, [33, 1], 3) == 1


def test_tile_arithmetic():
    assert tile_budget_policy(6, [0], 2) == 1               # nlive = 0: there is no empty form
    assert tile_budget_policy(6, [1], 2) == 1
    assert tile_budget_policy(6, [16], 2) == 1
    assert tile_budget_policy(6, [17], 2) == 2
    assert tile_budget_policy(6, [96], 2) == 6
    assert tile_budget_policy(2, [96], 2) == 2              # never above the chain's own tiles


@pytest.mark.parametrize("case", LOOP_CASES)
def test_reference_live_count_never_grows(case):
    """The precondition, on the reference's tokens (not on the code under test): a row that stood at the end position stays there, so
    the live count at the head of the steps falls monotonically - per chain for the two-chain case."""
    tok = C.oracle_tokens(case)
    at_end = tok[:, :, 0] == R.END[0]
    assert (at_end[:, 1:] >= at_end[:, :-1]).all()          # once ended, ended at every later step
    chains = [slice(0, 96), slice(96, 192)] if case == "chains2x96" else [slice(None)]
    for sl in chains:
        live_at_head = np.concatenate([[at_end[sl].shape[0]], (~at_end[sl]).sum(0)[:-1]])      # step j sees the ends of steps < j
        assert (np.diff(live_at_head) <= 0).all(), case
        fe = R.first_end_step(tok[sl])
        assert np.array_equal(live_at_head, [int((fe >= j).sum()) for j in range(R.STEPS)])


# decode_level, written out.  One string per (SKIP_ENDED, COMPACT_LIVE, TILE_BUDGET) and _profile; its 16 digits are the levels of the
# calls numbered 8 * mask_invalid + 4 * return_logits + 2 * (force_tokens given) + (an ablation set): only call 8 - masked, nobody looks
# at logits, nothing forced, nothing ablated - ever leaves level 0.  Packing needs the skip, budgets need the packing, and the timed GEMM
# launch ("gemm" in _profile) keeps budgets off.
PROFILES = ("", "attn", "attn,gemm")
LEVELS = {
    (False, False, False): ("0000000000000000", "0000000000000000", "0000000000000000"),
    (False, False, True): ("0000000000000000", "0000000000000000", "0000000000000000"),
    (False, True, False): ("0000000000000000", "0000000000000000", "0000000000000000"),
    (False, True, True): ("0000000000000000", "0000000000000000", "0000000000000000"),
    (True, False, False): ("0000000010000000", "0000000010000000", "0000000010000000"),
    (True, False, True): ("0000000010000000", "0000000010000000", "0000000010000000"),
    (True, True, False): ("0000000020000000", "0000000020000000", "0000000020000000"),
    (True, True, True): ("0000000030000000", "0000000030000000", "0000000020000000"),
}


def test_decode_level_table():
    assert len(LEVELS) == 8
    for switches, rows in LEVELS.items():
        for profile, row in zip(PROFILES, rows):
            for call in range(16):
                mask, logits, forced, ablated = (bool(call >> s & 1) for s in (3, 2, 1, 0))
                force = np.zeros((1, 1, 2), np.int64) if forced else None
                for ablate in (("gemm", "attn", "attn@1", "gemm@0,attn@1") if ablated else ("",)):      # any ablation, whole or per chain
                    got = decode_level(mask, logits, force, ablate, profile, *switches)
                    assert got == int(row[call]), (switches, profile, call, ablate, got)
