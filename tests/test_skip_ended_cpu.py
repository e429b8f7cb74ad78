"""The invariant CondTupleGPT.SKIP_ENDED rests on, pinned with the oracle alone (no GPU): a row whose last position is the end
position, at step >= 1 and with mask_invalid on, can only draw (end0, end1), both with log-probability exactly 0 - whatever the
logits are.  With mask_invalid off it can draw anything, which is why the skip is not armed then."""
import numpy as np
import pytest

from oracle import tokens_oracle as TO

V, END = 4097, (4096, 4096)
L_COND = 3


def _idx(cur_pos):
    """(1, L_cond + 2, 2): a condition [10, 20, end], one generated token at the end position, and the token being sampled."""
    idx = np.array([[[10, 1], [20, 2], [END[0], END[1]], [END[0], END[1]], [cur_pos, 0]]], np.int64)
    assert idx.shape[1] == L_COND + 2
    return idx


def _logit_rows():
    rng = np.random.default_rng(0)
    rows = {"random": rng.standard_normal(V).astype(np.float32) * 3,
            "huge": (rng.standard_normal(V) * 1e30).astype(np.float32),
            "very negative": np.full(V, -3e38, np.float32),
            "max float": np.full(V, np.finfo(np.float32).max, np.float32),
            "end is the smallest": rng.standard_normal(V).astype(np.float32)}
    rows["end is the smallest"][END[0]] = -1e30
    return rows


def _draw(ml, greedy, u):
    """The oracle's draw from one masked row (oracle.gpt_oracle.sample_indices) and its log-probability as the sampler forms it:
    masked logit of the choice minus the log-sum-exp of the masked row, in float32."""
    if greedy:
        choice = int(np.argmax(ml))
    else:
        choice = TO.sample_filtered(TO.filter_sampling_logits(ml, 100, 0.4, 1.0), u)
    m = np.float32(ml.max())
    lse = m + np.log(np.exp(ml - m, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32)
    return choice, np.float32(ml[choice]) - lse


@pytest.mark.parametrize("completion", [True, False])
@pytest.mark.parametrize("step", [1, 7])
def test_ended_row_can_only_draw_the_end_pair(completion, step):
    for name, lg in _logit_rows().items():
        for greedy in (True, False):
            for u in (0.0, 0.37, 0.999999):
                m0 = TO.sampling_masker(lg[None], _idx(0), L_COND, step, 0, END, True, completion)[0]
                assert np.isfinite(m0).sum() == 1 and np.isfinite(m0[END[0]]), name      # exactly one finite entry: the end position
                pos, lp0 = _draw(m0, greedy, u)
                assert pos == END[0] and lp0 == 0.0 and not np.signbit(lp0), (name, pos, lp0)
                m1 = TO.sampling_masker(lg[None], _idx(pos), L_COND, step, 1, END, True, completion)[0]
                assert np.isfinite(m1).sum() == 1 and m1[END[1]] == 1.0, name
                val, lp1 = _draw(m1, greedy, u)
                assert val == END[1] and lp1 == 0.0 and not np.signbit(lp1), (name, val, lp1)


def test_step_zero_and_mask_invalid_off_are_not_forced():
    """Step 0 is not masked by the last position (the reference masks from step 1 on), and with mask_invalid off nothing is: the
    property fails, so the skip needs the next step index >= 1 and is not armed without mask_invalid."""
    lg = _logit_rows()["random"]
    for step, mask_invalid in ((0, True), (1, False), (7, False)):
        m0 = TO.sampling_masker(lg[None], _idx(0), L_COND, step, 0, END, mask_invalid, True)[0]
        assert np.isfinite(m0).sum() > 1
        assert int(np.argmax(m0)) != END[0]
        drawn = {TO.sample_filtered(TO.filter_sampling_logits(m0, 100, 0.4, 1.0), u) for u in np.linspace(0, 0.99, 12)}
        assert drawn - {END[0]}


def test_end_value_at_a_real_position_does_not_force_the_next_step():
    """A token (real position, end value) counts as "ended" for the early stop, but the next step's masks leave more than the end
    position: such a row is not skipped."""
    lg = _logit_rows()["random"]
    idx = _idx(0)
    idx[0, -2] = [4000, END[1]]
    m0 = TO.sampling_masker(lg[None], idx, L_COND, 3, 0, END, True, True)[0]
    assert np.isfinite(m0).sum() == V - 4001      # 4001 .. 4096
