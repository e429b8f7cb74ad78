"""Conditions and CPU-oracle tokens shared by tests/test_skip_ended_cpu.py and tests/test_skip_ended_gpu.py (ended rows of the
decode loop: CondTupleGPT.SKIP_ENDED).  Tiny model of tests/test_gpt_gpu.py; no GPU is touched here.

Two kinds of condition rows:
  "E" (early): the single position 4090.  From step 1 on positions ascend strictly and stay <= the next condition position, so once
      the row stands at 4090 or beyond it draws the end position 4096 within six steps.  Step 0 is unmasked (the reference masks
      from step 1 on), so WHEN a row reaches 4090 depends on its uniforms: the tests assert on the oracle's tokens that it did.
  "L" (live): 30 ascending positions 4001, 4004, ..., 4088.  A completion position never passes the next condition position and the
      end position is masked while a condition position remains, so a row whose unmasked step-0 draw lands below 4001 needs more
      than 30 steps to end: it is live for all 24.  (Spread over 0..3000 instead, a quarter of the rows drew a step-0 position beyond
      the last condition position and ended within ten steps.)  Asserted on the oracle's tokens as well.
"""
import functools

import numpy as np
import torch

STEPS = 24
END = (4096, 4096)
KW = dict(n_embd=128, n_head=2, n_layers=(2, 1), block_size=96)
LIVE_POS = [4001 + 3 * i for i in range(30)]

# the four cases: (kinds of the rows, seed)
CASES = {
    "rows96": ("E" * 48 + "EL" * 24, 11),      # two GEMM row groups of three tiles: group 0 dies completely, group 1 holds mixed tiles
    "rows50": ("ELLE" * 12 + "EL", 12),         # one group, ragged last tile
    "chains2x96": ("E" * 96 + "EL" * 48, 13),   # chain 0 all early, chain 1 mixed
    "shared16": ("E" * 16, 14),                 # sample(shared_prefix=True): one early condition, rows end at different steps
}


@functools.lru_cache(maxsize=None)
def model():
    from oracle import gpt_oracle as GO, vqdif_oracle as VO
    from shapeformer_amd import weights as W
    sd = W.make_state_dict(W.gpt_spec(n_embd=128, n_layers=(2, 1), block_size=96))
    return sd, VO.to_torch_sd(sd), GO.GPTCfg(**KW)


def conditions(kinds):
    """-> c (B, 31, 2) int64 padded with end pairs, Lc (B,) int32 (the end pair included)."""
    B = len(kinds)
    c = np.full((B, len(LIVE_POS) + 1, 2), END[0], np.int64)
    Lc = np.zeros(B, np.int32)
    for b, k in enumerate(kinds):
        pos = [4090] if k == "E" else LIVE_POS
        c[b, :len(pos), 0] = pos
        c[b, :len(pos), 1] = [(7 * p) % 4096 for p in pos]      # rows of a kind are identical (the shared-prefix case needs that)
        Lc[b] = len(pos) + 1
    return c, Lc


@functools.lru_cache(maxsize=None)
def oracle_tokens(case):
    """(B, STEPS, 2) tokens of oracle.gpt_oracle.sample_indices for every row of the case, on the uniforms of the case's seed; rows of
    one kind (one condition length) go through the oracle as one batch - the greedy row is global row 0, as in the device sampler."""
    from oracle import gpt_oracle as GO
    kinds, seed = CASES[case]
    B = len(kinds)
    _, sd_t, cfg = model()
    c, Lc = conditions(kinds)
    u = GO.uniforms(seed, STEPS, B)
    out = np.zeros((B, STEPS, 2), np.int64)
    for k in "EL":
        rows = [b for b in range(B) if kinds[b] == k]
        if not rows:
            continue
        cb = torch.from_numpy(c[rows][:, :Lc[rows[0]]])
        tok, _, _ = GO.sample_indices(sd_t, cfg, cb, STEPS, u[:, :, rows], use_cache=True, stop_early=False,
                                      best_in_first=(rows[0] == 0), return_logits=False)
        out[rows] = tok
    return out


def first_end_step(tok):
    """(B,) first step whose position is the end position (STEPS where there is none)."""
    hit = tok[:, :, 0] == END[0]
    return np.where(hit.any(1), hit.argmax(1), STEPS)
