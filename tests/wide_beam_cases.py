"""Cases of the wide beam-step tests (tests/test_gpu_wide_beam.py, tests/test_wide_beam_cpu.py): seeded per-step scores, the kernel's arithmetic restated on the host
(one rounding per operation) and the pinned CPU loop `oracle/generate_ref.beam_search` run over them.  Everything here is CPU work and cached per case: the CPU test
asserts what the cases must exercise (`few`, `tied`, hypotheses closed by the end-of-sequence token before max_length, re-ordering past the old LDS limit) from the
oracle's trace alone, the GPU test feeds the same inputs to the kernel and compares."""
import functools
import itertools

import numpy as np
import torch

from oracle import generate_ref as G

EOS, START, W_CTC, W_LM = 1, 2, 0.3, 0.5
SHAPES = [(2, 17, 51), (1, 64, 51), (2, 33, 500), (2, 60, 5001)]       # (B, W, V): first width past 16 with 2W < V; 2W > V; in between; the recipe's, W * V > 32 Ki
FOLLOW = [(B, W, V, ctc, lm, lp, es) for (B, W, V), ctc, lm, lp, es in itertools.product(SHAPES, (True, False), (False, True), (1.0, 0.6), (False, True, "never"))]
TIES = [(2, 17, 51, True, False), (1, 64, 51, True, True), (2, 33, 500, True, False), (2, 60, 5001, True, False), (2, 60, 5001, False, True)]
MINUS_INF = [(2, 33, 500, True, False), (2, 33, 500, False, True)]
LONG = dict(B=2, W=60, V=51, max_length=140, late=125)                 # W * (cur_len + Lmax) * 8 > 96 KiB from cur_len = 64 on
OLD_LDS = 96 * 1024


def step_inputs(gen, t, n, V, with_ctc, with_lm, ties, eos_logit):
    """random (logits, CTC scores | None, LM logits | None) (n, V) of step t, the end-of-sequence logit lifted by `eos_logit`.  `ties`: every stream on a coarse grid,
    so that groups of candidates share a value and their index order decides"""
    lg = torch.randn(n, V, generator=gen) * 2.0
    ctc = (torch.randn(n, V, generator=gen) * 3.0 - 5.0) if with_ctc else None
    lm = (torch.randn(n, V, generator=gen) * 2.0) if with_lm else None
    if ties:
        lg = (lg * 4).round().clamp(max=12) / 4
        ctc = (ctc / 3).round().clamp(-1, 1) - 5 if with_ctc else None
        lm = lm.round().clamp(max=1) if with_lm else None
    lg[:, EOS] += eos_logit                                           # (a multiple of the grid: lifted above the cap, still tied with its like)
    return lg, ctc, lm


def processed_scores(lg, lse, ctc, lm, lm_lse, pad):
    """the kernel's arithmetic on the host: s = logit - lse; [CTC: pad -> logzero, s = (1 - w) s + w ctc]; [LM: l = lm - lm_lse; m = w_lm l; s = s + m]"""
    sc = (lg - lse[:, None]).numpy()
    if ctc is not None:
        sc[:, pad] = np.float32(-10000000000.0)
        sc = np.float32(1 - W_CTC) * sc + np.float32(W_CTC) * ctc.numpy()
    if lm is not None:
        l = (lm - lm_lse[:, None]).numpy()
        m = np.float32(W_LM) * l
        sc = sc + m
    return sc.astype(np.float32)


@functools.lru_cache(maxsize=4)
def build(B, W, V, with_ctc, with_lm, lp, es, kind="", max_length=11, late=0):
    """-> dict(steps = per step (logits, lse, ctc, lm, lm_lse) CPU tensors, oracle = (sequences, scores), trace, calls = steps the oracle ran, few, tied, eos_closed).
    `kind`: "" | "ties" | "minus_inf" (at steps 1 and 2 utterance (t - 1) % B gets -inf everywhere but W finite candidates of one beam, none of them EOS or pad).
    `late` > 0: the end-of-sequence logit is held at -5 before step `late` and lifted by 3 from there on; otherwise -5 at the first step and lifted afterwards."""
    seed = B * 100000 + W * 1000 + V + 7 * (kind == "ties") + 13 * (kind == "minus_inf") + 17 * with_ctc + 19 * with_lm + (29 if lp != 1.0 else 0) + 31 * [False, True, "never"].index(es)
    gen = torch.Generator().manual_seed(seed)
    pad, n = V - 1, B * W
    boost = 5.0 if V > 1000 else 3.0
    steps, processed = [], []
    for t in range(max_length - 1):
        eos_logit = (3.0 if t >= late else -5.0) if late else (boost if t >= 1 else -5.0)
        lg, ctc, lm = step_inputs(gen, t, n, V, with_ctc, with_lm, kind == "ties", eos_logit)
        if kind == "minus_inf" and t in (1, 2):
            b = (t - 1) % B
            keep = torch.zeros(W, V, dtype=torch.bool)
            keep[t % W, 3 + 7 * torch.arange(W)] = True
            lg[b * W:(b + 1) * W][~keep] = -float("inf")
            if ctc is not None:
                ctc[b * W:(b + 1) * W][~keep] = -float("inf")
        lse = torch.logsumexp(lg, 1).float()
        lm_lse = torch.logsumexp(lm, 1).float() if lm is not None else None
        steps.append((lg, lse, ctc, lm, lm_lse))
        processed.append(processed_scores(lg, lse, ctc, lm, lm_lse, pad))
    calls = []

    def score_fn(rows):
        calls.append(rows.shape[1])
        return processed[len(calls) - 1]
    tr = {}
    seq, scores = G.beam_search(score_fn, B, W, V, max_length=max_length, eos=EOS, pad=pad, start=START, length_penalty=lp, early_stopping=es, trace=tr)
    few = tied = 0
    for t in range(len(calls)):
        ov, _ = tr["cands"][t]
        for b in np.nonzero(tr["open"][t])[0]:
            few += int(np.isfinite(tr["acc"][t][b]).sum() < 2 * W)
            tied += int((ov[b][:-1] == ov[b][1:]).any())
    # hypotheses closed by the end-of-sequence token before max_length (the token ends a hypothesis wherever it appears)
    eos_closed = int((seq[:, :max_length - 1] == EOS).any(1).sum())
    # steps whose running beams are not the previous ones in place (beams re-order)
    reorder = [bool((tr["running"][t + 1][:, :, :-1] != tr["running"][t]).any()) for t in range(len(calls) - 1)]
    tr.pop("acc", None)                                                # (the largest item: W * V floats per utterance and step)
    return dict(steps=steps, oracle=(seq, scores), trace=tr, calls=len(calls), few=few, tied=tied, eos_closed=eos_closed, reorder=reorder, pad=pad, max_length=max_length)
