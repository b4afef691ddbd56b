"""CPU restatement of the CTC greedy transcription semantics the device kernels implement (csrc/ctc_decode.hip), for the tests.

    best[b, t] = torch.argmax(x[b, t])                       (lowest index among equal maxima; the first NaN beats every number; an all -inf row gives 0)
    frame t is kept  iff  t < n_b  and  best[b, t] != blank  and  (t == 0 or best[b, t] != best[b, t - 1]),   n_b = lengths[b] or T
    tokens[b] = the kept ids in order, then pad_id;   n_tokens[b] = their count;   frames[b] = the kept frames' indices, then -1

Written from that statement: run starts come from a shifted comparison, the compaction is a numpy boolean index."""
import os

import numpy as np
import torch

CASES = ["all_blank_row", "blank_dominated", "blank_not_last", "exact_ties", "random", "single_token_row"]      # row order of the fixture's `meta`


def load_case(golden_dir, name):
    """a case of tests/golden/ctc_greedy.npz -> (logits (B, T, V1) fp32, blank, pad, the reference's ids (B, T) int64)"""
    d = np.load(os.path.join(golden_dir, "ctc_greedy.npz"))
    blank, pad = (int(v) for v in d["meta"][CASES.index(name)])
    return torch.from_numpy(d[name + ".q8"].astype(np.float32) / 8.0), blank, pad, d[name + ".ids"].astype(np.int64)


def argmax_frames(x: torch.Tensor) -> np.ndarray:
    """(B, T, V) float tensor (any device / float dtype) -> (B, T) int64 numpy"""
    return torch.argmax(x.detach().float().cpu(), dim=-1).numpy()


def collapse(best, blank, pad_id, lengths=None):
    """best (B, T) integer array -> (tokens (B, T) int64, n_tokens (B) int64, frames (B, T) int64)"""
    best = np.asarray(best).astype(np.int64)
    B, T = best.shape
    n = np.full((B,), T, dtype=np.int64) if lengths is None else np.clip(np.asarray(lengths).astype(np.int64), 0, T)
    t = np.arange(T)[None, :]
    run_start = np.ones((B, T), dtype=bool)
    run_start[:, 1:] = best[:, 1:] != best[:, :-1]
    keep = run_start & (best != blank) & (t < n[:, None])
    tokens = np.full((B, T), pad_id, dtype=np.int64)
    frames = np.full((B, T), -1, dtype=np.int64)
    count = keep.sum(1)
    for b in range(B):
        tokens[b, :count[b]] = best[b, keep[b]]
        frames[b, :count[b]] = np.nonzero(keep[b])[0]
    return tokens, count, frames


def greedy(x: torch.Tensor, blank, pad_id, lengths=None):
    best = argmax_frames(x)
    tokens, count, frames = collapse(best, blank, pad_id, lengths)
    return dict(best=best, tokens=tokens, n_tokens=count, frames=frames)
