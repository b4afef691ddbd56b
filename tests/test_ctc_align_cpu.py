"""CPU: the host restatements of CTC forced alignment (tests/ctc_align_ref.py) held to each other — the float64 recursion against the enumeration of every
alignment, the bit-exact float32 restatement against the float64 recursion within the rounding bound — the tie rules and fills on constructed inputs, and the
host-side refusals of ops.ctc_align, EBranchformerEngine.align, Wav2Vec2EBranchformerForCTC.align and the C entry (no device is touched)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_align_ref as R  # noqa: E402

DRAWS = 20


def draw_logits(T, V1, seed, scale=3.0):
    return (np.random.default_rng(seed).standard_normal((T, V1)) * scale).astype(np.float32)


draw_labels = R.draw_labels


def lp32_of(x):
    """(lse float32, lp (T, V1) = the float32 values x - lse the kernel forms)"""
    lse = R.row_lse32(x)
    return lse, (x - lse[:, None]).astype(np.float32)


# ---------------------------------------------------------------- 1. float64 recursion == enumeration
TINY = [(1, 2, []), (1, 2, [0]), (3, 3, [0]), (4, 3, [0, 1]), (5, 3, [1, 1]), (5, 4, [0, 2]), (6, 4, [2, 2, 1]), (6, 4, [0, 1, 2]), (6, 3, []), (6, 4, [1, 1, 1]), (4, 4, [1, 1, 1])]


@pytest.mark.parametrize("T,V1,labels", TINY)
def test_float64_recursion_equals_the_enumeration(T, V1, labels):
    positive = 0
    for seed in range(DRAWS):
        lp = R.log_softmax(draw_logits(T, V1, seed))
        want, paths = R.brute_force(lp, labels, V1 - 1)
        got = R.viterbi64(lp, labels, V1 - 1)
        if not paths:
            assert got["score"] == R.NEG and got["path"] is None
            continue
        assert abs(got["score"] - want) <= 1e-12 * max(1.0, abs(want))
        assert got["path"] in paths
        if got["margin"] > 1e-9:
            positive += 1
            assert paths == [got["path"]]
        if len(paths) > 1:
            assert got["margin"] <= 1e-9
    if T >= len(labels) + sum(a == b for a, b in zip(labels, labels[1:])):
        assert positive >= DRAWS - 2, positive                             # continuous draws: ties are the exception


def test_margin_is_the_gap_to_the_second_best_alignment():
    """on a tiny case the margin equals best - (best score among alignments that leave the best path's cells), enumerated"""
    T, V1, labels = 5, 3, [0, 1]
    for seed in range(5):
        lp = R.log_softmax(draw_logits(T, V1, seed))
        got = R.viterbi64(lp, labels, V1 - 1)
        others = [R.path_score(lp, p) for p in itertools.product(range(V1), repeat=T) if R.collapse(p, V1 - 1) == labels and list(p) != got["path"]]
        # different state sequences can share a class sequence only through the blank/label identity, which the state graph of a fixed target excludes
        assert abs(got["margin"] - (got["score"] - max(others))) <= 1e-12


# ---------------------------------------------------------------- 2. float32 restatement against the float64 recursion
SHAPES = [(12, 3, 7, False), (12, 5, 7, True), (7, 3, 7, True), (40, 9, 30, False)]
SCORE_ONLY = [(130, 70, 30, True), (300, 140, 500, False)]


def _compare(T, n, V1, repeats, seed):
    x = draw_logits(T, V1, seed)
    labels = draw_labels(n, V1, seed, repeats)
    lse, lp = lp32_of(x)
    r64 = R.viterbi64(lp, labels, V1 - 1)                                  # the same float32 log-probabilities, widened: only the recursion's adds differ
    r32 = R.viterbi32(x, lse, np.asarray(labels, dtype=np.int64), T, V1 - 1)
    assert r64["path"] is not None and r32["score"] > R.NEG
    path = r32["path"].tolist()
    assert len(path) == T and min(path) >= 0 and R.collapse(path, V1 - 1) == labels
    # one rounded add per frame: each partial sum is within 2^-24 |delta| of exact, for the chosen and for the optimal path
    bound = R.rounding_bound(T, r64["max_delta"])
    rescored = R.path_score(lp.astype(np.float64), path)
    assert r64["score"] - rescored <= bound and rescored <= r64["score"] + 1e-12
    assert abs(float(r32["score"]) - r64["score"]) <= bound
    return r64, r32, bound


@pytest.mark.parametrize("T,n,V1,repeats", SHAPES)
def test_float32_restatement_follows_the_float64_recursion(T, n, V1, repeats):
    under = 0
    for seed in range(DRAWS):
        r64, r32, bound = _compare(T, n, V1, repeats, seed)
        if r64["margin"] > bound:
            assert r32["path"].tolist() == r64["path"], seed
            for u in range(n):                                             # the spans are the frames of the token's state
                fr = [t for t, s in enumerate(r64["states"]) if s == 2 * u + 1]
                assert (int(r32["start"][u]), int(r32["end"][u])) == (fr[0], fr[-1] + 1)
        else:
            under += 1
    assert under <= 1, under                                               # the condition on the draws: at most 1 in 20 under the bound


@pytest.mark.parametrize("T,n,V1,repeats", SCORE_ONLY)
def test_float32_restatement_scores_and_validity_on_longer_targets(T, n, V1, repeats):
    for seed in range(4):
        _compare(T, n, V1, repeats, seed)


# ---------------------------------------------------------------- 3. tie rules, fills, infeasible inputs
def _v32(x, labels, in_len=None, blank=None, U=None):
    x = np.asarray(x, dtype=np.float32)
    blank = x.shape[1] - 1 if blank is None else blank
    row = np.full(len(labels) if U is None else U, -100, dtype=np.int64)
    row[:len(labels)] = labels
    return R.viterbi32(x, R.row_lse32(x), row, x.shape[0] if in_len is None else in_len, blank)


def test_all_equal_logits_tokens_come_as_early_as_they_can():
    r = _v32(np.zeros((5, 4)), [1, 2])
    assert r["path"].tolist() == [1, 2, 3, 3, 3]                           # stay beats s-1 beats s-2; the end prefers the trailing blank
    assert r["start"].tolist() == [0, 1] and r["end"].tolist() == [1, 2]
    lp = np.float32(0.0) - R.row_lse32(np.zeros((1, 4)))[0]
    assert r["score"] == np.float32(5) * lp and (r["token_lp"] == lp).all()
    r = _v32(np.zeros((6, 3)), [0, 0])                                     # a repeat needs its blank
    assert r["path"].tolist() == [0, 2, 0, 2, 2, 2]


def test_two_equal_predecessors_stay_wins():
    x = np.zeros((2, 3), dtype=np.float32)
    x[1] = [0.0, 2.0, 0.0]                                                 # frame 0: blank and label tie; frame 1: the label wins the end
    r = _v32(x, [1])
    assert r["path"].tolist() == [1, 1] and (r["start"][0], r["end"][0]) == (0, 2)


def test_equal_end_states_end_in_the_blank():
    x = np.zeros((2, 3), dtype=np.float32)
    x[0] = [0.0, 1.0, 0.0]
    r = _v32(x, [1])
    assert r["path"].tolist() == [1, 2] and (r["start"][0], r["end"][0]) == (0, 1)


def test_infeasible_inputs_and_empty_targets():
    x = draw_logits(4, 5, 3)
    empty = _v32(x, [], U=3)
    assert empty["path"].tolist() == [4, 4, 4, 4] and empty["tgt_len"] == 0 and (empty["start"] == -1).all() and (empty["token_lp"] == 0).all()
    assert abs(float(empty["score"]) - R.path_score(R.log_softmax(x), [4] * 4)) < 1e-5
    for labels, in_len in (([0, 1, 2, 3, 0], 4), ([1, 1, 2], 3), ([1], 0), ([7], 4), ([4], 4), ([1, 5], 4)):      # too long, repeat without room, no frames, label >= V1, blank as a label
        r = _v32(x, labels, in_len=in_len, U=6)
        assert r["score"] == np.float32(R.NEG) and (r["path"] == -1).all() and (r["start"] == -1).all() and (r["end"] == -1).all() and (r["token_lp"] == 0).all()
        assert r["tgt_len"] == len(labels)
    tight = _v32(x, [1, 1, 2], in_len=4, U=6)                              # exactly n + repeats frames
    assert tight["path"].tolist() == [1, 4, 1, 2]
    none = _v32(x, [], in_len=0)
    assert none["score"] == 0 and (none["path"] == -1).all()
    part = _v32(x, [2], in_len=2, U=2)                                     # frames past in_len hold -1, entries past the target -1 / 0
    assert (part["path"][2:] == -1).all() and (part["path"][:2] >= 0).all() and part["start"][1] == -1 and part["token_lp"][1] == 0
    mid = R.viterbi32(x, R.row_lse32(x), np.array([-100, 2, -1, 3, -100], dtype=np.int64), 4, 4)      # padding in the middle of the row
    assert mid["tgt_len"] == 2 and R.collapse(mid["path"], 4) == [2, 3] and mid["start"][2] == -1
    col = x.copy()
    col[:, 1] = R.NEG                                                      # a -inf column under a label the target needs
    assert _v32(col, [1])["score"] == np.float32(R.NEG)


# ---------------------------------------------------------------- 4. host-side refusals
def test_ops_ctc_align_refuses_on_the_host():
    from huggingface_asr_amd import ops
    x, lab = torch.zeros(2, 6, 5), torch.zeros(2, 3, dtype=torch.int64)
    for bad_x in (x.double(), x[0], x.to(torch.int32), x.transpose(1, 2), torch.zeros(2, 6, 1), "x"):
        with pytest.raises(ValueError):
            ops.ctc_align(bad_x, lab)
    for bad_lab in (lab.to(torch.int32), lab[0], torch.zeros(3, 3, dtype=torch.int64), lab.float()):
        with pytest.raises(ValueError):
            ops.ctc_align(x, bad_lab)
    for bad_len in (torch.zeros(2, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32), [6, 6]):
        with pytest.raises(ValueError):
            ops.ctc_align(x, lab, bad_len)
    for blank in (5, -1):
        with pytest.raises(ValueError):
            ops.ctc_align(x, lab, blank=blank)
    with pytest.raises(ValueError):
        ops.ctc_align(x, lab, lse=torch.zeros(11))
    with pytest.raises(RuntimeError, match="device tensors"):              # well-formed, but on the CPU
        ops.ctc_align(x, lab, torch.full((2,), 6, dtype=torch.int32))


def test_engine_and_model_align_refuse_on_the_host():
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.engine import EBranchformerEngine
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    feats, lab = torch.zeros(1, 100, 80), torch.zeros(1, 3, dtype=torch.int64)
    eng = EBranchformerEngine(dict(shapes.TINY), "cpu")
    with pytest.raises(ValueError, match="span"):
        eng.align(feats, None, lab, span="inner")
    with pytest.raises(ValueError, match="labels"):
        eng.align(feats, None, lab.to(torch.int32))
    with pytest.raises(RuntimeError):                                      # no weights, a CPU tensor: as forward()
        eng.align(feats, None, lab)
    base = dict(shapes.TINY); base.pop("num_fbanks")
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**base))
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.align(feats, labels=lab)
    model.eval()
    with pytest.raises(RuntimeError, match="GPU"):
        model.align(feats, labels=lab)
    with pytest.raises(ValueError, match="span"):
        model.align(feats, labels=lab, span="inner")
    assert "conv_stride" in Wav2Vec2EBranchformerForCTC.align.__doc__


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """MI_ERR_ARG / MI_ERR_UNSUPPORTED come back from argument checks alone: no device is needed (and none is here)"""
    R.check_c_entry_refusals()
