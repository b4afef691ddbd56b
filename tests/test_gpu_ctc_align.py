"""GPU: CTC forced alignment on the device (csrc/ctc_align.hip; ops.ctc_align, EBranchformerEngine.align, Wav2Vec2EBranchformerForCTC.align) against the bit-exact
float32 restatement of its semantics (tests/ctc_align_ref.py `viterbi32`; tests/test_ctc_align_cpu.py holds that to the float64 recursion and the enumeration).

Every comparison is for equality: path, tgt_len, start, end as integers, score and token_lp bit for bit; no draw is excluded.  The row log-sum-exp fed to both
sides is the device's own (ops.row_lse).  Output buffers and the workspace are filled with garbage before every raw call, and everything past the lengths is
checked for the documented fill."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_align_ref as R  # noqa: E402

draw_labels = R.draw_labels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def logits_of(B, T, V1, seed, scale=3.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal((B, T, V1)) * scale).astype(np.float32))


def label_rows(rows, U=None, pad=-100):
    U = max(len(r) for r in rows) if U is None else U
    out = np.full((len(rows), U), pad, dtype=np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out


def device_lse(xd):
    from huggingface_asr_amd import ops
    B, T, V1 = xd.shape
    return torch.stack([ops.row_lse(xd[b]) for b in range(B)])             # (B, T): any strides


def align_raw(xd, lse, labels, in_len, blank):
    """mi_ctc_align itself over garbage-filled outputs and workspace -> numpy dict (spans (B, U))"""
    from huggingface_asr_amd import _lib
    L = _lib.lib()
    B, T, V1 = xd.shape
    U = labels.shape[1]
    lab = torch.from_numpy(labels).to(DEV)
    lens = torch.as_tensor([T] * B if in_len is None else in_len, dtype=torch.int32).to(DEV)
    nbytes = int(L.mi_ctc_align_workspace_bytes(B, T, U))
    ws = torch.full((max(nbytes, 16),), 0x7f, dtype=torch.uint8, device=DEV)
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)
    f32 = lambda *s: torch.full(s, 0x7f, dtype=torch.uint8, device=DEV).repeat_interleave(4, -1).view(torch.float32)
    path, tl, start, end = i32(B, T), i32(B), i32(B, max(U, 1)), i32(B, max(U, 1))
    score, tlp = f32(B), f32(B, max(U, 1))
    assert lse.is_contiguous() and lse.shape == (B, T)
    rc = L.mi_ctc_align(xd.data_ptr(), xd.stride(0), xd.stride(1), 0 if xd.dtype == torch.float32 else 1, lse.data_ptr(), T, lab.data_ptr() if U else None, U,
                        lens.data_ptr(), blank, V1, B, ws.data_ptr() if nbytes else None, nbytes, path.data_ptr(), score.data_ptr(), tl.data_ptr(),
                        start.data_ptr() if U else None, end.data_ptr() if U else None, tlp.data_ptr() if U else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dict(path=path.cpu().numpy(), score=score.cpu().numpy(), tgt_len=tl.cpu().numpy(), start=start.cpu().numpy()[:, :U], end=end.cpu().numpy()[:, :U],
                token_lp=tlp.cpu().numpy()[:, :U])


def same(got, want, where=""):
    for k in ("path", "tgt_len", "start", "end"):
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (where, k, got[k], want[k])
    for k in ("score", "token_lp"):
        g, w = np.ascontiguousarray(got[k], dtype=np.float32), np.ascontiguousarray(want[k], dtype=np.float32)
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (where, k, g, w)


def check(x, labels, in_len=None, blank=None, view=None, where=""):
    """x (B, T, V1) host tensor (fp32 / bf16), labels (B, U) int64 numpy; view: maps the device tensor to the (strided) one the kernel reads"""
    B, T, V1 = x.shape
    blank = V1 - 1 if blank is None else blank
    xd = x.to(DEV) if view is None else view(x)
    assert torch.equal(xd.cpu(), x)
    lse = device_lse(xd)
    got = align_raw(xd, lse, labels, in_len, blank)
    want = R.viterbi32_batch(x.float().numpy(), lse.cpu().numpy(), labels, in_len, blank)
    same(got, want, where)
    nb = [T] * B if in_len is None else [min(max(int(v), 0), T) for v in in_len]
    for b in range(B):                                                     # the documented fills, stated here once more
        n = int(got["tgt_len"][b])
        assert n == len(R.target(labels[b]))
        assert (got["path"][b, nb[b]:] == -1).all() and (got["start"][b, n:] == -1).all() and (got["end"][b, n:] == -1).all() and (got["token_lp"][b, n:] == 0).all()
        if got["score"][b] == -np.inf:
            assert (got["path"][b] == -1).all() and (got["start"][b] == -1).all() and (got["end"][b] == -1).all() and (got["token_lp"][b] == 0).all()
        else:
            assert R.collapse(got["path"][b, :nb[b]], blank) == R.target(labels[b])
    return got, want


def strided(x, pad_t=3, pad_b=5):
    """rows ld_t = V1 + pad_t apart, utterances more than T * ld_t apart; the padding holds values that would win every comparison"""
    B, T, V1 = x.shape
    ld_t = V1 + pad_t
    buf = torch.full((B, T * ld_t + pad_b), 1e30, dtype=x.dtype, device=DEV)
    v = buf.as_strided((B, T, V1), (T * ld_t + pad_b, ld_t, 1), 1)
    v.copy_(x.to(DEV))
    return v


# ------------------------------------------------------------------------------------------------ 1. small shapes and edges
def test_one_frame():
    x = logits_of(2, 1, 5, 1)
    check(x, np.zeros((2, 0), dtype=np.int64), where="U = 0")
    got, _ = check(x, np.full((2, 2), -100, dtype=np.int64), in_len=[0, 1], where="n = 0, with and without a frame")
    assert got["score"][0] == 0 and got["path"].tolist() == [[-1], [4]]
    got, _ = check(x, label_rows([[2], [3]]), where="U = 1")
    assert got["path"].tolist() == [[2], [3]] and got["start"].tolist() == [[0], [0]] and got["end"].tolist() == [[1], [1]]


def test_exactly_as_many_frames_as_labels_and_tight_repeats():
    lab = draw_labels(9, 7, 3)
    got, _ = check(logits_of(1, 9, 7, 2), label_rows([lab]), where="T = n")
    assert got["path"][0].tolist() == lab
    rep = [1, 1, 2, 2, 2, 5]                                               # 6 labels, 3 repeats: 9 frames at least
    got, _ = check(logits_of(3, 10, 7, 3), label_rows([rep] * 3), in_len=[10, 9, 8], where="tight repeats")
    assert np.isfinite(got["score"][:2]).all() and got["score"][2] == -np.inf
    assert got["path"][1, :9].tolist() == [1, 6, 1, 2, 6, 2, 6, 2, 5]
    got, _ = check(logits_of(3, 10, 4, 4), label_rows([[2, 2, 2, 2]] * 3), in_len=[10, 7, 6], where="all repeats")
    assert got["score"][2] == -np.inf and got["path"][1, :7].tolist() == [2, 3, 2, 3, 2, 3, 2]


def test_two_classes():
    check(logits_of(2, 9, 2, 5), label_rows([[0, 0, 0], [0]]), where="V1 = 2")
    check(logits_of(2, 9, 2, 5), label_rows([[1, 1], [1]]), blank=0, where="V1 = 2, blank first")


@pytest.mark.parametrize("n", [7, 8, 15, 16])
def test_backpointer_word_edges(n):
    check(logits_of(2, 41, 12, 10 + n), label_rows([draw_labels(n, 12, n), draw_labels(n, 12, n + 50, repeats=True)]), in_len=[41, 33], where=f"S = {2 * n + 1}")


@pytest.mark.parametrize("n", [62, 63, 64, 65, 255, 256, 257, 511, 512, 767, 768])
def test_around_the_boundaries_between_kernel_forms(n):
    """U = n selects the form: one wave up to 63 labels, the block form beyond, with 1 .. 4 pairs of states per thread (n + 1 pairs, 256 per step)"""
    T = n + n // 3 + 40
    check(logits_of(1, T, 30, 20 + n), label_rows([draw_labels(n, 30, n, repeats=True)]), where=f"n = {n}")


def test_widest_block_form():
    check(logits_of(1, 1100, 20, 31), label_rows([draw_labels(n, 20, n) for n in (1023,)]), where="n = 1023")
    check(logits_of(2, 540, 20, 32), label_rows([draw_labels(513, 20, 1), draw_labels(511, 20, 2)]), in_len=[540, 530], where="n = 513, 511 in one batch")


def _switch(U):
    """the largest T whose backpointers stay in LDS for label rows of width U"""
    from huggingface_asr_amd import _lib
    L = _lib.lib()
    lo, hi = 1, 1 << 16
    assert L.mi_ctc_align_workspace_bytes(1, lo, U) == 0 and L.mi_ctc_align_workspace_bytes(1, hi, U) > 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if L.mi_ctc_align_workspace_bytes(1, mid, U) == 0 else (lo, mid)
    return lo


@pytest.mark.parametrize("U", [63, 64])
def test_around_the_switch_from_lds_to_workspace(U):
    T = _switch(U)
    assert T % 8 == 0 and T >= 1000
    x = logits_of(1, T + 1, 24, 40 + U)
    lab = label_rows([draw_labels(U - 3, 24, U, repeats=True)], U=U)
    for t in (T - 1, T, T + 1):                                            # LDS, LDS at its last size, workspace
        check(x[:, :t].contiguous(), lab, where=f"U = {U}, T = {t}")


def test_batch_of_mixed_rows():
    T, V1 = 30, 11
    x = logits_of(5, T, V1, 50)
    rows = [draw_labels(6, V1, 1), [], draw_labels(9, V1, 2), [3, 11, 4], draw_labels(12, V1, 3, repeats=True)]
    lab = label_rows(rows, U=14)
    in_len = [T, 17, 0, T, 12]                                             # row 2: no frames; row 3: a label >= V1; row 4: 12 labels with repeats in 12 frames
    got, want = check(x, lab, in_len, where="mixed batch")
    assert np.isfinite(got["score"][[0, 1]]).all() and (got["score"][[2, 3, 4]] == -np.inf).all()
    assert (got["path"][1, :17] == V1 - 1).all()
    for b in range(5):                                                     # each row alone: the rows around it change nothing
        one = align_raw(x[b:b + 1].to(DEV), device_lse(x[b:b + 1].to(DEV)), lab[b:b + 1], in_len[b:b + 1], V1 - 1)
        same(one, {k: v[b:b + 1] for k, v in got.items()}, f"row {b} alone")
    blank_label = label_rows([[3, V1 - 1, 4]], U=4)                        # the blank as a label
    assert check(x[:1], blank_label)[0]["score"][0] == -np.inf
    check(x[:2], lab[:2], [T + 5, -3], where="in_len is clamped to [0, T]")


@pytest.mark.parametrize("U", [70, 300])
def test_wide_label_rows_with_short_empty_and_infeasible_targets(U):
    """the block form is chosen from the row's width alone: targets far shorter than U, n = 0, no frames and infeasible rows under it"""
    T, V1 = 90, 13
    x = logits_of(7, T, V1, 55 + U)
    rows = [draw_labels(5, V1, 1), [], draw_labels(63, V1, 2), draw_labels(64, V1, 3), draw_labels(9, V1, 4), [3, 13, 4], draw_labels(70, V1, 5, repeats=True)]
    lab = label_rows(rows, U=U)
    lab[0] = np.roll(lab[0], U - 20)                                       # the five labels of row 0 sit behind 40+ entries of padding
    in_len = [T, 31, T, T, 0, T, T]                                        # row 4: no frames; row 5: a label >= V1; row 6: 70 labels with repeats need 93 frames
    got, _ = check(x, lab, in_len, where=f"wide rows, U = {U}")
    assert np.isfinite(got["score"][:4]).all() and (got["score"][4:] == -np.inf).all() and got["tgt_len"].tolist() == [5, 0, 63, 64, 9, 3, 70]
    none = np.full((2, U), -100, dtype=np.int64)
    got, _ = check(x[:2], none, [0, T], where="wide rows, no labels at all")
    assert got["score"][0] == 0 and (got["path"][1] == V1 - 1).all()


def test_padding_in_the_middle_of_the_row():
    x = logits_of(2, 25, 9, 60)
    lab = np.array([[-100, 3, -1, -1, 5, 5, -100, 0], [2, -100, -100, -100, -100, -100, -100, 2]], dtype=np.int64)
    got, _ = check(x, lab, where="padding inside")
    assert got["tgt_len"].tolist() == [4, 2]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [9, 80])
def test_strided_logits_both_dtypes_and_inf_columns(n, dtype):
    T, V1 = n + 31, 17
    x = logits_of(3, T, V1, 70 + n).to(dtype)
    lab = label_rows([draw_labels(n, V1, 5), draw_labels(n - 2, V1, 6, repeats=True), draw_labels(n, V1, 7)])
    check(x, lab, [T, T - 4, T], view=strided, where="strided")
    check(x, lab, [T, T - 4, T], where="contiguous")
    xi = x.clone()
    xi[0, :, int(lab[0, 1])] = float("-inf")                               # a column the target needs: no alignment exists
    xi[1, 3, :5] = float("-inf")                                           # ... scattered
    xi[2, ::2, int(lab[2, 0])] = float("-inf")                             # ... on every other frame only
    got, _ = check(xi, lab, [T, T - 4, T], view=strided, where="-inf columns")
    assert got["score"][0] == -np.inf and np.isfinite(got["score"][2])


def test_long_utterance_takes_the_workspace_path_and_two_runs_agree():
    from huggingface_asr_amd import _lib, ops
    T, n, V1 = 1500, 400, 40
    assert _lib.lib().mi_ctc_align_workspace_bytes(2, T, n) > 0
    x = logits_of(2, T, V1, 80)
    lab = label_rows([draw_labels(n, V1, 8, repeats=True), draw_labels(n - 57, V1, 9)])
    got, _ = check(x, lab, [T, T - 123], where="long")
    xd, labd, lens = x.to(DEV), torch.from_numpy(lab).to(DEV), torch.tensor([T, T - 123], dtype=torch.int32, device=DEV)
    a, b = ops.ctc_align(xd, labd, lens), ops.ctc_align(xd, labd, lens)
    for k in ("path", "score", "tgt_len", "start", "end", "token_lp"):
        assert torch.equal(a[k], b[k]), k                                  # two runs: the same bits
    same({k: v.cpu().numpy() for k, v in a.items()}, got, "ops.ctc_align against the raw call")
    short = ops.ctc_align(xd, labd, lens, return_spans=False)
    assert set(short) == {"path", "score", "tgt_len"} and torch.equal(short["path"], a["path"]) and torch.equal(short["score"], a["score"])
    noblank = ops.ctc_align(xd, labd, lens, blank=V1 - 1, lse=ops.row_lse(xd.reshape(-1, V1)))
    assert torch.equal(noblank["score"], a["score"]) and torch.equal(noblank["token_lp"], a["token_lp"])


def test_c_entry_refusals_launch_nothing():
    R.check_c_entry_refusals()                                             # the argument checks of tests/test_ctc_align_cpu.py, here beside a live device
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. against the greedy decoder
def test_aligning_the_greedy_transcript_gives_back_the_greedy_path():
    from huggingface_asr_amd import ops
    B, T, V1 = 4, 60, 33
    x = logits_of(B, T, V1, 90, scale=1.0)
    xd = x.to(DEV)
    g = ops.ctc_greedy_decode(xd, V1 - 1, -1, return_frames=True)
    out = ops.ctc_align(xd, g["tokens"])
    assert torch.equal(out["path"], g["best"]) and torch.equal(out["tgt_len"], g["n_tokens"])
    assert torch.equal(out["start"], g["frames"])
    lp = R.log_softmax(x.numpy())
    best = g["best"].cpu().numpy()
    for b in range(B):
        exact = R.path_score(lp[b], best[b])
        n = int(out["tgt_len"][b])
        r64 = R.viterbi64(lp[b], g["tokens"][b, :n].tolist(), V1 - 1)
        assert r64["path"] == best[b].tolist() and abs(r64["score"] - exact) <= 1e-9      # the greedy path IS the best alignment of its own collapse
        bound = R.rounding_bound(T, r64["max_delta"])
        print(f"utterance {b}: device {float(out['score'][b]):.6f} float64 {exact:.6f} bound {bound:.2e}")
        assert abs(float(out["score"][b]) - exact) <= bound
        assert abs(float(out["token_lp"][b, :n].double().sum()) - sum(lp[b, t, best[b, t]] for t in range(T) if best[b, t] != V1 - 1)) <= bound


# ------------------------------------------------------------------------------------------------ 3. engine and model
def _tiny():
    from helpers import case_inputs, load_golden
    from huggingface_asr_amd import shapes
    cfg = dict(shapes.TINY)
    cfg.update(ctc_zero_infinity=True, ctc_loss_reduction="mean")
    sd, x, am, lab = case_inputs(load_golden("tiny_rel"), cfg)
    return cfg, sd, x.to(DEV), am.to(DEV), lab.to(DEV)


KEYS = ("path", "score", "tgt_len", "start", "end", "token_lp")


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("span", ["valid", "all"])
def test_engine_align_equals_the_op_on_the_forward_logits(precision, span):
    from huggingface_asr_amd import ops
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg, sd, x, am, lab = _tiny()
    eng = EBranchformerEngine(cfg, DEV, precision=precision)
    eng.load_state_dict(sd)
    lens = am.sum(-1).to(torch.int32)
    assert int(lens[0]) != int(lens[1])
    fwd = eng.forward(x, lens)
    want = ops.ctc_align(fwd["logits"], lab, fwd["outer_len"] if span == "valid" else None)
    got = eng.align(x, lens, lab, span=span)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["outer_len"], fwd["outer_len"]) and torch.equal(got["inner_len"], fwd["inner_len"])
    assert torch.isfinite(got["score"]).all() and torch.equal(got["tgt_len"], (lab >= 0).sum(-1).to(torch.int32))


def test_engine_align_with_the_head_epilogue_lse():
    """head_lse on, a head the fused GEMM + log-sum-exp kernel takes (hidden size 128): align feeds the epilogue's lse, whose bits may differ from ops.row_lse's,
    so the comparison that holds bit for bit is the op given that same lse; against the row_lse route the path agrees and the scores differ by rounding only"""
    from huggingface_asr_amd import ops, shapes, synth
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg = dict(shapes.TINY, hidden_size=128, intermediate_size=256, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 11).items()}
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(sd)
    x = torch.from_numpy(synth.normal(3, "feats", (2, 200, 80), 1.0)).to(DEV)
    lens = torch.tensor([200, 163], dtype=torch.int32, device=DEV)
    lab = torch.from_numpy(label_rows([draw_labels(7, 51, 1), draw_labels(4, 51, 2)])).to(DEV)
    plain = eng.align(x, lens, lab)
    eng.head_lse = True
    fwd = eng.forward(x, lens, want_hidden=False)
    assert fwd["lse"] is not None
    want = ops.ctc_align(fwd["logits"], lab, fwd["outer_len"], lse=fwd["lse"])
    got = eng.align(x, lens, lab)
    for k in KEYS:
        assert torch.equal(got[k], want[k]), k
    assert torch.isfinite(got["score"]).all()
    torch.testing.assert_close(got["score"], plain["score"], rtol=0, atol=1e-3)       # two lse of the same rows, ~1e-6 apart, over 50 frames


def test_engine_align_of_its_own_transcript_reproduces_transcribe():
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg, sd, x, am, _ = _tiny()
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(sd)
    eng.head_argmax = False                                                # the un-fused head: both calls rank the same fp32 logits
    lens = am.sum(-1).to(torch.int32)
    tr = eng.transcribe(x, lens, pad_id=-1, return_frames=True)
    got = eng.align(x, lens, tr["tokens"])
    T2 = tr["best"].shape[1]
    valid = torch.arange(T2, device=DEV)[None, :] < tr["outer_len"][:, None]
    assert torch.equal(got["tgt_len"], tr["n_tokens"])
    assert torch.equal(got["path"][valid], tr["best"][valid]) and (got["path"][~valid] == -1).all()
    assert torch.equal(got["start"], tr["frames"])


def test_model_align_through_the_mask_and_collator_padding():
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.modeling_ebranchformer import CTCAlignment, Wav2Vec2EBranchformerForCTC
    cfg, sd, x, am, lab = _tiny()
    base = dict(shapes.TINY); base.pop("num_fbanks")
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**base))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    model = model.to(DEV).eval()
    assert (lab == -100).any()
    with torch.no_grad():
        got = model.align(x, attention_mask=am, labels=lab)
    want = model._get_engine(x.device).align(x, am.sum(-1).to(torch.int32), lab)
    assert isinstance(got, CTCAlignment)
    for k in ("path", "score", "start", "end", "token_lp"):
        assert torch.equal(getattr(got, k), want[k]), k
    assert torch.equal(got.n_tokens, want["tgt_len"]) and torch.isfinite(got.score).all()
    model.train()
    with pytest.raises(RuntimeError):
        model.align(x, attention_mask=am, labels=lab)
