"""GPU: CTC greedy transcription on the device — the stand-alone kernels (csrc/ctc_decode.hip), the argmax epilogue of the head GEMM (mi_gemm_argmax_bf16),
`EBranchformerEngine.transcribe` and the model surface — against the CPU restatement of the semantics (tests/ctc_greedy_ref.py, itself pinned to the reference's
function by tests/golden/ctc_greedy.npz in tests/test_ctc_decode_cpu.py).  Every comparison is of integers and exact unless it says otherwise."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_greedy_ref as R  # noqa: E402
from helpers import case_inputs, load_golden  # noqa: E402
from huggingface_asr_amd import shapes  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["random", "blank_dominated", "all_blank_row", "single_token_row", "exact_ties", "blank_not_last"]


def _cfg(base, **kw):
    c = dict(base)
    c.update(ctc_zero_infinity=True, ctc_loss_reduction="mean")
    c.update(kw)
    return c


def _check(out, want, B, T, dtype=torch.int64, frames=True):
    """device result dict against the restatement's"""
    assert out["tokens"].dtype == dtype and out["tokens"].shape == (B, T) and out["n_tokens"].dtype == torch.int32
    assert np.array_equal(out["best"].cpu().numpy(), want["best"])
    assert np.array_equal(out["tokens"].cpu().numpy().astype(np.int64), want["tokens"])
    assert np.array_equal(out["n_tokens"].cpu().numpy(), want["n_tokens"])
    if frames:
        assert out["frames"].dtype == torch.int32 and np.array_equal(out["frames"].cpu().numpy(), want["frames"])


# ------------------------------------------------------------------------------------------------ 1. stand-alone kernels
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_cases(golden_dir, name, dtype):
    """the reference's own outputs (the fixture's logits are multiples of 1/8: exact in bf16 too, ties included)"""
    from huggingface_asr_amd import decoding, ops
    x, blank, pad, ids = R.load_case(golden_dir, name)
    xd = x.to(DEV, dtype)
    out = ops.ctc_greedy_decode(xd, blank, pad, return_frames=True)
    assert np.array_equal(out["tokens"].cpu().numpy(), ids)
    _check(out, R.greedy(x, blank, pad), *x.shape[:2])
    got = decoding.ctc_greedy_decode(xd, blank, pad)                      # the drop-in: same positional arguments, (B, T) int64 on the logits' device
    assert got.dtype == torch.int64 and got.device == xd.device and np.array_equal(got.cpu().numpy(), ids)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_head_sized_logits_with_padded_rows(dtype):
    """(32, 250, 5001) in the engine's layout: rows padded to 5008 elements, 5001 not a multiple of the 16-B vectors; lengths with one row at 0 and one at T"""
    from huggingface_asr_amd import ops
    B, T, V1, ld = 32, 250, 5001, 5008
    g = torch.Generator().manual_seed(3)
    buf = torch.full((B, T, ld), 1e30)                                    # the padding columns would win every row if they were read as classes
    buf[..., :V1] = torch.randn(B, T, V1, generator=g)
    buf[..., V1 - 1] += 2.5                                               # blank-dominated, as a trained head is
    buf[:, :, 4996:5001] += torch.randn(B, T, 5, generator=g) * 2         # winners inside the last partial vector too
    bufd = buf.to(DEV, dtype)
    x = bufd[..., :V1]
    assert x.stride() == (T * ld, ld, 1)
    lengths = torch.tensor([0, T] + [T - 7 * i for i in range(B - 2)], dtype=torch.int32)
    xc = x.float().cpu()
    for ln in (None, lengths):
        for tok in (torch.int64, torch.int32):
            out = ops.ctc_greedy_decode(x, V1 - 1, 0, None if ln is None else ln.to(DEV), return_frames=True, dtype=tok)
            _check(out, R.greedy(xc, V1 - 1, 0, None if ln is None else ln.numpy()), B, T, tok)
    assert (np.asarray(R.argmax_frames(xc)) >= 4996).any()
    best = ops.row_argmax(x.reshape(B * T, V1))                           # the 2-D form on the same strided rows
    assert np.array_equal(best.cpu().numpy().reshape(B, T), R.argmax_frames(xc))
    out = ops.ctc_greedy_decode(x, V1 - 1, 0, lengths.to(DEV))
    assert int(out["n_tokens"][0]) == 0 and (out["tokens"][0] == 0).all()


@pytest.mark.parametrize("shape", [(2, 1500, 51), (1, 2500, 5001)], ids=["whisper_frames", "100s_clip"])
def test_long_utterances_cross_the_collapse_chunks(shape):
    """T beyond one 1024-frame chunk of the collapse: the carried count and the predecessor across the chunk edge (long runs, so that edges fall inside runs)"""
    from huggingface_asr_amd import ops
    B, T, V1 = shape
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, V1, generator=g)
    run = torch.randint(0, V1, (B, (T + 2) // 3), generator=g).repeat_interleave(3, dim=1)[:, :T]          # runs of three: every chunk edge but one cuts a run
    x.scatter_add_(2, run[..., None], torch.full((B, T, 1), 6.0))
    x[:, 1020:1030, :] = x[:, 1020:1021, :]                                # one run across frame 1024 in any case
    lengths = torch.tensor([T - 3, 1025][:B], dtype=torch.int32)
    for ln in (None, lengths):
        out = ops.ctc_greedy_decode(x.to(DEV), V1 - 1, 7, None if ln is None else ln.to(DEV), return_frames=True)
        _check(out, R.greedy(x, V1 - 1, 7, None if ln is None else ln.numpy()), B, T)
    best = torch.from_numpy(R.argmax_frames(x)).to(DEV, torch.int32)
    sep = ops.ctc_collapse(best, V1 - 1, 7, return_frames=True)            # mi_ctc_collapse alone
    sep["best"] = best
    _check(sep, R.greedy(x, V1 - 1, 7), B, T)


def test_nan_and_inf_rows():
    from huggingface_asr_amd import ops
    ninf, inf, nan = float("-inf"), float("inf"), float("nan")
    V1 = 300
    x = torch.randn(1, 12, V1, generator=torch.Generator().manual_seed(9))
    x[0, 0, :] = ninf                                                      # all -inf: class 0
    x[0, 1, :] = ninf; x[0, 1, 257] = -1e30
    x[0, 2, 70] = nan; x[0, 2, 3] = inf                                    # a NaN beats +inf
    x[0, 3, 260] = nan; x[0, 3, 130] = nan; x[0, 3, 131] = nan             # the first NaN wins (three lanes, two vectors)
    x[0, 4, :] = nan                                                       # all NaN: class 0
    x[0, 5, 299] = inf; x[0, 5, 298] = inf                                 # equal maxima: the lower index
    x[0, 6, :] = 0.0                                                       # all equal: class 0
    x[0, 7, :] = ninf; x[0, 7, 299] = nan
    x[0, 8, :] = -1.0; x[0, 8, 200] = 0.0; x[0, 8, 9] = -0.0                # -0 equals +0: the lower index
    x[0, 9, :] = -1.0; x[0, 9, 200] = -0.0; x[0, 9, 9] = 1e-42              # a denormal is above both zeros
    want = R.argmax_frames(x)
    assert want[0, :10].tolist() == [0, 257, 70, 130, 0, 298, 0, 299, 9, 9]
    for dt in (torch.float32, torch.bfloat16):
        xd = x.to(DEV, dt)
        assert np.array_equal(ops.row_argmax(xd[0]).cpu().numpy(), R.argmax_frames(xd.float().cpu())[0])
        assert ops.row_argmax(xd[0]).cpu().numpy()[:9].tolist() == want[0, :9].tolist()
        _check(ops.ctc_greedy_decode(xd, V1 - 1, 0, return_frames=True), R.greedy(xd.float().cpu(), V1 - 1, 0), 1, 12)
    un = torch.randn(5, 77, generator=torch.Generator().manual_seed(2)).to(DEV)[:, 1:]          # rows that are not 16-B aligned: the element-wise path
    assert np.array_equal(ops.row_argmax(un).cpu().numpy(), torch.argmax(un.cpu(), -1).numpy())


# ------------------------------------------------------------------------------------------------ 2. the head GEMM's argmax epilogue
def _head_operands(M, N, K, seed, ties=()):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(torch.bfloat16)
    b = torch.randn(N, generator=g) * 0.1
    for lo, hi in ties:                                                    # class hi = class lo: same weight row, same bias -> the same fp32 logit in every row
        w[hi] = w[lo]; b[hi] = b[lo]
    return a.to(DEV), w.to(DEV), b.to(DEV)


@pytest.mark.parametrize("M,N,K", [(8000, 5001, 512), (7993, 5001, 256), (8000, 51, 512), (7993, 51, 256)])
def test_gemm_argmax_equals_argmax_of_the_head_gemm(M, N, K):
    """right-hand side: row_argmax over the fp32 output of the existing head GEMM (unchanged by this work) on the same operands"""
    from huggingface_asr_amd import _lib, ops
    a, w, b = _head_operands(M, N, K, 11)
    logits = ops.gemm(a, w, b, out_dtype=torch.float32)
    want = ops.row_argmax(logits)
    assert np.array_equal(want.cpu().numpy(), torch.argmax(logits.cpu(), -1).numpy())
    ws = torch.empty((int(_lib.lib().mi_gemm_argmax_workspace_floats(M, N)),), device=DEV, dtype=torch.float32)
    best = torch.full((M,), -1, device=DEV, dtype=torch.int32)
    rc = _lib.lib().mi_gemm_argmax_bf16(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), b.data_ptr(), best.data_ptr(), ws.data_ptr(), M, N, K, ops._stream())
    assert rc == 0                                                         # these shapes run the fused kernel itself, not the fallback
    assert torch.equal(best, want)
    assert torch.equal(ops.gemm_argmax(a, w, b), want)
    assert torch.equal(ops.gemm_argmax(a, w, None), ops.row_argmax(ops.gemm(a, w, None, out_dtype=torch.float32)))


def test_gemm_argmax_ties_across_wave_blocks_and_tiles():
    """two classes with the same weight row and bias tie exactly in every row; boosted so that they ARE the row maxima: the lower index must win across 64-column
    wave blocks (10 / 100), across 256-column tiles (300 / 4000) and into the last, partial tile (70 / 5000)"""
    from huggingface_asr_amd import ops
    M, N, K = 2048, 5001, 512
    pairs = [(10, 100), (300, 4000), (70, 5000)]
    a, w, b = _head_operands(M, N, K, 13, ties=pairs)
    for lo, hi in pairs:
        b2 = b.clone(); b2[lo] += 50.0; b2[hi] += 50.0
        logits = ops.gemm(a, w, b2, out_dtype=torch.float32)
        assert torch.equal(logits[:, lo], logits[:, hi])
        best = ops.gemm_argmax(a, w, b2)
        assert (best == lo).all(), (lo, hi, best.unique().tolist())
        assert torch.equal(best, ops.row_argmax(logits))
    b3 = b.clone(); b3[4000] += 50.0; b3[300] += 50.0; b3[5000] += 50.0; b3[70] += 50.0       # both pairs on top: whichever pair wins a row, its lower member
    logits = ops.gemm(a, w, b3, out_dtype=torch.float32)
    best = ops.gemm_argmax(a, w, b3)
    assert torch.equal(best, ops.row_argmax(logits)) and set(best.unique().tolist()) <= {70, 300}


def test_gemm_argmax_unsupported_shape_takes_the_fallback():
    """K = 64 is below the 256 x 256 kernel's two K tiles: the C entry says MI_ERR_UNSUPPORTED, the op runs GEMM + row_argmax"""
    from huggingface_asr_amd import _lib, ops
    M, N, K = 300, 51, 64
    a, w, b = _head_operands(M, N, K, 17)
    ws = torch.empty((int(_lib.lib().mi_gemm_argmax_workspace_floats(M, N)),), device=DEV, dtype=torch.float32)
    best = torch.empty((M,), device=DEV, dtype=torch.int32)
    rc = _lib.lib().mi_gemm_argmax_bf16(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), b.data_ptr(), best.data_ptr(), ws.data_ptr(), M, N, K, ops._stream())
    assert rc == _lib.ERR_UNSUPPORTED
    logits = ops.gemm(a, w, b, out_dtype=torch.float32)
    assert torch.equal(ops.gemm_argmax(a, w, b), ops.row_argmax(logits))
    assert np.array_equal(ops.gemm_argmax(a, w, b).cpu().numpy(), torch.argmax(logits.cpu(), -1).numpy())


# ------------------------------------------------------------------------------------------------ 3. engine.transcribe
ENGINE_CASES = [
    ("tiny_rel", _cfg(shapes.TINY)),
    ("tiny_rotary", _cfg(shapes.TINY, position_embeddings_type="rotary")),
    ("tiny_causal", _cfg(shapes.TINY, is_causal=True)),
    ("small_rel", _cfg(shapes.SMALL)),
    ("base_rel", _cfg(shapes.BASE)),
]


def _engine(cfg, sd):
    from huggingface_asr_amd.engine import EBranchformerEngine
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(sd)
    return eng


def _same(a, b, keys=("best", "tokens", "n_tokens")):
    return all(torch.equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("span", ["valid", "all"])
@pytest.mark.parametrize("name,cfg", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_transcribe_fused_unfused_and_logits_path_agree(name, cfg, span):
    """seeded weights and the padded batch of the encoder fixtures: the head's argmax epilogue, GEMM + argmax pass, and decoding the engine's own logits give the same
    per-frame classes, ids and counts; utterance i decoded alone equals row i of the batch up to its length; two calls give the same bits"""
    from huggingface_asr_amd import ops
    g = load_golden(name)
    sd, x, am, _ = case_inputs(g, cfg)
    eng = _engine(cfg, sd)
    xd, lens = x.to(DEV), am.sum(-1).to(DEV, torch.int32)
    V1, pad = cfg["vocab_size"] + 1, 3
    fwd = eng.forward(xd, lens)
    ref = ops.ctc_greedy_decode(fwd["logits"], V1 - 1, pad, fwd["outer_len"] if span == "valid" else None, return_frames=True)
    assert np.array_equal(ref["best"].cpu().numpy(), R.argmax_frames(fwd["logits"]))
    eng.head_argmax = True
    fused = eng.transcribe(xd, lens, span=span, pad_id=pad, return_frames=True, want_hidden=True)
    eng.head_argmax = False
    plain = eng.transcribe(xd, lens, span=span, pad_id=pad, return_frames=True)
    assert _same(fused, ref, ("best", "tokens", "n_tokens", "frames")) and _same(plain, ref, ("best", "tokens", "n_tokens", "frames"))
    assert torch.equal(fused["outer_len"], fwd["outer_len"]) and torch.equal(fused["inner_len"], fwd["inner_len"])
    assert torch.equal(fused["last_hidden"], fwd["last_hidden"]) and "last_hidden" not in plain
    want = R.collapse(ref["best"].cpu().numpy(), V1 - 1, pad, fwd["outer_len"].cpu().numpy() if span == "valid" else None)
    assert np.array_equal(fused["tokens"].cpu().numpy(), want[0]) and np.array_equal(fused["n_tokens"].cpu().numpy(), want[1])
    if span == "valid":
        assert int(fused["n_tokens"].max()) > 0 and (fused["n_tokens"] <= fwd["outer_len"]).all()
    eng.head_argmax = True
    again = eng.transcribe(xd, lens, span=span, pad_id=pad, return_frames=True)
    assert _same(again, fused, ("best", "tokens", "n_tokens", "frames"))
    assert eng._head_fusable() == (cfg["hidden_size"] >= 128)          # tiny heads (K = 64) are outside the fused kernel: they run GEMM + argmax pass in either mode
    if span == "valid":
        for i in range(xd.shape[0]):
            one = eng.transcribe(xd[i:i + 1].contiguous(), lens[i:i + 1].contiguous(), span=span, pad_id=pad)
            n, k = int(fwd["outer_len"][i]), int(fused["n_tokens"][i])
            assert torch.equal(one["best"][0, :n], fused["best"][i, :n]) and int(one["n_tokens"][0]) == k
            assert torch.equal(one["tokens"][0, :k], fused["tokens"][i, :k])


def test_transcribe_at_the_bench_size_is_batch_independent_and_reproducible():
    """base encoder, 32 x 10 s (the fused head at its real shape, folded LayerNorms): against the logits path, row i alone, and itself"""
    from huggingface_asr_amd import ops, synth
    cfg = _cfg(shapes.BASE)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 0).items()}
    eng = _engine(cfg, sd)
    eng.ln_fold = True                                                     # pinned, so that a batch of one runs the same layer form (tests/test_gpu_encoder.py)
    B, T, V1 = 32, 1000, cfg["vocab_size"] + 1
    feats = torch.from_numpy(synth.normal(7, "feats", (B, T, 80), 1.0)).to(DEV)
    lens = torch.tensor([998 - 37 * (i % 9) for i in range(B)], dtype=torch.int32, device=DEV)
    feats = feats * (torch.arange(T, device=DEV)[None, :, None] < lens[:, None, None])
    fwd = eng.forward(feats, lens)
    ref = ops.ctc_greedy_decode(fwd["logits"], V1 - 1, 0, fwd["outer_len"])
    eng.head_argmax = True
    got = eng.transcribe(feats, lens, pad_id=0)
    assert eng._head_fusable() and _same(got, ref)
    eng.head_argmax = False
    assert _same(eng.transcribe(feats, lens, pad_id=0), ref)
    eng.head_argmax = True
    for _ in range(3):
        assert _same(eng.transcribe(feats, lens, pad_id=0), got)
    for i in (0, 5, 31):
        one = eng.transcribe(feats[i:i + 1].contiguous(), lens[i:i + 1].contiguous(), pad_id=0)
        n, k = int(got["outer_len"][i]), int(got["n_tokens"][i])
        assert torch.equal(one["best"][0, :n], got["best"][i, :n]) and int(one["n_tokens"][0]) == k and torch.equal(one["tokens"][0, :k], got["tokens"][i, :k])


def test_transcribe_from_pipeline_lanes():
    """ForwardPipeline runs transcribe on its lanes as it runs forward: lanes 0-3, each on its own stream and workspace, give the single-stream ids"""
    from huggingface_asr_amd import synth
    from huggingface_asr_amd.pipeline import ForwardPipeline
    cfg = _cfg(shapes.BASE)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 0).items()}
    lens = torch.full((32,), 998, dtype=torch.int32, device=DEV)
    pipe = ForwardPipeline(cfg, DEV, sd, lanes=4)
    feats = [torch.from_numpy(synth.normal(11 + i, "feats", (32, 1000, 80), 1.0)).to(DEV) for i in range(4)]
    for e in pipe.engines:
        e.head_argmax = True                                               # the fused head: its workspace is per call, so lanes share nothing but the weights
    refs = [pipe.engines[i].transcribe(feats[i], lens, pad_id=0) for i in range(4)]
    torch.cuda.synchronize()
    outs = [pipe.submit(lambda e, lane: e.transcribe(feats[lane], lens, pad_id=0)) for _ in range(12)]
    torch.cuda.synchronize()
    assert [lane for lane, _ in outs] == [j % 4 for j in range(12)]
    for k, (lane, got) in enumerate(outs):
        assert _same(got, refs[lane]), k
    assert not _same(refs[0], refs[1])                                     # different batches, different transcripts: the comparison above is not vacuous


# ------------------------------------------------------------------------------------------------ 4. against the reference's logits
@pytest.mark.parametrize("name,cfg", ENGINE_CASES[:3], ids=[c[0] for c in ENGINE_CASES[:3]])
def test_best_equals_the_reference_argmax_where_its_margin_allows(name, cfg):
    """The fixtures hold the reference's full fp32 logits.  tests/test_gpu_encoder.py holds the engine to max |dlogit| < 0.06 against them: where the reference's top two
    classes are more than 0.12 apart, winner and runner-up cannot change places, so the engine's per-frame class must BE the reference's.  (Random-weight models:
    logit std ~0.8 over 51 classes, so a third of the frames are closer than that and are left out; the share compared is asserted, at least 60 % of each fixture's
    valid frames.)"""
    g = load_golden(name)
    sd, x, am, _ = case_inputs(g, cfg)
    eng = _engine(cfg, sd)
    out = eng.transcribe(x.to(DEV), am.sum(-1).to(DEV, torch.int32), pad_id=0)
    ref = torch.from_numpy(g["logits"]).float()
    top2 = ref.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1]).numpy()
    outer = np.asarray(g["outer_lens"])
    valid = np.arange(ref.shape[1])[None, :] < outer[:, None]
    use = valid & (margin > 0.12)
    share = use.sum() / valid.sum()
    print(f"{name}: {use.sum()} of {valid.sum()} valid frames compared ({share:.1%})")
    assert share >= 0.60, share
    best = out["best"].cpu().numpy()
    assert np.array_equal(best[use], R.argmax_frames(ref)[use])


# ------------------------------------------------------------------------------------------------ 5. model surface
def test_model_transcribe_equals_decoding_its_logits():
    from huggingface_asr_amd import decoding
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    cfg = _cfg(shapes.TINY)
    g = load_golden("tiny_rel")
    sd, x, am, _ = case_inputs(g, cfg)
    base = dict(shapes.TINY); base.pop("num_fbanks")
    pad = 3
    model = Wav2Vec2EBranchformerForCTC(Wav2Vec2EBranchformerConfig(**base, pad_token_id=pad))
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    model = model.to(DEV).eval()
    V = cfg["vocab_size"]
    with torch.no_grad():
        logits = model(x.to(DEV), attention_mask=am.to(DEV)).logits
        ids_all, n_all = model.transcribe(x.to(DEV), attention_mask=am.to(DEV), span="all")
        ids, n = model.transcribe(x.to(DEV), attention_mask=am.to(DEV))
    full = decoding.ctc_greedy_decode(logits, V, pad)
    assert ids_all.dtype == torch.int64 and torch.equal(ids_all, full)
    assert np.array_equal(n_all.cpu().numpy(), (R.collapse(R.argmax_frames(logits), V, pad)[1]))
    outer = np.asarray(g["outer_lens"])
    want = R.greedy(logits, V, pad, outer)                                 # the same call cut at the outer lengths
    assert np.array_equal(ids.cpu().numpy(), want["tokens"]) and np.array_equal(n.cpu().numpy(), want["n_tokens"])
    for b in range(ids.shape[0]):
        cut = decoding.ctc_greedy_decode(logits[b:b + 1, :int(outer[b])].contiguous(), V, pad)[0]
        k = int(n[b])
        assert torch.equal(ids[b, :k], cut[:k]) and (cut[k:] == pad).all() and (ids[b, k:] == pad).all()
    model.train()
    with pytest.raises(RuntimeError):
        model.transcribe(x.to(DEV))
