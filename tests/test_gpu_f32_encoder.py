"""The fp32 inference mode (`EBranchformerEngine(..., precision="fp32")`, mi_ebf_forward_f32) end to end — SURVEY.md §7's acceptance tier (i), "fp32-mode kernels
vs fp32 oracle: max |dlogit| <= 1e-3", which no test could reach while the library had a bf16 mode only.

The engine against the reference's own fp32 goldens, held to the bars tests/test_oracle_golden.py holds the fp32 CPU oracle to — the project's definition of "an fp32
implementation agrees with the reference":
    tiny:          atol 2e-4 on `logits` and `last_hidden`
    small / base:  5e-4 on `logits_slice` and `logits_blank`, |std - logits_std| < 1e-4
    all:           relative CTC-loss error < 1e-4, `outer_len` / `inner_len` equal
Every one of them is inside BASELINE.json north_star's 1e-3.  (The bf16 mode's bars on the same fixtures, tests/test_gpu_encoder.py: max 0.06 / mean 0.009.)
Each case prints what it observed: `F32ENC <fixture> max|dlogit|=... max|dhidden|=... loss rel=...` (pytest -s); the maxima are recorded in DESIGN.md §4.

Then: the default mode is untouched (an engine built without the argument and one built with precision="bf16" give the same bits), transcribe() in fp32 mode, the
model-level switch (`config.hip_precision`), and run-to-run bit identity."""
import numpy as np
import pytest
import torch

import ctc_greedy_ref as GR
from helpers import case_inputs, load_golden
from huggingface_asr_amd import shapes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(base, **kw):
    c = dict(base)
    c.update(ctc_zero_infinity=True, ctc_loss_reduction="mean")
    c.update(kw)
    return c


CASES = {
    "tiny_rel": _cfg(shapes.TINY),
    "tiny_rotary": _cfg(shapes.TINY, position_embeddings_type="rotary"),
    "tiny_causal": _cfg(shapes.TINY, is_causal=True),
    "tiny_nomacaron": _cfg(shapes.TINY, csgu_activation="gelu", csgu_use_linear_after_conv=True),
    "tiny_shared_gated_fallthrough": _cfg(shapes.TINY, context_awareness_type="shared_gated"),      # the reference's dict lookup resolves it to the plain conv
    "small_rel": _cfg(shapes.SMALL),
    "small_causal": _cfg(shapes.SMALL, is_causal=True),
    "base_rel": _cfg(shapes.BASE),
    "base_rotary": _cfg(shapes.BASE, position_embeddings_type="rotary"),
}
_RUNS = {}


def _engine(name, precision="fp32", **kw):
    from huggingface_asr_amd.engine import EBranchformerEngine
    g = load_golden(name)
    sd, x, am, lab = case_inputs(g, CASES[name])
    eng = EBranchformerEngine(CASES[name], DEV, **({} if precision is None else dict(precision=precision)), **kw)
    eng.load_state_dict(sd)
    return eng, g, x.to(DEV), am.sum(-1).to(DEV, torch.int32), lab.to(DEV)


def _run(name):
    """one fp32 forward per fixture, shared by the tests below (nothing mutates it)"""
    if name not in _RUNS:
        from huggingface_asr_amd import ops
        eng, g, x, fl, lab = _engine(name)
        out = eng.forward(x, fl)
        loss, _, _ = ops.ctc_loss(out["logits"], lab, out["outer_len"], reduction="mean", zero_infinity=True)
        torch.cuda.synchronize()
        _RUNS[name] = (eng, g, x, fl, lab, out, float(loss))
    return _RUNS[name]


@pytest.mark.parametrize("name", [n for n in CASES if n.startswith("tiny")])
def test_fp32_engine_tiny_full_tensors(name):
    _, g, _, _, _, out, loss = _run(name)
    logits, hidden = out["logits"].cpu().numpy(), out["last_hidden"].cpu().numpy()
    assert out["logits"].dtype == torch.float32
    dl, dh = np.abs(logits - g["logits"]).max(), np.abs(hidden - g["last_hidden"]).max()
    rel = abs(loss - float(g["loss"])) / abs(float(g["loss"]))
    print(f"F32ENC {name} max|dlogit|={dl:.3e} max|dhidden|={dh:.3e} loss rel={rel:.2e}")
    np.testing.assert_array_equal(out["outer_len"].cpu().numpy(), g["outer_lens"])
    np.testing.assert_array_equal(out["inner_len"].cpu().numpy(), g["inner_lens"])
    np.testing.assert_allclose(hidden, g["last_hidden"], atol=2e-4, rtol=0)
    np.testing.assert_allclose(logits, g["logits"], atol=2e-4, rtol=0)
    assert rel < 1e-4


@pytest.mark.parametrize("name", [n for n in CASES if not n.startswith("tiny")])
def test_fp32_engine_small_base_slices(name):
    _, g, _, _, _, out, loss = _run(name)
    lg = out["logits"].cpu().numpy()
    assert lg.shape == (2, 250, 5001)
    d1, d2 = np.abs(lg[:, ::25, :64] - g["logits_slice"]).max(), np.abs(lg[:, :, -1] - g["logits_blank"]).max()
    rel = abs(loss - float(g["loss"])) / abs(float(g["loss"]))
    print(f"F32ENC {name} max|dlogit| slice={d1:.3e} blank={d2:.3e} dstd={abs(float(lg.std()) - float(g['logits_std'])):.2e} loss rel={rel:.2e}")
    np.testing.assert_array_equal(out["outer_len"].cpu().numpy(), g["outer_lens"])
    np.testing.assert_array_equal(out["inner_len"].cpu().numpy(), g["inner_lens"])
    np.testing.assert_allclose(lg[:, ::25, :64], g["logits_slice"], atol=5e-4, rtol=0)
    np.testing.assert_allclose(lg[:, :, -1], g["logits_blank"], atol=5e-4, rtol=0)
    assert abs(float(lg.std()) - float(g["logits_std"])) < 1e-4
    assert rel < 1e-4


@pytest.mark.parametrize("name", ["tiny_rel", "base_rel"])
def test_default_mode_is_unchanged(name):
    """an engine built without the argument and one built with precision="bf16": the same slot dtypes, the same bits"""
    a, _, x, fl, _ = _engine(name, precision=None)
    b, _, _, _, _ = _engine(name, precision="bf16")
    assert a.precision == b.precision == "bf16"
    assert [None if t is None else t.dtype for t in a._slots] == [None if t is None else t.dtype for t in b._slots]
    oa, ob = a.forward(x, fl), b.forward(x, fl)
    assert torch.equal(oa["logits"], ob["logits"]) and torch.equal(oa["last_hidden"], ob["last_hidden"])
    f32 = _run(name)[5]["logits"]
    assert not torch.equal(f32, oa["logits"])                       # and the fp32 mode is a different computation, not an alias


@pytest.mark.parametrize("name", ["tiny_rel", "small_rel"])
def test_fp32_forward_is_bit_reproducible(name):
    eng, _, x, fl, _, out, _ = _run(name)
    again = eng.forward(x, fl)
    assert torch.equal(again["logits"], out["logits"]) and torch.equal(again["last_hidden"], out["last_hidden"])


@pytest.mark.parametrize("span", ["valid", "all"])
def test_fp32_transcribe_equals_collapsing_its_own_logits(span):
    """greedy: the head GEMM's fp32 logits, mi_row_argmax, mi_ctc_collapse == tests/ctc_greedy_ref.py over the same engine's forward() logits; lengths (T, T/2)"""
    eng, _, x, _, _, _, _ = _run("tiny_rel")
    T = x.shape[1]
    fl = torch.tensor([T, T // 2], dtype=torch.int32, device=DEV)
    V, pad = eng.cfg["vocab_size"], 0
    fwd = eng.forward(x, fl)
    got = eng.transcribe(x, fl, span=span, pad_id=pad, return_frames=True)
    want = GR.greedy(fwd["logits"], V, pad, fwd["outer_len"].cpu().numpy() if span == "valid" else None)
    np.testing.assert_array_equal(got["best"].cpu().numpy(), want["best"])
    np.testing.assert_array_equal(got["tokens"].cpu().numpy(), want["tokens"])
    np.testing.assert_array_equal(got["n_tokens"].cpu().numpy(), want["n_tokens"])
    np.testing.assert_array_equal(got["frames"].cpu().numpy(), want["frames"])
    assert int(got["n_tokens"].sum()) > 0


def test_fp32_transcribe_with_beams():
    """beams=5 through ops.ctc_beam_decode over the fp32 logits: the best hypothesis' score (log of its summed alignment probability) is at least the log-probability
    of the single greedy path"""
    eng, _, x, _, _, _, _ = _run("tiny_rel")
    T = x.shape[1]
    fl = torch.tensor([T, T // 2], dtype=torch.int32, device=DEV)
    fwd = eng.forward(x, fl)
    out = eng.transcribe(x, fl, beams=5, pad_id=0)
    assert out["tokens"].shape == fwd["logits"].shape[:2] and out["scores"].shape == (2, 1)
    lp = torch.log_softmax(fwd["logits"].double(), -1).max(-1).values.cpu()
    n = fwd["outer_len"].cpu()
    greedy = torch.stack([lp[b, : int(n[b])].sum() for b in range(2)])
    assert bool((out["scores"][:, 0].cpu().double() >= greedy - 1e-4).all()), (out["scores"], greedy)


def _model(hip_precision):
    from huggingface_asr_amd.configuration_ebranchformer import Wav2Vec2EBranchformerConfig
    from huggingface_asr_amd.modeling_ebranchformer import Wav2Vec2EBranchformerForCTC
    base = dict(shapes.TINY); base.pop("num_fbanks")
    cfg = Wav2Vec2EBranchformerConfig(**base, ctc_zero_infinity=True, ctc_loss_reduction="mean", pad_token_id=0)
    if hip_precision is not None:
        cfg.hip_precision = hip_precision
    model = Wav2Vec2EBranchformerForCTC(cfg)
    g = load_golden("tiny_rel")
    sd, x, am, lab = case_inputs(g, CASES["tiny_rel"])
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    return model.to(DEV), g, x.to(DEV), am.to(DEV), lab.to(DEV)


def test_model_level_fp32_switch():
    """config.hip_precision = "fp32": the eval forward is the engine's (same bits), the loss is the golden's; switching the value rebuilds the engine; train mode refuses"""
    model, g, x, am, lab = _model("fp32")
    model.eval()
    with torch.no_grad():
        out = model(x, attention_mask=am, labels=lab)
    assert model._engine.precision == "fp32"
    assert torch.equal(out.logits, _run("tiny_rel")[5]["logits"])
    assert abs(float(out.loss) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    tokens, n = model.transcribe(x, am)
    want = GR.greedy(out.logits, model.config.vocab_size, 0, _run("tiny_rel")[5]["outer_len"].cpu().numpy())
    np.testing.assert_array_equal(tokens.cpu().numpy(), want["tokens"])
    model.config.hip_precision = "bf16"
    with torch.no_grad():
        out16 = model(x, attention_mask=am)
    assert model._engine.precision == "bf16" and not torch.equal(out16.logits, out.logits)
    model.config.hip_precision = "fp32"
    model.train()
    with pytest.raises(NotImplementedError, match="fp32"):
        model(x, attention_mask=am, labels=lab)


def test_fp32_refusals_on_the_device_engine():
    eng, _, x, fl, _, _, _ = _run("tiny_rel")
    with pytest.raises(NotImplementedError, match="want_all_hidden"):
        eng.forward(x, fl, want_all_hidden=True)
    with pytest.raises(NotImplementedError, match="lanes"):
        eng.forward(x, fl, slot=1)
