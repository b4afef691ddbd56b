"""GPU: Whisper encoder training on the HIP path — the attention backward with no score-sized tensor (attn_bwd_fused.hip), the encoder's backward against
transformers' own autograd, and `WhisperForConditionalGeneration` training under HFASR_WHISPER_STRICT=1 (no PyTorch encoder pass).

Gradient bounds: the HIP path keeps weights and activations in bf16 (8 significant bits, relative rounding 2^-9 ~ 2e-3 per operand) and sums in fp32; a
gradient passes through ~10 such roundings per layer, so a per-tensor relative error ||g - g_ref|| / ||g_ref|| of a few 1e-3 is the expected level and 2e-2
leaves room for the deeper tensors.  A wrong term (a missing path, a transposed operand, a wrong scale) gives O(1) relative error or cosine < 0.99."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL, COS = 2e-2, 0.999


def _close(g, r, rel=REL, cos=COS, what=""):
    g, r = g.double().flatten(), r.double().flatten()
    e = float((g - r).norm() / r.norm().clamp_min(1e-30))
    c = float(torch.dot(g, r) / (g.norm() * r.norm()).clamp_min(1e-30))
    assert e <= rel and c >= cos, (what, e, c)


def _attn_case(B, T, H, hd, lengths=None, seed=0):
    from huggingface_asr_amd import ops
    gen = torch.Generator().manual_seed(seed)
    d = H * hd
    qkv = (torch.randn(B * T, 3 * d, generator=gen) * 0.5).to(DEV, torch.bfloat16)
    dctx = torch.randn(B * T, d, generator=gen).to(DEV, torch.bfloat16)
    ln = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    lse = torch.empty((B, H, T), device=DEV, dtype=torch.float32)
    ctx = ops.attention_qkv(qkv, B, T, H, lengths=ln, lse=lse)
    return qkv, ctx, dctx, lse, ln


def _attn_ref(qkv, dctx, B, T, H, hd, lengths):
    d = H * hd
    x = qkv.double().cpu().requires_grad_(True)
    q, k, v = [x[:, i * d:(i + 1) * d].view(B, T, H, hd).transpose(1, 2) for i in range(3)]
    s = q @ k.transpose(-1, -2) / math.sqrt(hd)
    if lengths is not None:
        m = torch.arange(T)[None, :] >= torch.tensor(lengths)[:, None]
        s = s.masked_fill(m[:, None, None, :], float("-inf"))
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B * T, d)
    o.backward(dctx.double().cpu())
    return x.grad


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("B,T,H,lens", [(2, 1, 2, None), (2, 37, 2, None), (2, 37, 2, [37, 20]), (2, 250, 2, None), (2, 250, 3, [250, 111]),
                                        (1, 1500, 1, None), (1, 1500, 1, [1000])])
def test_attn_bwd_fused_matches_fp64_and_materialising_path(B, T, H, hd, lens):
    from huggingface_asr_amd import ops_train as OT
    qkv, ctx, dctx, lse, ln = _attn_case(B, T, H, hd, lens)
    d = H * hd
    g = OT.attn_bwd_fused(qkv, B, T, H, ctx, dctx, lse, torch.empty((B * T, 3 * d), device=DEV, dtype=torch.bfloat16), lengths=ln)
    g2 = OT.attn_bwd_fused(qkv, B, T, H, ctx, dctx, lse, torch.full((B * T, 3 * d), 7.0, device=DEV, dtype=torch.bfloat16), lengths=ln)
    torch.cuda.synchronize()
    assert torch.equal(g, g2)                                      # bit-identical runs, every element written
    assert torch.isfinite(g.float()).all()
    ref = _attn_ref(qkv, dctx, B, T, H, hd, lens)
    for i, n in enumerate("qkv"):
        if float(ref[:, i * d:(i + 1) * d].norm()) > 0:
            _close(g[:, i * d:(i + 1) * d].float().cpu(), ref[:, i * d:(i + 1) * d], what=f"d{n}")
    if lens is not None:                                           # keys beyond a length get exactly zero dK / dV
        for b, L in enumerate(lens):
            assert float(g[b * T + L:(b + 1) * T, d:].float().abs().sum()) == 0.0
    m = OT.attn_bwd_materialized(qkv, B, T, H, ctx, dctx, lse, torch.zeros((B * T, 3 * d), device=DEV, dtype=torch.bfloat16), lengths=ln)
    _close(g.float(), m.float(), rel=1e-2, cos=0.9999, what="vs materialising")


def _tiny_cfg(**kw):
    from transformers import WhisperConfig
    c = dict(d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=256,
             num_mel_bins=80, max_source_positions=64, max_target_positions=32, vocab_size=100, pad_token_id=0, bos_token_id=1, eos_token_id=2,
             decoder_start_token_id=1, suppress_tokens=None, begin_suppress_tokens=None)
    c.update(kw)
    return WhisperConfig(**c)


def _encoder(cfg, seed=0):
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    from huggingface_asr_amd import bind
    bind.bind_all()
    torch.manual_seed(seed)
    enc = WhisperEncoder(cfg)
    with torch.no_grad():                                          # non-trivial LayerNorms
        for n, p in enc.named_parameters():
            if "layer_norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    return enc.to(DEV).train()


def _grads(enc, x, proj, hip):
    from transformers.models.whisper import modeling_whisper as MW
    enc.zero_grad(set_to_none=True)
    x = x.clone().requires_grad_(True)
    out = enc(x).last_hidden_state if hip else MW.WhisperEncoder._hfasr_reference_forward(enc, x).last_hidden_state
    (out * proj).sum().backward()
    return {n: p.grad.clone() if p.grad is not None else None for n, p in enc.named_parameters()}, x.grad.clone(), out.detach()


def _strict():
    os.environ["HFASR_WHISPER_STRICT"] = "1"


@pytest.mark.parametrize("fused", [True, False])
def test_encoder_gradients_match_transformers(fused, monkeypatch):
    from huggingface_asr_amd.whisper import WhisperEncoderEngine
    monkeypatch.setattr(WhisperEncoderEngine, "fused_attn_bwd", fused)
    _strict()
    try:
        cfg = _tiny_cfg()
        enc = _encoder(cfg)
        enc.embed_positions.weight.requires_grad_(True)            # unfrozen here so that its gradient is checked too
        g = torch.Generator().manual_seed(1)
        x = torch.randn(2, 80, 128, generator=g).to(DEV)
        proj = torch.randn(2, 64, 128, generator=g).to(DEV)
        gh, xh, oh = _grads(enc, x, proj, True)
        gr, xr, orf = _grads(enc, x, proj, False)
        _close(oh, orf, what="last_hidden_state")
        for n in gr:
            assert (gh[n] is None) == (gr[n] is None), n
            if gr[n] is not None:
                assert gh[n].shape == gr[n].shape and gh[n].dtype == gr[n].dtype
                _close(gh[n], gr[n], what=n)
        assert gh["layers.0.self_attn.k_proj.weight"] is not None
        _close(xh, xr, what="input_features")
        # reproducibility: an identical step gives bit-identical gradients
        gh2, xh2, _ = _grads(enc, x, proj, True)
        assert all(torch.equal(gh[n], gh2[n]) for n in gh if gh[n] is not None) and torch.equal(xh, xh2)
    finally:
        os.environ.pop("HFASR_WHISPER_STRICT", None)


@pytest.mark.parametrize("fused", [True, False])
def test_whisper_small_real_shape_one_step(fused, monkeypatch):
    from huggingface_asr_amd.whisper import WhisperEncoderEngine
    monkeypatch.setattr(WhisperEncoderEngine, "fused_attn_bwd", fused)
    _strict()
    try:
        cfg = _tiny_cfg(d_model=768, encoder_layers=12, encoder_attention_heads=12, encoder_ffn_dim=3072, max_source_positions=1500)
        enc = _encoder(cfg)
        g = torch.Generator().manual_seed(2)
        x = torch.randn(2, 80, 3000, generator=g).to(DEV)
        proj = torch.randn(2, 1500, 768, generator=g).to(DEV) / 100
        gh, xh, _ = _grads(enc, x, proj, True)
        gr, xr, _ = _grads(enc, x, proj, False)
        for n in ("conv1.weight", "conv1.bias", "layers.0.self_attn.q_proj.weight", "layers.0.fc1.weight", "layers.11.self_attn.v_proj.weight",
                  "layers.11.fc2.weight", "layer_norm.weight"):
            _close(gh[n], gr[n], rel=3e-2, cos=0.999, what=n)
    finally:
        os.environ.pop("HFASR_WHISPER_STRICT", None)


def test_conditional_generation_trains_under_strict():
    """Fails before this feature: training mode raised NotImplementedError under HFASR_WHISPER_STRICT=1."""
    from transformers import WhisperForConditionalGeneration
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd import bind
    bind.bind_all()
    cfg = _tiny_cfg()
    torch.manual_seed(0)
    hip = WhisperForConditionalGeneration(cfg).to(DEV).train()
    ref = WhisperForConditionalGeneration(cfg).to(DEV).train()
    ref.load_state_dict(hip.state_dict())
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 80, 128, generator=g).to(DEV)
    labels = torch.randint(3, 100, (2, 6), generator=g).to(DEV)
    oh = torch.optim.AdamW(hip.parameters(), lr=1e-3)
    orf = torch.optim.AdamW(ref.parameters(), lr=1e-3)
    losses = []
    _strict()
    try:
        for step in range(3):
            oh.zero_grad(); orf.zero_grad()
            lh = hip(input_features=x, labels=labels).loss
            lh.backward()
            MW.WhisperEncoder.forward = MW.WhisperEncoder._hfasr_reference_forward
            try:
                lr = ref(input_features=x, labels=labels).loss
                lr.backward()
            finally:
                MW.WhisperEncoder.forward = bind_forward()
            if step == 0:
                for (n, p), (_, q) in zip(hip.model.encoder.named_parameters(), ref.model.encoder.named_parameters()):
                    if q.grad is not None and float(q.grad.norm()) > 0:
                        _close(p.grad, q.grad, what=n)
            losses.append((float(lh), float(lr)))
            oh.step(); orf.step()
    finally:
        os.environ.pop("HFASR_WHISPER_STRICT", None)
    for a, b in losses:
        assert abs(a - b) <= 2e-2 * abs(b), losses


def bind_forward():
    from huggingface_asr_amd.whisper import hip_whisper_encoder_forward
    return hip_whisper_encoder_forward


def test_layerdrop_skips_the_same_layers_as_transformers():
    _strict()
    try:
        cfg = _tiny_cfg(encoder_layers=6, encoder_layerdrop=0.5)
        enc = _encoder(cfg)
        x = torch.randn(1, 80, 128).to(DEV)
        proj = torch.randn(1, 64, 128).to(DEV)
        torch.manual_seed(11)
        gh, _, oh = _grads(enc, x, proj, True)
        torch.manual_seed(11)
        gr, _, orf = _grads(enc, x, proj, False)
        _close(oh, orf, what="out")
        skipped = {l for l in range(6) if gr[f"layers.{l}.fc1.weight"] is None}
        assert skipped and len(skipped) < 6, skipped                # seed 11 drops some, not all
        for l in range(6):
            assert (gh[f"layers.{l}.fc1.weight"] is None) == (l in skipped), l
    finally:
        os.environ.pop("HFASR_WHISPER_STRICT", None)


def test_frozen_parts_and_fallbacks():
    import warnings
    _strict()
    try:
        enc = _encoder(_tiny_cfg())
        for n, p in enc.named_parameters():
            if n.startswith("conv") or n.startswith("layers.0."):
                p.requires_grad_(False)
        x = torch.randn(2, 80, 128).to(DEV)
        enc(x).last_hidden_state.sum().backward()
        for n, p in enc.named_parameters():
            assert (p.grad is None) == (not p.requires_grad), n
    finally:
        os.environ.pop("HFASR_WHISPER_STRICT", None)
    enc = _encoder(_tiny_cfg(dropout=0.1))
    _strict()
    try:
        with pytest.raises(NotImplementedError, match="dropout"):
            enc(x)
    finally:
        os.environ.pop("HFASR_WHISPER_STRICT", None)
    from huggingface_asr_amd.whisper import _stock_forward
    _stock_forward.said.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        enc(x).last_hidden_state.sum().backward()
    assert any("dropout" in str(v.message) for v in w)
