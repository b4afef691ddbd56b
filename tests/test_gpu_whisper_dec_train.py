"""GPU: Whisper decoder training on the HIP path — the tied head's cross-entropy out of the GEMM's epilogue (no logits), the teacher-forced decoder's
forward / backward against transformers' own autograd, and `WhisperForConditionalGeneration` training with `install_whisper(decoder=True, fused_loss=True)`
under HFASR_WHISPER_STRICT=1.

Gradient bounds (`_close`, REL, COS): those of tests/test_gpu_whisper_train.py, whose docstring gives the rationale (bf16 operands, fp32 sums).  The fused head against
the materialising kernels on the same logits differs only in the order of the row sums and in `exp(x - lse)` against `exp(x - max) / sum`: the "vs materialising"
numbers of the attention test (rel 1e-2, cos 0.9999; the bf16 rounding of the output, 2^-9 per element, is the floor of both)."""
import math
import os
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REL, COS = 2e-2, 0.999
BF16 = torch.bfloat16


def _close(g, r, rel=REL, cos=COS, what=""):
    g, r = g.double().flatten(), r.double().flatten()
    e = float((g - r).norm() / r.norm().clamp_min(1e-30))
    c = float(torch.dot(g, r) / (g.norm() * r.norm()).clamp_min(1e-30))
    assert e <= rel and c >= cos, (what, e, c)


def _strict():
    os.environ["HFASR_WHISPER_STRICT"] = "1"


# ------------------------------------------------------------------------------------------------------------------------------ 1. the fused head
def _head_case(M, N, K, seed, ignore="some"):
    gen = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=gen) * 0.5).to(DEV, BF16)
    w = (torch.randn(N, K, generator=gen) * 0.3).to(DEV, BF16)
    lab = torch.randint(0, N, (M,), generator=gen)
    lab[0], lab[1] = 0, N - 1
    if ignore == "some":
        lab[2::5] = -100
        lab[M - 1] = -100
    elif ignore == "all":
        lab[:] = -100
    return a, w, lab.to(DEV)


def _ulp(x):
    return torch.exp2(torch.floor(torch.log2(x.abs().double().clamp_min(1e-30))) - 23)


HEAD_SHAPES = [(7, 100, 128, None), (300, 257, 128, None), (300, 5001, 256, None), (300, 5001, 256, 5056), (260, 51865, 128, None)]


@pytest.mark.parametrize("M,N,K,ldo", HEAD_SHAPES)
def test_fused_head_matches_materialising_path_and_fp64(M, N, K, ldo):
    from huggingface_asr_amd import ops, ops_train as OT
    a, w, lab = _head_case(M, N, K, seed=M + N)
    ldo = (N + 7) // 8 * 8 if ldo is None else ldo
    valid = lab >= 0
    acc, lse, nll, tgt = ops.gemm_ce(a, w, lab, return_target=True)
    # the fp32 logits of the same kernel body (the LSE form of the head GEMM) and their row log-sum-exp
    buf = torch.empty((M, (N + 3) // 4 * 4), device=DEV, dtype=torch.float32)
    lse_ref = ops.gemm_lse(a, w, None, buf)
    logits = buf[:, :N]
    torch.cuda.synchronize()
    want_t = logits.gather(1, lab.clamp_min(0)[:, None])[:, 0]
    assert torch.equal(tgt[valid], want_t[valid])                                  # bit for bit: same kernel body, same K order
    assert bool(((lse.double() - lse_ref.double()).abs() <= 8 * _ulp(lse_ref)).all())
    assert torch.equal(nll[~valid], torch.zeros_like(nll[~valid]))
    assert torch.equal(nll[valid], (lse - tgt)[valid])
    assert float(acc[1]) == float(valid.sum())
    l64 = logits.double()
    ce64 = (torch.logsumexp(l64, 1) - l64.gather(1, lab.clamp_min(0)[:, None])[:, 0])[valid].mean()
    loss = float(acc[0] / acc[1])
    print(f"loss {loss:.8f} fp64 {float(ce64):.8f} rel {abs(loss - float(ce64)) / float(ce64):.2e}")
    assert abs(loss - float(ce64)) <= 1e-5 * float(ce64)
    acc2, lse2, nll2 = ops.gemm_ce(a, w, lab)
    assert torch.equal(acc, acc2) and torch.equal(lse, lse2) and torch.equal(nll, nll2)
    # ---- backward
    gscale = 0.7
    g = torch.where(valid, gscale / acc[1], torch.zeros((), device=DEV))
    dl = OT.gemm_ce_bwd(a, w, lab, lse, g, ldo)
    assert dl.shape == (M, ldo) and dl.dtype == BF16
    import huggingface_asr_amd._lib as _lib
    pre = torch.full((M, ldo), 7.0, device=DEV, dtype=BF16)
    rc = _lib.lib().mi_gemm_ce_bwd_bf16(a.data_ptr(), a.stride(0), w.data_ptr(), w.stride(0), None, lab.data_ptr(), lse.data_ptr(), g.data_ptr(), pre.data_ptr(), ldo, M, N, K,
                                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(dl, pre)                                                    # every element written, bit-identical runs
    assert float(dl[:, N:].float().abs().sum()) == 0.0                             # the padding columns
    assert float(dl[~valid].float().abs().sum()) == 0.0                            # ignored rows
    accm = ops.ce_label_smoothing(logits.view(1, M, N), lab.view(1, M), shift=0, eps=0.0, return_acc=True)
    dm = OT.ce_label_smoothing_bwd(logits.view(1, M, N), lab.view(1, M), accm, shift=0, eps=0.0, weight=gscale, ldo=ldo)
    _close(dl.float(), dm.float(), rel=1e-2, cos=0.9999, what="vs materialising")
    oh = torch.zeros_like(l64).scatter_(1, lab.clamp_min(0)[:, None], 1.0)
    d64 = (torch.softmax(l64, 1) - oh) * g.double()[:, None]
    _close(dl[:, :N].float(), d64, what="vs fp64")


@pytest.mark.parametrize("M,N,K", [(7, 100, 128), (300, 257, 128)])
def test_fused_head_all_rows_ignored(M, N, K):
    from huggingface_asr_amd import ops, ops_train as OT
    a, w, lab = _head_case(M, N, K, seed=5, ignore="all")
    acc, lse, nll = ops.gemm_ce(a, w, lab)
    assert float(acc[0]) == 0.0 and float(acc[1]) == 0.0 and math.isnan(float(acc[0] / acc[1]))
    assert float(nll.abs().sum()) == 0.0 and bool(torch.isfinite(lse).all())
    g = torch.where(lab >= 0, 1.0 / acc[1], torch.zeros((), device=DEV))
    dl = OT.gemm_ce_bwd(a, w, lab, lse, g)
    assert float(dl.float().abs().sum()) == 0.0


def test_fused_head_unsupported_shape_falls_back():
    """K = 64 is outside the 256 x 256 kernel: the C entries say so, the ops give the materialising path's result under the same contract"""
    import huggingface_asr_amd._lib as _lib
    from huggingface_asr_amd import ops, ops_train as OT
    M, N, K = 37, 257, 64
    a, w, lab = _head_case(M, N, K, seed=9)
    valid = lab >= 0
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    f = lambda n: torch.empty((n,), device=DEV, dtype=torch.float32)
    acc, lse, nll, tgt, ws = f(2), f(M), f(M), f(M), f(int(L.mi_gemm_lse_workspace_floats(M, N)))
    assert L.mi_gemm_ce_f32(a.data_ptr(), K, w.data_ptr(), K, None, lab.data_ptr(), acc.data_ptr(), lse.data_ptr(), nll.data_ptr(), tgt.data_ptr(), ws.data_ptr(),
                            M, N, K, st) == _lib.ERR_UNSUPPORTED
    ldo = (N + 7) // 8 * 8
    out = torch.empty((M, ldo), device=DEV, dtype=BF16)
    g = torch.zeros((M,), device=DEV)
    assert L.mi_gemm_ce_bwd_bf16(a.data_ptr(), K, w.data_ptr(), K, None, lab.data_ptr(), lse.data_ptr(), g.data_ptr(), out.data_ptr(), ldo, M, N, K, st) == _lib.ERR_UNSUPPORTED
    acc, lse, nll = ops.gemm_ce(a, w, lab)
    l64 = ops.gemm(a, w, out_dtype=torch.float32).double()
    n64 = torch.logsumexp(l64, 1) - l64.gather(1, lab.clamp_min(0)[:, None])[:, 0]
    assert float(acc[1]) == float(valid.sum())
    assert abs(float(acc[0] / acc[1]) - float(n64[valid].mean())) <= 1e-5 * float(n64[valid].mean())
    assert float(nll[~valid].abs().sum()) == 0.0
    assert float((nll.double() - n64)[valid].abs().max()) <= 1e-4
    assert float((lse.double() - torch.logsumexp(l64, 1)).abs().max()) <= 1e-5
    g = torch.where(valid, 0.7 / acc[1], torch.zeros((), device=DEV))
    dl = OT.gemm_ce_bwd(a, w, lab, lse, g, ldo)
    assert dl.shape == (M, ldo) and float(dl[:, N:].float().abs().sum()) == 0.0 and float(dl[~valid].float().abs().sum()) == 0.0
    oh = torch.zeros_like(l64).scatter_(1, lab.clamp_min(0)[:, None], 1.0)
    _close(dl[:, :N].float(), (torch.softmax(l64, 1) - oh) * g.double()[:, None], what="fallback vs fp64")


# ------------------------------------------------------------------------------------------------------------------------------ 3. / 4. the decoder
def _tiny_cfg(**kw):
    from transformers import WhisperConfig
    c = dict(d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=512,
             num_mel_bins=80, max_source_positions=64, max_target_positions=64, vocab_size=100, pad_token_id=0, bos_token_id=1, eos_token_id=2,
             decoder_start_token_id=1, suppress_tokens=None, begin_suppress_tokens=None)
    c.update(kw)
    return WhisperConfig(**c)


class _installed:
    """`install_whisper(...)` for the body; the stock forwards of the decoder and the language-model class are back afterwards, so later tests see today's binding"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from huggingface_asr_amd import bind
        from huggingface_asr_amd.whisper import install_whisper
        bind.bind_all()
        install_whisper(**self.kw)
        _strict()

    def __exit__(self, *exc):
        from transformers.models.whisper import modeling_whisper as MW
        os.environ.pop("HFASR_WHISPER_STRICT", None)
        for cls in (MW.WhisperDecoder, MW.WhisperForConditionalGeneration):
            if getattr(cls.forward, "_hfasr_hip", False):
                cls.forward = cls._hfasr_reference_forward
            if "_hfasr_reference_forward" in cls.__dict__:           # the un-opted binding has no such attribute on these two classes, and a later test says so
                del cls._hfasr_reference_forward
        return False


def _decoder(cfg, seed=0):
    from transformers.models.whisper.modeling_whisper import WhisperDecoder
    torch.manual_seed(seed)
    dec = WhisperDecoder(cfg)
    with torch.no_grad():                                          # non-trivial LayerNorms
        for n, p in dec.named_parameters():
            if "layer_norm" in n:
                p.add_(0.1 * torch.randn_like(p))
    dec.embed_positions.weight.requires_grad_(True)                # unfrozen so that its gradient is checked too
    return dec.to(DEV).train()


def _dec_grads(dec, ids, enc, proj, hip):
    from transformers.models.whisper import modeling_whisper as MW
    dec.zero_grad(set_to_none=True)
    enc = enc.clone().requires_grad_(True)
    fwd = dec.forward if hip else (lambda **kw: MW.WhisperDecoder._hfasr_reference_forward(dec, **kw))
    out = fwd(input_ids=ids, encoder_hidden_states=enc, use_cache=None if hip else False).last_hidden_state
    (out * proj).sum().backward()
    return {n: p.grad.clone() if p.grad is not None else None for n, p in dec.named_parameters()}, enc.grad.clone(), out.detach()


@pytest.mark.parametrize("B,U", [(2, 1), (2, 6), (2, 37)])
def test_decoder_gradients_match_transformers(B, U):
    with _installed(decoder=True):
        cfg = _tiny_cfg()
        dec = _decoder(cfg)
        g = torch.Generator().manual_seed(1)
        ids = torch.randint(0, 100, (B, U), generator=g).to(DEV)
        enc = torch.randn(B, 64, 128, generator=g).to(DEV)
        proj = torch.randn(B, U, 128, generator=g).to(DEV)
        gh, eh, oh = _dec_grads(dec, ids, enc, proj, True)
        gr, er, orf = _dec_grads(dec, ids, enc, proj, False)
        _close(oh, orf, what="last_hidden_state")
        scale = float(gr["layers.0.self_attn.v_proj.weight"].norm())
        for n in gr:
            assert (gh[n] is None) == (gr[n] is None), n
            if gr[n] is not None:
                assert gh[n].shape == gr[n].shape and gh[n].dtype == gr[n].dtype
                if float(gr[n].norm()) <= 1e-6 * scale:
                    # U = 1: a soft-max over one key has no gradient, so the self-attention's q / k gradients are zero in exact arithmetic.  The HIP backward forms
                    # dS = P (dP - delta) from two fp32 sums of the same 64 products in different orders (relative 64 * 2^-24 ~ 4e-6 of the products that make up the
                    # v gradient): noise far below 1e-3 of that gradient, where a wrong term would be O(1) of it.
                    assert float(gh[n].double().norm()) <= 1e-3 * scale, (n, float(gh[n].norm()), scale)
                else:
                    _close(gh[n], gr[n], what=n)
        assert gh["layers.0.encoder_attn.k_proj.weight"] is not None and gh["embed_positions.weight"] is not None
        _close(eh, er, what="encoder_hidden_states")
        gh2, eh2, oh2 = _dec_grads(dec, ids, enc, proj, True)       # an identical step gives bit-identical results
        assert torch.equal(oh, oh2) and torch.equal(eh, eh2) and all(torch.equal(gh[n], gh2[n]) for n in gh if gh[n] is not None)


def test_decoder_frozen_parameters_and_layerdrop():
    with _installed(decoder=True):
        dec = _decoder(_tiny_cfg())
        for n, p in dec.named_parameters():
            if n.startswith("embed") or n.startswith("layers.0.encoder_attn") or n == "layers.1.fc1.weight":
                p.requires_grad_(False)
        g = torch.Generator().manual_seed(4)
        ids = torch.randint(0, 100, (2, 6), generator=g).to(DEV)
        enc = torch.randn(2, 64, 128, generator=g).to(DEV)
        dec(input_ids=ids, encoder_hidden_states=enc).last_hidden_state.sum().backward()
        for n, p in dec.named_parameters():
            assert (p.grad is None) == (not p.requires_grad), n
        # LayerDrop: the same draws as the stock forward, so the same layers are skipped
        dec = _decoder(_tiny_cfg(decoder_layers=6, decoder_layerdrop=0.5))
        proj = torch.randn(2, 6, 128, generator=g).to(DEV)
        torch.manual_seed(11)
        gh, _, oh = _dec_grads(dec, ids, enc, proj, True)
        torch.manual_seed(11)
        gr, _, orf = _dec_grads(dec, ids, enc, proj, False)
        _close(oh, orf, what="out")
        skipped = {l for l in range(6) if gr[f"layers.{l}.fc1.weight"] is None}
        assert skipped and len(skipped) < 6, skipped
        for l in range(6):
            assert (gh[f"layers.{l}.fc1.weight"] is None) == (l in skipped), l


def test_decoder_real_widths_one_step():
    with _installed(decoder=True):
        cfg = _tiny_cfg(d_model=768, decoder_layers=2, decoder_attention_heads=12, decoder_ffn_dim=3072, vocab_size=51865, max_source_positions=1500,
                        max_target_positions=448)
        dec = _decoder(cfg)
        g = torch.Generator().manual_seed(2)
        ids = torch.randint(0, 51865, (2, 40), generator=g).to(DEV)
        enc = torch.randn(2, 1500, 768, generator=g).to(DEV)
        proj = torch.randn(2, 40, 768, generator=g).to(DEV) / 100
        gh, eh, _ = _dec_grads(dec, ids, enc, proj, True)
        gr, er, _ = _dec_grads(dec, ids, enc, proj, False)
        for n in ("embed_tokens.weight", "embed_positions.weight", "layers.0.self_attn.q_proj.weight", "layers.0.encoder_attn.k_proj.weight", "layers.0.fc1.weight",
                  "layers.1.encoder_attn.v_proj.bias", "layers.1.fc2.weight", "layer_norm.weight"):
            _close(gh[n], gr[n], rel=3e-2, cos=0.999, what=n)
        _close(eh, er, rel=3e-2, cos=0.999, what="encoder_hidden_states")


# ------------------------------------------------------------------------------------------------------------------------------ 5. the whole model
def test_conditional_generation_trains_with_the_fused_loss():
    from transformers import WhisperForConditionalGeneration
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd.whisper import _stock_decoder_forward
    cfg = _tiny_cfg()
    torch.manual_seed(0)
    hip = WhisperForConditionalGeneration(cfg).to(DEV).train()
    ref = WhisperForConditionalGeneration(cfg).to(DEV).train()
    ref.load_state_dict(hip.state_dict())
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 80, 128, generator=g).to(DEV)
    labels = torch.randint(3, 100, (2, 6), generator=g)
    labels[1, 4:] = -100
    labels = labels.to(DEV)
    from huggingface_asr_amd import bind
    bind.bind_all()
    gen = WhisperForConditionalGeneration(cfg).to(DEV).eval()      # generate (the cached route) before the opt-in ...
    gen.load_state_dict(hip.state_dict())
    tok_before = gen.generate(input_features=x, max_new_tokens=4, do_sample=False, num_beams=1)
    oh = torch.optim.AdamW(hip.parameters(), lr=1e-3)
    orf = torch.optim.AdamW(ref.parameters(), lr=1e-3)
    stock = {c: c.forward for c in (MW.WhisperEncoder, MW.WhisperDecoder, MW.WhisperForConditionalGeneration)}
    losses = []
    with _installed(decoder=True, fused_loss=True):
        ours = {c: c.forward for c in stock}
        assert ours[MW.WhisperDecoder] is not stock[MW.WhisperDecoder] and ours[MW.WhisperForConditionalGeneration] is not stock[MW.WhisperForConditionalGeneration]
        for step in range(3):
            oh.zero_grad(); orf.zero_grad()
            out = hip(input_features=x, labels=labels)
            assert out.logits is None
            out.loss.backward()
            for c in stock:                                          # the stock twin: transformers' own encoder, decoder and loss
                c.forward = c._hfasr_reference_forward
            try:
                lr = ref(input_features=x, labels=labels).loss
                lr.backward()
            finally:
                for c in stock:
                    c.forward = ours[c]
            if step == 0:
                ph, pr = dict(hip.named_parameters()), dict(ref.named_parameters())
                for n in ph:
                    if n == "model.decoder.embed_tokens.weight" or n.startswith("model.decoder.layers.1.") or n.startswith("model.encoder.layers.0."):
                        assert (ph[n].grad is None) == (pr[n].grad is None), n
                        if pr[n].grad is not None and float(pr[n].grad.norm()) > 0:
                            _close(ph[n].grad, pr[n].grad, what=n)
            losses.append((float(out.loss), float(lr)))
            oh.step(); orf.step()
        # eval: logits come back, equal to the stock head's on the same hidden states
        hip.eval()
        with torch.no_grad():
            ev = hip(input_features=x, labels=labels)
            hid = hip.model(x, decoder_input_ids=MW.shift_tokens_right(labels, cfg.pad_token_id, cfg.decoder_start_token_id)).last_hidden_state
            enc_h = hip.model.encoder(x).last_hidden_state
        assert ev.logits is not None and torch.equal(ev.logits, hip.proj_out(hid))
        tok_after = gen.generate(input_features=x, max_new_tokens=4, do_sample=False, num_beams=1)      # ... and under it, silently, STRICT or not
        assert torch.equal(tok_before, tok_after)
        hip.train()
        # dropout in training (the encoder states handed in, so that the decoder is the one asked): refused under STRICT, said once without it
        cfg.dropout = 0.1
        try:
            with pytest.raises(NotImplementedError, match="Whisper decoder.*dropout"):
                hip(encoder_outputs=(enc_h,), labels=labels)
            os.environ.pop("HFASR_WHISPER_STRICT", None)
            _stock_decoder_forward.said.clear()
            from huggingface_asr_amd.whisper import _stock_forward
            _stock_forward.said.clear()
            with warnings.catch_warnings(record=True) as wlist:
                warnings.simplefilter("always")
                o1 = hip(encoder_outputs=(enc_h,), labels=labels)
                hip(encoder_outputs=(enc_h,), labels=labels)
            assert o1.logits is not None and bool(torch.isfinite(o1.loss))
            assert sum("WhisperDecoder.forward" in str(v.message) and "dropout" in str(v.message) for v in wlist) == 1
        finally:
            cfg.dropout = 0.0
            _strict()
    for a, b in losses:
        assert abs(a - b) <= 2e-2 * abs(b), losses
