"""GPU: Whisper decoding on the HIP path — the rows-streaming linear against fp64, the decoder token step (launch-per-op form 1 and streaming form 2) against
transformers' `WhisperDecoder`, the device-resident greedy loop against a host loop over the same step, tokens against transformers' fp32 greedy path, and
`hip_generate` on a `WhisperForConditionalGeneration`.

Weights: `synth.uniform` with one seed — matrices +-sqrt(3 / fan_in), embeddings and biases +-0.1, LayerNorm weights 1 +- 0.1.  A decoder of this distribution (d 384,
6 heads, 2 layers, V 1003, 150 encoder frames) gives logits of std ~1.1; transformers' own bf16-autocast gap on it is ~0.04 max / ~0.007 mean, while swapping the encoder
rows moves the logits by ~2.4 max / ~0.36 mean: cross-attention and cache errors are far above the tolerance."""
import functools
import os

import numpy as np
import pytest
import torch

from huggingface_asr_amd import ops, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20
BF16 = torch.bfloat16
TINY = dict(d_model=384, decoder_layers=2, decoder_attention_heads=6, decoder_ffn_dim=1536, vocab_size=1003, max_target_positions=64, activation_function="gelu",
            scale_embedding=False)
T_ENC = 150


def _fill(module, seed):
    """the module's state dict re-drawn from synth.uniform by the rule in the file's docstring"""
    sd = {}
    for k, v in module.state_dict().items():
        shape = tuple(v.shape)
        if "layer_norm" in k:
            t = synth.uniform(seed, k, shape, -0.1, 0.1) + (1.0 if k.endswith("weight") else 0.0)
        elif "embed_" in k or k.endswith("bias"):
            t = synth.uniform(seed, k, shape, -0.1, 0.1)
        else:
            a = float(np.sqrt(3.0 / int(np.prod(shape[1:]))))
            t = synth.uniform(seed, k, shape, -a, a)
        sd[k] = torch.from_numpy(t.astype(np.float32))
    module.load_state_dict(sd, strict=True)
    return sd


def _hf_decoder(cfg, seed=SEED, device=DEV):
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperDecoder
    c = WhisperConfig(d_model=cfg["d_model"], decoder_layers=cfg["decoder_layers"], decoder_attention_heads=cfg["decoder_attention_heads"],
                      decoder_ffn_dim=cfg["decoder_ffn_dim"], vocab_size=cfg["vocab_size"], max_target_positions=cfg["max_target_positions"], encoder_layers=1,
                      encoder_attention_heads=cfg["decoder_attention_heads"], encoder_ffn_dim=64, pad_token_id=0, bos_token_id=1, eos_token_id=2, decoder_start_token_id=1,
                      suppress_tokens=None, begin_suppress_tokens=None)
    dec = WhisperDecoder(c)
    sd = _fill(dec, seed)
    return dec.to(device).eval(), sd


def _ref_logits(dec, ids, enc, autocast=False):
    """transformers' decoder over the whole sequence (causal: position t sees ids[:, :t + 1]) + the tied head -> (B, U, V) fp32"""
    with torch.no_grad(), torch.autocast("cuda" if ids.is_cuda else "cpu", dtype=BF16, enabled=autocast):
        h = dec(input_ids=ids, encoder_hidden_states=enc, use_cache=False).last_hidden_state
        return torch.nn.functional.linear(h, dec.embed_tokens.weight).float()


def _engine(cfg, sd, form=None):
    from huggingface_asr_amd.whisper import WhisperDecoderEngine
    eng = WhisperDecoderEngine(cfg, DEV)
    eng.load_state_dict(sd)
    eng.step_form = form
    return eng


def _teacher_forced(eng, ids, enc, P, head_bias=None, first_bias=None):
    """the engine's logits for positions P - 1 ... U - 1 of `ids` (one step of P positions, then one token per step) -> ((B, U - P + 1, V), cache)"""
    B, U = ids.shape
    kvs = eng.cross_kv(enc.to(BF16).reshape(B * enc.shape[1], -1).contiguous())
    cache = eng.init_cache(B, U)
    out = [eng.step(ids[:, :P], cache, kvs, enc.shape[1], first_bias).clone()]
    for t in range(P, U):
        out.append(eng.step(ids[:, t:t + 1], cache, kvs, enc.shape[1], head_bias).clone())
    return torch.stack(out, 1), cache


def _ids(seed, B, U, V):
    return torch.from_numpy(synth.labels(seed, B, U, V, lo=0)).to(DEV)


def _enc(seed, B, T, d):
    return torch.from_numpy(synth.normal(seed, "enc_states", (B, T, d), 1.0)).to(DEV)


# ------------------------------------------------------------------------------------------------------------------ 1. the linear against fp64
LINEAR_CASES = [
    # M, N, K, epilogue
    (1, 384, 384, "bf16"),
    (9, 1152, 384, "cache"),
    (17, 1536, 384, "gelu"),
    (33, 384, 1536, "resid"),
    (64, 1003, 384, "f32"),
    (16, 3072, 768, "f32"),
    (16, 768, 3072, "f32"),
    (64, 1024, 4096, "f32"),
    (5, 1280, 5120, "f32"),
    (3, 70, 200, "f32"),          # N below one tile, K not a multiple of the 64-wide chunk
]


@pytest.mark.parametrize("M,N,K,epi", LINEAR_CASES)
def test_linear_rows_against_fp64(M, N, K, epi):
    """|err| <= K 2^-24 sum_k |x_k||w_k| (worst-case fp32 accumulation) + 2^-24 |y| (the bias add), + 2^-8 |y| for a bf16 output, + the documented 2.6e-5 of the erf-GELU fit, + one fp32 rounding
    of the residual add.  Two runs are bit-identical; permuting the rows permutes the output bit for bit."""
    name = f"lin{M}x{N}x{K}"
    x = torch.from_numpy(synth.normal(SEED, name + "/x", (M, K), 1.0)).to(DEV).to(BF16)
    a = float(np.sqrt(3.0 / K))
    w = torch.from_numpy(synth.uniform(SEED, name + "/w", (N, K), -a, a)).to(DEV).to(BF16)
    b = torch.from_numpy(synth.uniform(SEED, name + "/b", (N,), -0.1, 0.1)).to(DEV)
    xd, wd = x.double(), w.double()
    y = xd @ wd.T + b.double()
    bound = K * 2.0 ** -24 * (xd.abs() @ wd.abs().T)
    perm = torch.from_numpy(np.random.RandomState(M).permutation(M)).to(DEV)

    def run(xin):
        if epi == "f32":
            buf = torch.full((M, (N + 7) // 8 * 8 + 8), 7.0, device=DEV)            # a padded row stride; the pad must stay untouched
            ops.linear_rows(xin, w, b, out=buf[:, :N])
            assert bool((buf[:, N:] == 7.0).all())
            return buf[:, :N].clone(), None
        if epi == "resid":
            out = resid.clone()
            ops.linear_rows(xin, w, b, out=out, accumulate=True)
            return out, None
        if epi == "gelu":
            return ops.linear_rows(xin, w, b, act="gelu"), None
        if epi == "cache":
            d, U, past, Lmax = N // 3, 3, 3, 8
            kc = torch.full((M // U, Lmax, d), 5.0, device=DEV, dtype=BF16)
            vc = torch.full((M // U, Lmax, d), 6.0, device=DEV, dtype=BF16)
            out = ops.linear_rows(xin, w, b, kv_cache=(kc, vc), U=U, past=past)
            return out, (kc, vc)
        return ops.linear_rows(xin, w, b), None

    resid = torch.from_numpy(synth.normal(SEED, name + "/r", (M, N), 1.0)).to(DEV)
    got, kv = run(x)
    tol = bound + 2.0 ** -24 * y.abs()                 # + the one fp32 rounding of the bias add
    want = y
    if epi == "gelu":
        want = torch.nn.functional.gelu(y)
        tol = tol + 2.6e-5
    if epi == "resid":
        want = y + resid.double()
        tol = tol + 2.0 ** -24 * want.abs()
    if got.dtype == BF16:
        tol = tol + 2.0 ** -8 * want.abs()
    err = (got.double() - want).abs()
    print(f"linear_rows {M}x{N}x{K} {epi}: max err {float(err.max()):.3e}, max err / tol {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), (float((err / tol).max()), float(err.max()))
    if epi == "cache":
        kc, vc = kv
        d, U, past = N // 3, 3, 3
        assert torch.equal(kc[:, past:past + U].reshape(M, d), got[:, d:2 * d]) and torch.equal(vc[:, past:past + U].reshape(M, d), got[:, 2 * d:])
        keep = [i for i in range(8) if not past <= i < past + U]
        assert bool((kc[:, keep] == 5.0).all()) and bool((vc[:, keep] == 6.0).all())
    again, _ = run(x)
    assert torch.equal(got, again)
    if epi != "cache":                         # (the cache case ties rows to (sequence, position) pairs)
        if epi == "resid":
            resid = resid[perm].contiguous()
        shuffled, _ = run(x[perm].contiguous())
        assert torch.equal(shuffled, got[perm])


# ------------------------------------------------------------------------------------------------------------------ 2. / 3. step logits against transformers
def _check_step(cfg, B, T_enc, P, steps, forms, seed_tag):
    dec, sd = _hf_decoder(cfg)
    ids = _ids(SEED + B, B, P + steps, cfg["vocab_size"])
    enc = _enc(SEED + B, B, T_enc, cfg["d_model"])
    ref = _ref_logits(dec, ids, enc)[:, P - 1:]
    gap = (_ref_logits(dec, ids, enc, autocast=True)[:, P - 1:] - ref).abs()
    gap_max, gap_mean = float(gap.max()), float(gap.mean())
    caches = {}
    for form in forms:
        eng = _engine(cfg, sd, form)
        got, cache = _teacher_forced(eng, ids, enc, P)
        assert got.shape == ref.shape and bool(torch.isfinite(got).all())
        d = (got - ref).abs()
        print(f"{seed_tag} B={B} form {form}: max {float(d.max()):.4f} mean {float(d.mean()):.5f}; autocast gap max {gap_max:.4f} mean {gap_mean:.5f}; logits std {float(ref.std()):.3f}")
        assert float(d.max()) <= 2.0 * gap_max and float(d.mean()) <= 1.5 * gap_mean, (form, float(d.max()), float(d.mean()), gap_max, gap_mean)
        caches[form] = cache
    return caches


@pytest.mark.parametrize("B", [1, 5, 9, 33, 64])
def test_step_logits_teacher_forced_against_transformers(B):
    """Seeded random token ids (not a greedy path), 20 steps after a 3-token prompt, forms 1 and 2, against transformers' fp32 `WhisperDecoder` on the GPU:
    max <= 2.0 x and mean <= 1.5 x transformers' own bf16-autocast-vs-fp32 gap on the same inputs (the rule of test_whisper_small_real_shape_vs_transformers)."""
    caches = _check_step(TINY, B, T_ENC, 3, 20, (1, 2), "tiny")
    # the self-attention caches of the two forms: the same bf16 values up to last-bit flips.  Layer 0 projects identical inputs (embedding + LayerNorm, the same kernels),
    # so its K / V differ only by the order of the fp32 sums: one bf16 ulp (2^-7 relative) + the worst-case sum-order gap d 2^-24 sum|x||w| < 1e-4 where values are
    # near zero.  Deeper layers project inputs that already carry such flips (2^-8 |x_k w_k| ~ 2e-4 each): held to 2^-6 of the largest value.
    a, b = caches[1], caches[2]
    for t in ("k", "v"):
        k1, k2 = a[t][0].float(), b[t][0].float()
        assert bool(((k1 - k2).abs() <= 2.0 ** -7 * torch.maximum(k1.abs(), k2.abs()) + 1e-4).all())
        for l in range(1, TINY["decoder_layers"]):
            k1, k2 = a[t][l].float(), b[t][l].float()
            assert float((k1 - k2).abs().max()) <= 2.0 ** -6 * float(k1.abs().max())
            assert float(k1.abs().max()) > 0.5


@pytest.mark.parametrize("d,H,V,B", [(768, 12, 51865, 16), (1024, 16, 1003, 64)])
def test_step_logits_at_real_widths(d, H, V, B):
    """whisper-small / whisper-medium widths, 1500 encoder keys, 2 layers, six steps after a 3-token prompt: the same rule"""
    cfg = dict(d_model=d, decoder_layers=2, decoder_attention_heads=H, decoder_ffn_dim=4 * d, vocab_size=V, max_target_positions=16, activation_function="gelu",
               scale_embedding=False)
    _check_step(cfg, B, 1500, 3, 6, (1, 2), f"d{d}")


# ------------------------------------------------------------------------------------------------------------------ 4. the device loop equals the host loop
ENC_TINY = dict(d_model=384, encoder_layers=1, encoder_attention_heads=6, encoder_ffn_dim=768)
SUPPRESS, BEGIN_SUPPRESS = [3, 11, 500], [7, 1002]


@functools.lru_cache(maxsize=None)
def _tiny_pair():
    from transformers import WhisperConfig
    from transformers.models.whisper.modeling_whisper import WhisperEncoder
    from huggingface_asr_amd.whisper import WhisperEncoderEngine
    c = WhisperConfig(d_model=384, encoder_layers=1, encoder_attention_heads=6, encoder_ffn_dim=768, num_mel_bins=80, max_source_positions=T_ENC, decoder_layers=1,
                      decoder_attention_heads=6, decoder_ffn_dim=64, vocab_size=16)
    enc_sd = {k: torch.from_numpy(synth.init_param(SEED, "enc." + k, tuple(v.shape))) for k, v in WhisperEncoder(c).state_dict().items()}
    enc = WhisperEncoderEngine(ENC_TINY, DEV)
    enc.load_state_dict(enc_sd)
    dec, sd = _hf_decoder(TINY)
    return enc, dec, sd


def _host_greedy(enc_eng, eng, feats, prompt, max_new, eos, pad):
    """the loop `greedy_decode` runs, on the host over the engine's own step logits: mask -> torch.argmax -> append"""
    from huggingface_asr_amd.packing import suppression_vectors
    B, P = prompt.shape
    every, first = suppression_vectors(eng.cfg["vocab_size"], SUPPRESS, BEGIN_SUPPRESS, DEV)
    e = enc_eng.forward(input_features=feats)
    kvs = eng.cross_kv(ops.cast_bf16(e.reshape(-1, e.shape[2])))
    cache = eng.init_cache(B, P + max_new)
    ids, new = prompt.clone(), prompt
    done = torch.zeros(B, dtype=torch.bool, device=DEV)
    for n in range(max_new):
        logits = eng.step(new, cache, kvs, e.shape[1]) + (first if n == 0 else every)
        tok = torch.where(done, torch.full_like(done, pad, dtype=torch.long), torch.argmax(logits, -1))
        ids = torch.cat([ids, tok[:, None]], 1)
        done = done | (tok == eos)
        new = tok[:, None]
        if bool(done.all()):
            break
    return ids


POOL = 64


@pytest.mark.parametrize("B,form", [(5, 1), (5, 2), (33, 2)])
def test_device_greedy_loop_equals_the_host_loop(B, form):
    """Token ids exactly equal.  EOS is a token of row 0's free-running path, so rows stop at different steps, take pads, and the loop ends before max_new_tokens;
    stats["steps"] shows the early exit.  Greedy paths of a random decoder share few tokens, so the rows are drawn from a pool of 64 free-running candidates: the EOS is
    the token of row 0's path that most candidates reach, the batch is row 0 and the other candidates that reach it (repeated where fewer than B do)."""
    from huggingface_asr_amd.whisper import greedy_decode
    enc_eng, _, sd = _tiny_pair()
    eng = _engine(TINY, sd, form)
    V, max_new, pad = TINY["vocab_size"], 40, 0
    pool_feats = torch.from_numpy(synth.normal(SEED, "greedy_feats", (POOL, 80, 2 * T_ENC), 0.5)).to(DEV)
    pool_prompt = _ids(SEED + 1, POOL, 2, V)
    free = _host_greedy(enc_eng, _engine(TINY, sd, 2), pool_feats, pool_prompt, 30, SUPPRESS[0], pad)[:, 2:]        # a suppressed id as EOS: never emitted, every row runs on
    rows = [r.tolist() for r in free.cpu()]
    cands = [t for t in dict.fromkeys(rows[0]) if t != pad]
    eos = max(cands, key=lambda t: (len({r.index(t) for r in rows if t in r}), sum(t in r for r in rows), -rows[0].index(t)))
    reach = [i for i, r in enumerate(rows) if eos in r]
    pick = torch.tensor([reach[i % len(reach)] for i in range(B)], device=DEV)
    feats, prompt = pool_feats[pick].contiguous(), pool_prompt[pick].contiguous()
    want = _host_greedy(enc_eng, eng, feats, prompt, max_new, eos, pad)
    firsts = [r.index(eos) if eos in r else None for r in want[:, 2:].tolist()]
    print(f"B={B} form {form}: eos {eos}, {len(reach)} of {POOL} candidates reach it, first positions {firsts}")
    assert all(f is not None for f in firsts) and len(set(firsts)) > 1 and max(firsts) + 1 < max_new, (eos, firsts)
    stats = {}
    got = greedy_decode(enc_eng, eng, feats, prompt, max_new_tokens=max_new, eos_token_id=eos, pad_token_id=pad, suppress_tokens=SUPPRESS,
                        begin_suppress_tokens=BEGIN_SUPPRESS, stats=stats)
    assert got.dtype == torch.long and got.is_cuda
    assert got.shape == want.shape and torch.equal(got, want), (got.tolist(), want.tolist())
    assert got.shape[1] == 2 + max(firsts) + 1
    assert max(firsts) + 1 <= stats["steps"] <= max(firsts) + 1 + 2 < max_new, stats            # at most run_ahead = 2 steps past the last EOS
    for r, f in zip(got[:, 2:].tolist(), firsts):
        assert r[f] == eos and all(t == pad for t in r[f + 1:]) and eos not in r[:f]
    assert not (set(got[:, 2:].reshape(-1).tolist()) & set(SUPPRESS)) and not (set(got[:, 2].tolist()) & set(BEGIN_SUPPRESS))
    with pytest.raises(ValueError):
        greedy_decode(enc_eng, eng, feats, prompt, max_new_tokens=TINY["max_target_positions"], eos_token_id=eos, pad_token_id=pad)
    with pytest.raises(RuntimeError):
        greedy_decode(enc_eng, eng, feats.cpu(), prompt, max_new_tokens=4, eos_token_id=eos, pad_token_id=pad)


# ------------------------------------------------------------------------------------------------------------------ 5. tokens against transformers
def reference_greedy(dec, enc, prompt, steps, every, first):
    """transformers' fp32 greedy path: the explicit loop over the un-patched decoder with the two masks -> (ids (B, P + steps), top-2 margins (B, steps))"""
    ids, margins = prompt, []
    for n in range(steps):
        logits = _ref_logits(dec, ids, enc)[:, -1] + (first if n == 0 else every)
        top = logits.topk(2, -1)
        margins.append(top.values[:, 0] - top.values[:, 1])
        ids = torch.cat([ids, top.indices[:, :1]], 1)
    return ids, torch.stack(margins, 1)


def test_tokens_against_transformers_greedy_path():
    """At every position the HIP arg-max for the reference's prefix equals the reference's token wherever the reference's top-2 margin is >= 2 x gap_max (its own
    bf16-autocast gap); at most 15 % of the positions may fall under that margin."""
    from huggingface_asr_amd.packing import suppression_vectors
    _, dec, sd = _tiny_pair()
    B, P, steps, V = 5, 2, 24, TINY["vocab_size"]
    enc = _enc(105, B, T_ENC, TINY["d_model"])        # input seed checked on the CPU: the reference alone leaves 6 of 120 positions (5 %) under the margin, five distinct rows
    prompt = _ids(106, B, P, V)
    every, first = suppression_vectors(V, SUPPRESS, BEGIN_SUPPRESS, DEV)
    ids, margins = reference_greedy(dec, enc, prompt, steps, every, first)
    tf = ids[:, :-1]                                                              # the inputs of the 24 predictions
    gap_max = float((_ref_logits(dec, tf, enc, autocast=True) - _ref_logits(dec, tf, enc))[:, P - 1:].abs().max())
    decisive = margins >= 2.0 * gap_max
    share = 1.0 - float(decisive.float().mean())
    print(f"gap_max {gap_max:.4f}; positions under the margin: {int((~decisive).sum())} of {decisive.numel()} ({100 * share:.1f} %); distinct tokens {len(set(ids[:, P:].reshape(-1).tolist()))}")
    assert share <= 0.15, share
    for form in (1, 2):
        got, _ = _teacher_forced(_engine(TINY, sd, form), tf, enc, P, every, first)
        tok = torch.argmax(got, -1)
        bad = decisive & (tok != ids[:, P:])
        assert not bool(bad.any()), (form, bad.nonzero().tolist())
        print(f"form {form}: {int((tok == ids[:, P:]).sum())} of {tok.numel()} tokens equal")


# ------------------------------------------------------------------------------------------------------------------ 6. hip_generate
def test_hip_generate_on_a_transformers_model():
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    from transformers.generation.utils import GenerationMixin
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd import bind
    from huggingface_asr_amd.whisper import WhisperDecoderEngine, WhisperEncoderEngine, greedy_decode, hip_generate
    bind.bind_all()
    os.environ["HFASR_WHISPER_STRICT"] = "1"
    try:
        cfg = WhisperConfig(d_model=128, encoder_layers=2, decoder_layers=2, encoder_attention_heads=2, decoder_attention_heads=2, encoder_ffn_dim=256, decoder_ffn_dim=512,
                            num_mel_bins=80, max_source_positions=100, max_target_positions=40, vocab_size=120, pad_token_id=0, bos_token_id=1, eos_token_id=2,
                            decoder_start_token_id=1, suppress_tokens=None, begin_suppress_tokens=None)
        torch.manual_seed(0)
        model = WhisperForConditionalGeneration(cfg)
        _fill(model.model.decoder, SEED)
        model = model.to(DEV).eval()
        gc = model.generation_config
        gc.eos_token_id, gc.pad_token_id, gc.decoder_start_token_id = 2, 0, 1
        gc.suppress_tokens, gc.begin_suppress_tokens = [5, 17], [2, 9]
        x = torch.from_numpy(synth.normal(SEED, "gen_feats", (3, 80, 200), 0.5)).to(DEV)
        out = hip_generate(model, x, max_new_tokens=12)
        assert out.dtype == torch.long and out.shape[0] == 3 and 2 <= out.shape[1] <= 13 and bool((out[:, 0] == 1).all())
        enc_eng = WhisperEncoderEngine(dict(d_model=128, encoder_layers=2, encoder_attention_heads=2, encoder_ffn_dim=256), DEV)
        enc_eng.load_state_dict(model.model.encoder.state_dict())
        dcfg = dict(d_model=128, decoder_layers=2, decoder_attention_heads=2, decoder_ffn_dim=512, vocab_size=120, max_target_positions=40)
        dec_eng = WhisperDecoderEngine(dcfg, DEV)
        dec_eng.load_state_dict(model.model.decoder.state_dict())
        start = torch.full((3, 1), 1, dtype=torch.long, device=DEV)
        want = greedy_decode(enc_eng, dec_eng, x, start, max_new_tokens=12, eos_token_id=2, pad_token_id=0, suppress_tokens=[5, 17], begin_suppress_tokens=[2, 9])
        assert torch.equal(out, want), (out.tolist(), want.tolist())
        gen = out[:, 1:]
        assert not (set(gen.reshape(-1).tolist()) & {5, 17}) and not (set(gen[:, 0].tolist()) & {2, 9})
        # a prompt, max_length instead of max_new_tokens
        prompt = torch.tensor([[1, 40, 41]] * 3, device=DEV)
        out2 = hip_generate(model, x, decoder_input_ids=prompt, max_length=9, num_beams=1, do_sample=False)
        assert out2.shape[1] <= 9 and torch.equal(out2[:, :3], prompt)
        assert torch.equal(out2, greedy_decode(enc_eng, dec_eng, x, prompt, max_new_tokens=6, eos_token_id=2, pad_token_id=0, suppress_tokens=[5, 17], begin_suppress_tokens=[2, 9]))
        # the engine is cached per decoder module and follows the weights
        eng0 = model.model.decoder.__dict__["_hfasr_engine"][1]
        hip_generate(model, x, max_new_tokens=4)
        assert model.model.decoder.__dict__["_hfasr_engine"][1] is eng0
        with torch.no_grad():
            model.model.decoder.embed_tokens.weight.mul_(-1.0)
        out3 = hip_generate(model, x, max_new_tokens=12)
        assert model.model.decoder.__dict__["_hfasr_engine"][1] is not eng0
        assert out3.shape != out.shape or not torch.equal(out3, out)
        with pytest.raises(RuntimeError):
            hip_generate(model, x.cpu(), max_new_tokens=4)
        # model.generate is still transformers': only WhisperEncoder.forward is bound
        assert getattr(MW.WhisperEncoder.forward, "_hfasr_hip", False)
        assert MW.WhisperDecoder.forward.__module__.startswith("transformers.") and MW.WhisperDecoderLayer.forward.__module__.startswith("transformers.")
        assert WhisperForConditionalGeneration.generate.__module__.startswith("transformers.") and GenerationMixin.generate.__module__.startswith("transformers.")
        assert not hasattr(MW.WhisperDecoder, "_hfasr_reference_forward") and "generate" not in model.__dict__
    finally:
        os.environ.pop("HFASR_WHISPER_STRICT", None)
