"""Whisper-small encoder training step at 16 x 30 s on one GPU: forward + backward on the HIP path, transformers' own PyTorch forward / backward as the yardstick,
and one layer's attention backward — the fused kernel (ops_train.attn_bwd_fused) against the materialising attn_bwd_probs + bgemm path — at T' = 1500.

    python tools/whisper_train_bench.py [--batch 16] [--iters 5] [--out FILE.json]

Times are medians of `--iters` timed repetitions after two warm-ups, measured with CUDA events around the whole step."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from transformers import WhisperConfig
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd import bind, ops, ops_train as OT
    from huggingface_asr_amd import whisper as W
    bind.bind_all()
    dev = "cuda:0"
    B = a.batch
    res = dict(batch=B, shape="whisper-small encoder, 16 x 30 s" if B == 16 else f"whisper-small encoder, {B} x 30 s")

    # one layer's attention backward at T' = 1500, H = 12, hd = 64
    T, H, hd = 1500, 12, 64
    d = H * hd
    g = torch.Generator().manual_seed(0)
    qkv = (torch.randn(B * T, 3 * d, generator=g) * 0.5).to(dev, torch.bfloat16)
    dctx = torch.randn(B * T, d, generator=g).to(dev, torch.bfloat16)
    lse = torch.empty((B, H, T), device=dev, dtype=torch.float32)
    ctx = ops.attention_qkv(qkv, B, T, H, lse=lse)
    dq = torch.empty((B * T, 3 * d), device=dev, dtype=torch.bfloat16)
    res["attn_bwd_fused_ms"] = _time(lambda: OT.attn_bwd_fused(qkv, B, T, H, ctx, dctx, lse, dq), a.iters)
    res["attn_bwd_materialising_ms"] = _time(lambda: OT.attn_bwd_materialized(qkv, B, T, H, ctx, dctx, lse, dq), a.iters)
    res["attn_bwd_flop"] = 7 * 2 * B * H * T * T * hd          # the fused form's five products + the recomputed S and dP of the dQ walk
    res["attn_bwd_fused_tflops"] = res["attn_bwd_flop"] / res["attn_bwd_fused_ms"] / 1e9
    del qkv, dctx, ctx, dq, lse

    cfg = WhisperConfig(d_model=768, encoder_layers=12, encoder_attention_heads=12, encoder_ffn_dim=3072, num_mel_bins=80, max_source_positions=1500,
                        decoder_layers=1, decoder_attention_heads=12, decoder_ffn_dim=3072, vocab_size=100)
    torch.manual_seed(0)
    enc = MW.WhisperEncoder(cfg).to(dev).train()
    x = torch.randn(B, 80, 3000, device=dev)
    proj = torch.randn(B, 1500, 768, device=dev) / 100

    def hip_step():
        enc.zero_grad(set_to_none=True)
        (enc(x).last_hidden_state * proj).sum().backward()

    def ref_step():
        enc.zero_grad(set_to_none=True)
        (MW.WhisperEncoder._hfasr_reference_forward(enc, x).last_hidden_state * proj).sum().backward()

    for fused in (True, False):
        W.WhisperEncoderEngine.fused_attn_bwd = fused
        res["hip_step_ms_" + ("fused_attn_bwd" if fused else "materialising_attn_bwd")] = _time(hip_step, a.iters)
    W.WhisperEncoderEngine.fused_attn_bwd = False
    res["transformers_fp32_step_ms"] = _time(ref_step, a.iters)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        res["transformers_bf16_autocast_step_ms"] = _time(ref_step, a.iters)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
