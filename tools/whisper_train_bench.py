#!/usr/bin/env python
"""ms per training step (forward + backward + AdamW) of a Whisper-small sized `WhisperForConditionalGeneration`, 16 clips of 30 s, for the three bindings of
`whisper.install_whisper`, alternated in ONE process on the same model:

    a  encoder        the HIP encoder; decoder, proj_out and CrossEntropyLoss in PyTorch (what `bind_all()` installs without a switch)
    b  decoder        + `install_whisper(decoder=True)`: the teacher-forced decoder pass on the HIP engine
    c  fused_loss     + `install_whisper(fused_loss=True)`: the loss out of the tied head's GEMM (`ops.gemm_ce` / `ops_train.gemm_ce_bwd`), no logits

    python tools/whisper_train_bench.py [--reps 5] [--warmup 2] [--labels 128 448] [--out FILE.txt]

Labels 16 x 128 and 16 x 448 (the recipe's maximum), every position valid.  Reported per route: the median over the repetitions and the run-to-run spread
(max - min); a route beats its predecessor when the medians differ by more than the larger of the two spreads.  The engines are rebuilt when a parameter changed, i.e.
after every optimiser step: the step time includes that repacking, and the tool times it on its own as well.  Then the head alone at M = 16 x 448 rows: the fused pair
against the library's materialising route (fp32 `ops.gemm` + `ce_label_smoothing` + `ce_label_smoothing_bwd`), with the logit bytes the fused pair does not move.
One JSON line per measurement, then a table.

    python tools/whisper_train_bench.py --encoder [--batch 16] [--iters 5] [--out FILE.json]

The encoder alone (DESIGN "Whisper encoder training"): its forward + backward on the HIP path against transformers' own PyTorch forward / backward, and one layer's attention
backward — the fused kernel (ops_train.attn_bwd_fused) against the materialising attn_bwd_probs + bgemm path — at T' = 1500; medians of `--iters` timed repetitions after
two warm-ups, device events around the whole step, one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
B, V, D, LAYERS, HEADS = 16, 51865, 768, 12, 12


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def med_spread(v):
    return statistics.median(v), max(v) - min(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--labels", type=int, nargs="+", default=[128, 448])
    ap.add_argument("--encoder", action="store_true", help="the encoder alone and one layer's attention backward (see above); takes --batch / --iters")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    (encoder_main if a.encoder else step_main)(a)


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


def encoder_main(a):
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


def step_main(a):
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    from transformers.models.whisper import modeling_whisper as MW

    from huggingface_asr_amd import ops, ops_train as OT, whisper as W
    W.install_whisper(decoder=True, fused_loss=True)
    classes = (MW.WhisperDecoder, MW.WhisperForConditionalGeneration)
    hip = {c: c.forward for c in classes}
    stock = {c: c._hfasr_reference_forward for c in classes}
    routes = {"a_encoder": {c: stock[c] for c in classes}, "b_decoder": {MW.WhisperDecoder: hip[MW.WhisperDecoder], MW.WhisperForConditionalGeneration: stock[MW.WhisperForConditionalGeneration]},
              "c_fused_loss": hip}
    cfg = WhisperConfig(d_model=D, encoder_layers=LAYERS, decoder_layers=LAYERS, encoder_attention_heads=HEADS, decoder_attention_heads=HEADS, encoder_ffn_dim=4 * D,
                        decoder_ffn_dim=4 * D, vocab_size=V, max_source_positions=1500, max_target_positions=448, num_mel_bins=80, pad_token_id=50257, bos_token_id=50257,
                        eos_token_id=50257, decoder_start_token_id=50258, suppress_tokens=None, begin_suppress_tokens=None)
    torch.manual_seed(0)
    with torch.device(DEV):
        model = WhisperForConditionalGeneration(cfg).train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-5)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(B, 80, 3000, generator=gen).to(DEV)
    lines, table = [], []

    def step(route, labels):
        for c, f in routes[route].items():
            c.forward = f
        opt.zero_grad(set_to_none=True)
        out = model(input_features=x, labels=labels)
        out.loss.backward()
        opt.step()
        return out

    for U in a.labels:
        labels = torch.randint(0, 50257, (B, U), generator=gen).to(DEV)
        for r in routes:
            for _ in range(a.warmup):
                step(r, labels)
        per = {r: [] for r in routes}
        for _ in range(a.reps):
            for r in routes:
                per[r].append(timed(lambda: step(r, labels)))
        ms = {r: med_spread(v) for r, v in per.items()}
        names = list(routes)
        beats = {names[i]: bool(ms[names[i - 1]][0] - ms[names[i]][0] > max(ms[names[i - 1]][1], ms[names[i]][1])) for i in (1, 2)}
        res = dict(tool="whisper_train_bench", what="step", device=torch.cuda.get_device_name(0), size="small", B=B, U=U, V=V, reps=a.reps,
                   median_ms={r: round(m, 2) for r, (m, _) in ms.items()}, spread_ms={r: round(s, 2) for r, (_, s) in ms.items()},
                   reps_ms={r: [round(t, 2) for t in v] for r, v in per.items()}, beats_predecessor=beats)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        table.append(f"step 16 x 30 s, labels 16 x {U:3d} | " + " | ".join(f"{r} {m:8.2f} ms (+-{s:.2f})" for r, (m, s) in ms.items()))
    # the repacking a changed parameter costs: the engines of both halves, rebuilt from the module's state dict
    enc, dec = model.model.encoder, model.model.decoder
    rep = {"encoder": [], "decoder": []}
    for _ in range(a.reps):
        enc.__dict__.pop("_hfasr_engine", None)
        dec.__dict__.pop("_hfasr_engine", None)
        rep["encoder"].append(timed(lambda: W._engine_for(enc)))
        rep["decoder"].append(timed(lambda: W._decoder_engine_for(dec)))
    res = dict(tool="whisper_train_bench", what="engine_rebuild", median_ms={k: round(med_spread(v)[0], 2) for k, v in rep.items()},
               spread_ms={k: round(med_spread(v)[1], 2) for k, v in rep.items()})
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    table.append("engine rebuild after an optimiser step (inside the step times above) | " + " | ".join(f"{k} {med_spread(v)[0]:.2f} ms (+-{med_spread(v)[1]:.2f})" for k, v in rep.items()))
    del model, opt
    torch.cuda.empty_cache()
    # the head alone: loss + logit gradient at M = 16 x 448 rows
    M = B * 448
    hid = (torch.randn(M, D, generator=gen) * 0.5).to(DEV, torch.bfloat16)
    w16 = (torch.randn(V, D, generator=gen) * 0.05).to(DEV, torch.bfloat16)
    lab = torch.randint(0, V, (M,), generator=gen).to(DEV)
    ldo = OT.pad64(V)

    def fused():
        acc, lse, _ = ops.gemm_ce(hid, w16, lab)
        g = torch.where(lab >= 0, 1.0 / acc[1], torch.zeros((), device=DEV))
        return OT.gemm_ce_bwd(hid, w16, lab, lse, g, ldo)

    def materialising():
        lg = ops.gemm(hid, w16, out_dtype=torch.float32).view(1, M, V)
        acc = ops.ce_label_smoothing(lg, lab.view(1, M), shift=0, eps=0.0, return_acc=True)
        return OT.ce_label_smoothing_bwd(lg, lab.view(1, M), acc, shift=0, eps=0.0, weight=1.0, ldo=ldo)

    legs = {"fused": fused, "materialising": materialising}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    per = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():
            per[k].append(timed(lambda: [fn() for _ in range(10)]) / 10)          # ten calls back to back per sample: a window of tens of ms
    ms = {k: med_spread(v) for k, v in per.items()}
    logit_bytes = M * V * 4
    res = dict(tool="whisper_train_bench", what="head", M=M, N=V, K=D, median_ms={k: round(m, 3) for k, (m, _) in ms.items()}, spread_ms={k: round(s, 3) for k, (_, s) in ms.items()},
               reps_ms={k: [round(t, 3) for t in v] for k, v in per.items()}, fp32_logit_bytes=logit_bytes,
               materialising_logit_traffic_bytes=6 * logit_bytes,          # written by the GEMM; read twice by the loss (max + sum, exp) and three times by its backward
               fused_beats_materialising=bool(ms["materialising"][0] - ms["fused"][0] > max(ms["fused"][1], ms["materialising"][1])))
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    table.append(f"head alone, loss + dlogits, M {M} N {V} K {D} | " + " | ".join(f"{k} {m:7.3f} ms (+-{s:.3f})" for k, (m, s) in ms.items())
                 + f" | fp32 logits {logit_bytes / 1e9:.2f} GB, written once and read five times by the materialising route")
    print("\n".join(table))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines + table) + "\n")


if __name__ == "__main__":
    main()
