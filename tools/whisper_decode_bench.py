#!/usr/bin/env python
"""ms per token of the Whisper decoder step: the streaming form (mi_gpt2_config.step_form = 2, csrc/linear_rows.hip), the launch-per-op form (1) and transformers' own
decoder with its KV cache under bf16 autocast, alternated in ONE process on the same weights.

    python tools/whisper_decode_bench.py [--steps 200] [--rounds 3] [--warmup 20] [--out FILE.txt] [--timestamps]

Shapes: whisper-small size (d 768, 12 layers, V 51865, 1500 encoder keys) at B = 1, 16, 64 and whisper-medium size (d 1024, 24 layers) at B = 16.  A round of a leg is
`steps` consecutive token steps after a one-token prompt between two device events; the legs run 2 1 T 2 1 T ... for `rounds` rounds.  Reported per leg: the mean over
the rounds and the spread (max - min of the per-round means) — form 2 has to beat form 1 by more than that spread to be what `WhisperDecoderEngine` selects.  Next to
them the byte floor of a step (decoder weights + tied head + the cached encoder K/V of every row, each read once) at the 6.3 TB/s a streaming read achieves on this part,
and the share of that rate form 2 reaches.  One JSON line per shape, then a table.

--timestamps measures the token choice instead: the step followed by `mi_row_argmax` next to the step followed by `mi_whisper_timestamp_argmax` (the timestamp rules of
`greedy_decode(timestamps=...)`; an open segment of 32 sampled tokens as history), alternated R A R A ... in the engine's own step form, same rounds and spread rule."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from huggingface_asr_amd.whisper import WhisperDecoderEngine  # noqa: E402

DEV = "cuda:0"
ACHIEVABLE_TBS = 6.3
SHAPES = [("small", 768, 12, 12, 1), ("small", 768, 12, 12, 16), ("small", 768, 12, 12, 64), ("medium", 1024, 16, 24, 16)]
V, T_ENC, LMAX = 51865, 1500, 448


def floor_bytes(d, L, B):
    weights = L * (12 * d * d) * 2              # per layer wqkv 3d^2, wo, wq, wco d^2 each, fc1 + fc2 8d^2 — minus the cross K/V projection, which runs once per utterance
    head = V * d * 2
    cross = L * T_ENC * 2 * d * 2 * B
    return weights, head, cross


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--timestamps", action="store_true")
    a = ap.parse_args()
    assert 1 + a.steps <= LMAX and a.warmup + 1 <= LMAX
    from transformers import WhisperConfig
    from transformers.cache_utils import DynamicCache, EncoderDecoderCache
    from transformers.models.whisper.modeling_whisper import WhisperDecoder

    lines, table = [], []
    for name, d, H, L, B in SHAPES:
        c = WhisperConfig(d_model=d, decoder_layers=L, decoder_attention_heads=H, decoder_ffn_dim=4 * d, vocab_size=V, max_target_positions=LMAX, encoder_layers=1,
                          encoder_attention_heads=H, encoder_ffn_dim=64)
        torch.manual_seed(0)
        with torch.device(DEV):
            dec = WhisperDecoder(c).eval()
        cfg = dict(d_model=d, decoder_layers=L, decoder_attention_heads=H, decoder_ffn_dim=4 * d, vocab_size=V, max_target_positions=LMAX)
        eng = WhisperDecoderEngine(cfg, DEV)
        eng.load_state_dict(dec.state_dict())
        enc = torch.randn((B, T_ENC, d), device=DEV)
        kvs = eng.cross_kv(enc.to(torch.bfloat16).reshape(B * T_ENC, d))
        cache = eng.init_cache(B, LMAX)
        tok = torch.randint(0, V, (B, 1), device=DEV)

        def hip_leg(form):
            def run(n):
                eng.step_form = form
                cache["past"] = 0
                eng.step(tok, cache, kvs, T_ENC)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    eng.step(tok, cache, kvs, T_ENC)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / n
            return run

        def hf_leg(n):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                pkv = EncoderDecoderCache(DynamicCache(config=c), DynamicCache(config=c))
                step = lambda: torch.nn.functional.linear(dec(input_ids=tok, encoder_hidden_states=enc, past_key_values=pkv, use_cache=True).last_hidden_state[:, -1],
                                                          dec.embed_tokens.weight)
                step()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    step()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / n

        if a.timestamps:
            from huggingface_asr_amd import ops
            tb, P, n_hist = 50364, 4, 32
            ids = torch.randint(0, tb - 1, (B, LMAX), device=DEV)
            ids[:, P] = tb                                    # an open segment: one timestamp, then text
            rules = dict(begin_index=P, cur_len=P + n_hist, no_timestamps_token_id=tb - 1, eos_token_id=50257, max_initial_timestamp_index=50)

            def choice_leg(choose):
                def run(n):
                    eng.step_form = None
                    cache["past"] = 0
                    choose(eng.step(tok, cache, kvs, T_ENC))
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n):
                        choose(eng.step(tok, cache, kvs, T_ENC))
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1) / n
                return run
            legs = {"rules": choice_leg(lambda lg: ops.whisper_timestamp_argmax(lg, ids, **rules)), "argmax": choice_leg(ops.row_argmax)}
            for fn in legs.values():
                fn(a.warmup)
            per = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    per[k].append(fn(a.steps))
            mean = {k: sum(v) / len(v) for k, v in per.items()}
            spread = {k: max(v) - min(v) for k, v in per.items()}
            res = dict(tool="whisper_decode_bench", case="timestamps", device=torch.cuda.get_device_name(0), size=name, d=d, layers=L, B=B, V=V, keys=T_ENC, steps=a.steps,
                       rounds=a.rounds, form=eng.form_for(B), mean_ms={k: round(v, 4) for k, v in mean.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                       rounds_ms={k: [round(t, 4) for t in v] for k, v in per.items()}, row_bytes=V * 4,
                       rules_slower_than_argmax=bool(mean["rules"] - mean["argmax"] > max(spread.values())))
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            table.append(f"{name:7s} d {d:4d} L {L:2d} B {B:2d} | step + timestamp rules {mean['rules']:7.3f} ms (+-{spread['rules']:.3f}) | step + row argmax {mean['argmax']:7.3f} ms "
                         f"(+-{spread['argmax']:.3f}) | difference {1e3 * (mean['rules'] - mean['argmax']):+6.1f} us")
            del dec, eng, kvs, cache, enc
            torch.cuda.empty_cache()
            continue
        legs = {"form2": hip_leg(2), "form1": hip_leg(1), "transformers": hf_leg}
        for fn in legs.values():
            fn(a.warmup)
        per = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                per[k].append(fn(a.steps))
        wb, hb, cb = floor_bytes(d, L, B)
        floor_ms = (wb + hb + cb) / (ACHIEVABLE_TBS * 1e9)
        mean = {k: sum(v) / len(v) for k, v in per.items()}
        spread = {k: max(v) - min(v) for k, v in per.items()}
        res = dict(tool="whisper_decode_bench", device=torch.cuda.get_device_name(0), size=name, d=d, layers=L, B=B, V=V, keys=T_ENC, steps=a.steps, rounds=a.rounds,
                   mean_ms={k: round(v, 4) for k, v in mean.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                   rounds_ms={k: [round(t, 4) for t in v] for k, v in per.items()},
                   floor_bytes=dict(weights=wb, head=hb, cross_kv=cb), floor_ms_at_6p3_tbs=round(floor_ms, 4), form2_share_of_6p3_tbs=round(floor_ms / mean["form2"], 3),
                   form2_beats_form1=bool(mean["form1"] - mean["form2"] > max(spread["form1"], spread["form2"])))
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        table.append(f"{name:7s} d {d:4d} L {L:2d} B {B:2d} | form 2 {mean['form2']:7.3f} ms (+-{spread['form2']:.3f}) | form 1 {mean['form1']:7.3f} ms (+-{spread['form1']:.3f}) | "
                     f"transformers bf16 {mean['transformers']:7.3f} ms (+-{spread['transformers']:.3f}) | floor {floor_ms:6.3f} ms | form 2 at {100 * floor_ms / mean['form2']:4.1f} % of 6.3 TB/s")
        del dec, eng, kvs, cache, enc
        torch.cuda.empty_cache()
    print("\n".join(table))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines + table) + "\n")


if __name__ == "__main__":
    main()
