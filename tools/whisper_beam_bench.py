#!/usr/bin/env python
"""Whisper beam search: `whisper.beam_decode` (device loop, cross K/V shared by an utterance's hypotheses) next to transformers' own beam search with its KV cache under
bf16 autocast, on the same random weights, alternated in ONE process.

    python tools/whisper_beam_bench.py [--tokens 64] [--rounds 3] [--out profiles/whisper_beam_bench.txt]

Shapes: whisper-small size (d 768, 12 layers) and whisper-medium size (d 1024, 24 layers), B = 16 utterances x W = 5 beams, 1500 encoder keys, V 51865, a prompt of four
tokens.  EOS is suppressed on both sides, so every decode runs exactly `tokens` steps.  Legs, run D W T D W T ... for `rounds` rounds after one warm-up decode each:
`beam_decode` on the beam kernel `beam_loop_route` picks for this request (mi_beam_step), `beam_decode` forced onto mi_beam_step_wide, and `GenerationMixin.generate`
(num_beams = 5, the encoder output given, W-fold replicated by transformers).  Reported per leg: ms per decode and per token, the mean over the rounds and the spread
(max - min of the per-round means).  A leg counts as faster than another only by more than the larger of the two spreads; `beam_loop_route`'s rule is not changed by
this tool's output alone.  Then `mi_whisper_beam_scores` alone on 80 rows of V 51865 (suppression vector and timestamp rules on) next to `mi_row_lse` alone, device events.
One JSON line per measurement, then a table."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from huggingface_asr_amd import ops  # noqa: E402
from huggingface_asr_amd.decoder import beam_loop_route  # noqa: E402
from huggingface_asr_amd.whisper import WhisperDecoderEngine, beam_decode  # noqa: E402

DEV = "cuda:0"
SHAPES = [("small", 768, 12, 12), ("medium", 1024, 16, 24)]
V, T_ENC, LMAX, B, W, P = 51865, 1500, 448, 16, 5, 4
EOS, PAD, TB = 50257, 50256, 50364


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert P + a.tokens <= LMAX
    from transformers import WhisperConfig, WhisperForConditionalGeneration
    from transformers.generation.utils import GenerationMixin
    from transformers.modeling_outputs import BaseModelOutput
    lines, table = [], []
    for name, d, H, L in SHAPES:
        c = WhisperConfig(d_model=d, decoder_layers=L, decoder_attention_heads=H, decoder_ffn_dim=4 * d, vocab_size=V, max_target_positions=LMAX, encoder_layers=1,
                          encoder_attention_heads=H, encoder_ffn_dim=64, max_source_positions=T_ENC, pad_token_id=PAD, eos_token_id=EOS, bos_token_id=EOS,
                          decoder_start_token_id=50258, suppress_tokens=None, begin_suppress_tokens=None)
        torch.manual_seed(0)
        with torch.device(DEV):
            model = WhisperForConditionalGeneration(c).eval()
        eng = WhisperDecoderEngine(dict(d_model=d, decoder_layers=L, decoder_attention_heads=H, decoder_ffn_dim=4 * d, vocab_size=V, max_target_positions=LMAX), DEV)
        eng.load_state_dict(model.model.decoder.state_dict())
        enc = torch.randn((B, T_ENC, d), device=DEV)
        kvs = eng.cross_kv(enc.to(torch.bfloat16).reshape(B * T_ENC, d))
        prompt = torch.tensor([[50258, 50259, 50359, 50363]] * B, device=DEV)
        gc = model.generation_config
        gc.suppress_tokens, gc.begin_suppress_tokens, gc.eos_token_id, gc.pad_token_id = [EOS], None, EOS, PAD
        picked = beam_loop_route(W, V, P + a.tokens)

        def hip_leg(route):
            def run():
                state = dict(kvs=kvs, T2=T_ENC, cache=eng.init_cache(B, P + a.tokens))
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = beam_decode(None, eng, None, prompt, max_new_tokens=a.tokens, eos_token_id=EOS, pad_token_id=PAD, num_beams=W, suppress_tokens=[EOS], state=state, route=route)
                torch.cuda.synchronize()
                assert out.shape[1] == P + a.tokens
                return (time.perf_counter() - t) * 1e3
            return run

        def hf_leg():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = GenerationMixin.generate(model, encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=prompt, num_beams=W, max_new_tokens=a.tokens,
                                               do_sample=False)
                torch.cuda.synchronize()
                assert out.shape[1] == P + a.tokens
                return (time.perf_counter() - t) * 1e3
        legs = {f"beam_decode ({picked})": hip_leg(None), "beam_decode (device_wide)": hip_leg("device_wide"), "transformers bf16": hf_leg}
        for fn in legs.values():
            fn()
        per = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                per[k].append(fn())
        mean = {k: sum(v) / len(v) for k, v in per.items()}
        spread = {k: max(v) - min(v) for k, v in per.items()}
        res = dict(tool="whisper_beam_bench", device=torch.cuda.get_device_name(0), size=name, d=d, layers=L, B=B, W=W, V=V, keys=T_ENC, tokens=a.tokens, rounds=a.rounds,
                   decode_ms={k: round(v, 2) for k, v in mean.items()}, token_ms={k: round(v / a.tokens, 4) for k, v in mean.items()},
                   spread_ms={k: round(v, 2) for k, v in spread.items()}, rounds_ms={k: [round(t, 2) for t in v] for k, v in per.items()})
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        for k in legs:
            table.append(f"{name:7s} d {d:4d} L {L:2d} B {B} W {W} | {k:28s} | {mean[k]:8.1f} ms per decode (+-{spread[k]:.1f}) | {mean[k] / a.tokens:7.3f} ms per token")
        del model, eng, kvs, enc
        torch.cuda.empty_cache()
    # the score kernel alone
    rows = B * W
    Vp = (V + 7) // 8 * 8
    logits = torch.randn((rows, Vp), device=DEV)[:, :V]
    sup = torch.zeros(V, device=DEV)
    sup[torch.randperm(V, device=DEV)[:90]] = float("-inf")
    ids = torch.randint(0, TB - 1, (rows, LMAX), device=DEV)
    ids[:, P] = TB
    rules = dict(begin_index=P, cur_len=P + 32, suppress=sup, no_timestamps_token_id=TB - 1, eos_token_id=EOS, max_initial_timestamp_index=50)

    def timed(fn, n=200):
        for _ in range(20):
            fn()
        per = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            per.append(1e3 * e0.elapsed_time(e1) / n)
        return per
    k_us = {"mi_whisper_beam_scores": timed(lambda: ops.whisper_beam_scores(logits, ids, **rules)), "mi_row_lse": timed(lambda: ops.row_lse(logits))}
    res = dict(tool="whisper_beam_bench", case="score kernel alone", rows=rows, V=V, us={k: [round(t, 2) for t in v] for k, v in k_us.items()})
    lines.append(json.dumps(res))
    print(lines[-1], flush=True)
    for k, v in k_us.items():
        table.append(f"{k:24s} {rows} rows x V {V} | {sum(v) / len(v):7.2f} us per launch (+-{max(v) - min(v):.2f})")
    print("\n".join(table))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines + table) + "\n")


if __name__ == "__main__":
    main()
