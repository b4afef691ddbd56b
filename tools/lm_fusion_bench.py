#!/usr/bin/env python
"""What shallow-fusion LM rescoring costs per decode at the config-5 shape, and whether the LM's token step belongs on a stream of its own.

    python tools/lm_fusion_bench.py [--reps 7] [--warmup 2] [--out profiles/lm_fusion_bench.txt]

Model: BASELINE config 5 (E-Branchformer-base encoder + 8 x 512 GPT-2 decoder, V 5001, one 10 s clip, max_length 40, ctc_weight 0.3; seeded random weights, so every
decode runs its full length).  Language models: the GPT-2-small layout (d 768, 12 layers: outside the fused token step, launch per op) and d 512 / 6 layers (the fused
two-launches-per-layer step), both over the decoder's vocabulary.  Variants, alternated a b c a b c ... in ONE process for greedy and 5 beams:
    (a) no LM — the parent's number for the same call,   (b) LM step on the main stream behind the decoder step,   (c) LM step on its own stream beside it.
Reported per variant: the median over the repetitions of the decode (encoder output already there: `generate` from features) in ms and per token, and the spread
(max - min).  `decoder.generate`'s default becomes the side stream only if (c) beats (b) by more than that spread; (a) has no pass bar.  One JSON line per
(LM, beams), then a table."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from huggingface_asr_amd import fbank as FB, shapes, synth  # noqa: E402
from huggingface_asr_amd.decoder import GPT2LMEngine, JointAEDEngine, generate  # noqa: E402

DEV = "cuda:0"
V, MAXLEN = 5001, 40
LMS = [("gpt2-small layout", 768, 12, 12), ("d512 x 6", 512, 8, 6)]


def _block(sd, p, d, cross):
    names = [("ln_1.weight", (d,)), ("ln_1.bias", (d,)), ("attn.c_attn.weight", (d, 3 * d)), ("attn.c_attn.bias", (3 * d,)), ("attn.c_proj.weight", (d, d)),
             ("attn.c_proj.bias", (d,)), ("ln_2.weight", (d,)), ("ln_2.bias", (d,)), ("mlp.c_fc.weight", (d, 4 * d)), ("mlp.c_fc.bias", (4 * d,)),
             ("mlp.c_proj.weight", (4 * d, d)), ("mlp.c_proj.bias", (d,))]
    if cross:
        names += [("ln_cross_attn.weight", (d,)), ("ln_cross_attn.bias", (d,)), ("crossattention.q_attn.weight", (d, d)), ("crossattention.q_attn.bias", (d,)),
                  ("crossattention.c_attn.weight", (d, 2 * d)), ("crossattention.c_attn.bias", (2 * d,)), ("crossattention.c_proj.weight", (d, d)),
                  ("crossattention.c_proj.bias", (d,))]
    for n, s in names:
        sd[p + n] = torch.from_numpy(synth.init_param(0, p + n, s))


def joint_engine():
    enc_cfg = dict(shapes.BASE, vocab_size=5000, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    dec_cfg = dict(vocab_size=V, n_embd=512, n_layer=8, n_head=8, n_positions=256, head_locations=[5], head_weights=[0.4, 0.6], lsm_factor=0.1, pos_emb_fixed=True)
    jcfg = dict(ctc_weight=0.3, pad_token_id=5000, decoder_start_token_id=2)
    sd = {"encoder." + k: torch.from_numpy(synth.init_param(0, "encoder." + k, s)) for k, s in shapes.param_shapes(enc_cfg).items()}
    for n, s in [("decoder.transformer.wte.emb_layers.0.weight", (V, 512)), ("decoder.transformer.ln_f.weight", (512,)), ("decoder.transformer.ln_f.bias", (512,)),
                 ("decoder.lm_head.weight", (V, 512)), ("decoder.additional_lm_heads.0.weight", (V, 512))]:
        sd[n] = torch.from_numpy(synth.init_param(0, n, s))
    for l in range(8):
        _block(sd, f"decoder.transformer.h.{l}.", 512, True)
    eng = JointAEDEngine(enc_cfg, dec_cfg, jcfg, DEV)
    eng.load_state_dict(sd)
    return eng


def lm_engine(d, H, L):
    sd = {}
    for n, s in [("transformer.wte.weight", (V, d)), ("transformer.wpe.weight", (64, d)), ("transformer.ln_f.weight", (d,)), ("transformer.ln_f.bias", (d,))]:
        sd[n] = torch.from_numpy(synth.init_param(1, "lm." + n, s))
    for l in range(L):
        _block(sd, f"transformer.h.{l}.", d, False)
    eng = GPT2LMEngine(dict(vocab_size=V, n_embd=d, n_layer=L, n_head=H, n_positions=64, activation_function="gelu_new"), DEV)
    eng.load_state_dict(sd)                                      # no lm_head.weight: the tied head, GPT-2's default
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    eng = joint_engine()
    wave = torch.from_numpy(synth.waveforms(1, 1, 160000)).to(DEV)
    feats, frames = FB.fbank_gpu(wave, FB.FbankTables(80), pad_frames_to=100)
    lines, table = [], []
    for name, d, H, L in LMS:
        lm = lm_engine(d, H, L)
        for W in (1, 5):
            variants = {"a_no_lm": dict(), "b_lm_main_stream": dict(lm=lm, lm_weight=0.5), "c_lm_own_stream": dict(lm=lm, lm_weight=0.5, lm_side_stream=True)}
            times = {k: [] for k in variants}
            steps = {}
            for rep in range(a.warmup + a.reps):
                for k, kw in variants.items():
                    st = {}
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    generate(eng, feats, frames, num_beams=W, max_length=MAXLEN, ctc_weight=0.3, eos_token_id=1, stats=st, **kw)
                    torch.cuda.synchronize()
                    if rep >= a.warmup:
                        times[k].append((time.perf_counter() - t0) * 1e3)
                    steps[k] = st["steps"]
            med = {k: statistics.median(v) for k, v in times.items()}
            spread = {k: max(v) - min(v) for k, v in times.items()}
            side_wins = bool(med["b_lm_main_stream"] - med["c_lm_own_stream"] > max(spread["b_lm_main_stream"], spread["c_lm_own_stream"]))
            res = dict(tool="lm_fusion_bench", device=torch.cuda.get_device_name(0), lm=name, lm_d=d, lm_layers=L, beams=W, max_length=MAXLEN, reps=a.reps, steps=steps,
                       median_ms={k: round(v, 3) for k, v in med.items()}, spread_ms={k: round(v, 3) for k, v in spread.items()},
                       per_token_ms={k: round(med[k] / max(steps[k], 1), 4) for k in med}, lm_cost_ms=round(med["b_lm_main_stream"] - med["a_no_lm"], 3),
                       own_stream_beats_main_by_more_than_the_spread=side_wins)
            lines.append(json.dumps(res))
            print(lines[-1], flush=True)
            table.append(f"{name:18s} beams {W} | " + " | ".join(f"({k[0]}) {med[k]:7.2f} ms, {med[k] / max(steps[k], 1):6.3f} ms/token (spread {spread[k]:.2f})" for k in med) +
                         f" | own stream wins: {side_wins}")
        del lm
        torch.cuda.empty_cache()
    print("\n".join(table))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines + table) + "\n")


if __name__ == "__main__":
    main()
