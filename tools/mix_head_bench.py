#!/usr/bin/env python
"""ms per token of the config-5-shaped decoder step (8 layers x 512, 8 heads, V = 5001, 250 encoder frames, `head_locations=[5]`) with the folded two-tap head
(mi_decoder_step_taps; modes of GPT2LMMultiHeadModelMixing, `average_logits`) against the same step with the plain head (mi_gpt2_step / mi_decoder_step_beams — the
launches of the commit before the multi-tap head, bit for bit: tests/test_gpu_mix.py), alternated in ONE process on the same weights.

    python tools/mix_head_bench.py [--steps 200] [--rounds 5] [--warmup 20] [--out profiles/mix_head_bench.txt]

Settings: W = 1 and W = 5 for one utterance (1 and 5 rows: the plain head runs the fused three-launch form, the folded head the GEMV form — the fused form keeps a
layer's stream inside its launches), and 60 beams x 16 utterances (960 rows on shared cross K/V: one launch per op on both sides).  For W <= 8 a third leg times the plain
head on the GEMV form (step_form 1), which separates the cost of leaving the fused form from the cost of the taps and the wider head.  A round of a leg is `steps`
consecutive token steps after a one-token prompt between two device events; the legs alternate for `rounds` rounds.  Reported per leg: the mean over the rounds and the
spread (max - min of the per-round means).  Expected extra cost of the taps themselves: the second head matrix's bytes (V d 2 B = 5.1 MB: ~1 us at the 6.3 TB/s a
streaming read achieves) plus one small launch per tap.  One JSON line per setting, then a table."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from huggingface_asr_amd.decoder import GPT2DecoderEngine  # noqa: E402

DEV = "cuda:0"
CFG = dict(vocab_size=5001, n_embd=512, n_layer=8, n_head=8, n_positions=1024, head_locations=[5], head_weights=[0.5, 0.5], lsm_factor=0.0, layer_norm_epsilon=1e-5)
T_ENC, LMAX = 250, 256
SETTINGS = [("W=1", 1, 1), ("W=5", 5, 1), ("60x16", 960, 60)]          # (name, rows, beams of the shared-K/V step)


def state_dict(cfg, seed=0):
    """seeded GPT-2 cross-attention decoder weights in the reference's state-dict names (values only shape the timing through nothing: the step is shape-bound)"""
    g = torch.Generator().manual_seed(seed)
    d, V, L = cfg["n_embd"], cfg["vocab_size"], cfg["n_layer"]
    r = lambda *sh: torch.randn(*sh, generator=g) * 0.02
    sd = {"decoder.transformer.wte.weight": r(V, d), "decoder.transformer.wpe.weight": r(cfg["n_positions"], d), "decoder.transformer.ln_f.weight": torch.ones(d),
          "decoder.transformer.ln_f.bias": torch.zeros(d), "decoder.lm_head.weight": r(V, d), "decoder.additional_lm_heads.0.weight": r(V, d),
          "decoder.lm_mixing": 0.5 + 0.1 * torch.randn(2, V, generator=g)}
    for l in range(L):
        p = f"decoder.transformer.h.{l}."
        for ln in ("ln_1", "ln_2", "ln_cross_attn"):
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = torch.ones(d), torch.zeros(d)
        for name, (i, o) in {"attn.c_attn": (d, 3 * d), "attn.c_proj": (d, d), "crossattention.q_attn": (d, d), "crossattention.c_attn": (d, 2 * d),
                             "crossattention.c_proj": (d, d), "mlp.c_fc": (d, 4 * d), "mlp.c_proj": (4 * d, d)}.items():
            sd[p + name + ".weight"], sd[p + name + ".bias"] = r(i, o), torch.zeros(o)
    return sd


def leg(eng, rows, beams, form, steps, warmup):
    """ms per token of `steps` consecutive one-token steps of `eng` (after a one-token prompt and `warmup` steps) between two device events"""
    g = torch.Generator().manual_seed(1)
    enc = (torch.randn(rows // beams * T_ENC, CFG["n_embd"], generator=g)).to(DEV).to(torch.bfloat16)
    lens = torch.full((rows // beams,), T_ENC, dtype=torch.int32, device=DEV)
    kvs = eng.cross_kv(enc)
    cache = eng.init_cache(rows, LMAX)
    ids = torch.randint(3, CFG["vocab_size"], (rows, 1), generator=g).to(DEV)
    eng._gcfg.step_form = form
    try:
        for _ in range(1 + warmup):
            eng.step(ids, cache, kvs, T_ENC, lens, beams=beams)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            eng.step(ids, cache, kvs, T_ENC, lens, beams=beams)
        b.record()
        b.synchronize()
    finally:
        eng._gcfg.step_form = 0
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_head_bench: no GPU — a timing needs the device (nothing is measured on the CPU)")
    if 1 + a.warmup + a.steps >= LMAX:
        raise SystemExit(f"1 + warmup + steps must stay below the cache length {LMAX}")
    sd = state_dict(CFG)
    plain = GPT2DecoderEngine(dict(CFG), DEV)
    plain.load_state_dict(sd)
    mixed = GPT2DecoderEngine(dict(CFG, mixing_mode="linear"), DEV)
    mixed.load_state_dict(sd)
    lines = []
    for name, rows, beams in SETTINGS:
        legs = [("plain", plain, 0), ("folded", mixed, 0)] + ([("plain_form1", plain, 1)] if rows <= 8 else [])
        ms = {k: [] for k, _, _ in legs}
        for _ in range(a.rounds):
            for k, eng, form in legs:
                ms[k].append(leg(eng, rows, beams, form, a.steps, a.warmup))
        rec = dict(setting=name, rows=rows, beams=beams, steps=a.steps, rounds=a.rounds)
        for k, v in ms.items():
            rec[k + "_ms"], rec[k + "_spread_ms"] = round(sum(v) / len(v), 4), round(max(v) - min(v), 4)
        rec["folded_minus_plain_ms"] = round(rec["folded_ms"] - rec["plain_ms"], 4)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    table = ["setting   rows  plain ms (spread)   folded ms (spread)   plain, form 1 ms (spread)   folded - plain ms"]
    for r in lines:
        f1 = f"{r['plain_form1_ms']:.4f} ({r['plain_form1_spread_ms']:.4f})" if "plain_form1_ms" in r else "-"
        table.append(f"{r['setting']:<9} {r['rows']:<5} {r['plain_ms']:.4f} ({r['plain_spread_ms']:.4f})     {r['folded_ms']:.4f} ({r['folded_spread_ms']:.4f})      {f1:<27} "
                     f"{r['folded_minus_plain_ms']:+.4f}")
    text = "\n".join(table)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("python tools/mix_head_bench.py --steps %d --rounds %d --warmup %d\n" % (a.steps, a.rounds, a.warmup))
            f.write("\n".join(json.dumps(r) for r in lines) + "\n\n" + text + "\n")


if __name__ == "__main__":
    main()
