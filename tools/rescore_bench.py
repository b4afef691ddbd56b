"""Two-pass joint decoding (decoder.rescore: the CTC head's n-best, one teacher-forced decoder pass, a ranking) beside the token-by-token beam search (decoder.generate)
on the DeCRED_base-size structured model of tests/config5_model.py, in ONE process, shapes warmed, the two routes alternated, each call timed to a device synchronise:

  config 5   B = 1, a 10-s clip, W = 5, max_length 64, ctc_weight 0.3
  recipes    the settings of tools/wide_beam_bench.py: B = 16 clips of 10 s, W in {10, 60}, max_length 512, ctc_weight 0.3

Reports ms per call (median, min, max of the rounds), rescore's split into encoder, CTC beam search, decoder pass and select (device time between events,
decoder.rescore(stats=)), the shape of the pass (rows B * N, positions U, how many hypotheses exist) and the share of utterances whose rescored top-1 equals generate()'s.

    python tools/rescore_bench.py [--rounds 3] [--target-tokens 40 | --blank-bias X] [--out profiles/rescore_bench.txt]

What the numbers are and are not.  The model is untrained: its CTC head is random, so without help its hypotheses run to ~T' tokens, far past max_length.  The tool
adds a bias on the CTC head's blank (as tests/gen_model.py does), searched so that the best hypotheses have a transcript-like length (`--target-tokens`, a median over
the recipe batch; `--blank-bias` sets it by hand); the lengths that came out are printed.  The structured
decoder never favours the end-of-sequence token: generate() runs all max_length - 1 token steps — its worst case, and the recipes' cost bound — while a trained
model stops at the transcript's length.  The top-1 agreement is therefore expected to be 0 here and is reported, not asserted.  Word error rate: not measured (no
trained model, no data)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import config5_model as M  # noqa: E402
from huggingface_asr_amd import ops, synth  # noqa: E402
from huggingface_asr_amd.decoder import JointAEDEngine, generate, rescore  # noqa: E402

DEV = "cuda:0"


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def pick_blank_bias(eng, target, B=16):
    """the bias on the CTC head's blank logit at which the best hypothesis of the recipe batch has a median of `target` tokens (bisection; the length falls as the bias grows)"""
    x = torch.from_numpy(synth.normal(7, "rescore_bench/feats", (B, 1000, 80), 1.0)).to(DEV)
    enc_out, _, T2, _ = eng.encode(x, torch.full((B,), 1000, dtype=torch.int32, device=DEV))
    lens = enc_out["outer_len"].clamp(max=T2)
    lo, hi = 0.0, 16.0
    for _ in range(14):
        mid = (lo + hi) / 2
        lg = enc_out["logits"].float().clone()
        lg[..., -1] += mid
        n = ops.ctc_beam_decode(lg, lg.shape[-1] - 1, M.JCFG["pad_token_id"], lens, beams=5)["n_tokens"][:, 0]
        lo, hi = (mid, hi) if float(n.float().median()) > target else (lo, mid)
    return hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--target-tokens", type=int, default=40)
    ap.add_argument("--blank-bias", type=float, default=None)
    ap.add_argument("--settings", default="c5,w10,w60")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    sd = M.state_dict(0, structured=True)
    eng = JointAEDEngine(M.ENC_CFG, M.DEC_CFG, M.JCFG, DEV)
    eng.load_state_dict(sd)
    bias = a.blank_bias
    if bias is None:                                                   # the bias only shifts the blank's logit: search it on one batch of encoder logits
        bias = pick_blank_bias(eng, a.target_tokens)
    sd["encoder.blank_projection.bias"] = sd["encoder.blank_projection.bias"] + bias
    eng.load_state_dict(sd)
    say(f"rescore_bench: DeCRED_base-size structured model (V = {M.V}), 10-s clips, CTC blank bias +{bias:.3f} (best hypotheses of ~{a.target_tokens} tokens), "
        f"{a.rounds} rounds per route, alternated; {torch.cuda.get_device_name(0)}")
    table = dict(c5=("config 5", 1, 5, 64), w10=("recipe, 10 beams", 16, 10, 512), w60=("recipe, 60 beams", 16, 60, 512))
    for key in a.settings.split(","):
        name, B, W, ml = table[key]
        x = torch.from_numpy(synth.normal(7, "rescore_bench/feats", (B, 1000, 80), 1.0)).to(DEV)
        fl = torch.full((B,), 1000, dtype=torch.int32, device=DEV)
        kw = dict(num_beams=W, max_length=ml, ctc_weight=0.3, eos_token_id=1)
        gstats, rstats, tr = {}, {}, {}
        routes = [("generate", lambda: generate(eng, x, fl, stats=gstats, **kw)), ("rescore", lambda: rescore(eng, x, fl, stats=rstats, trace=tr, **kw))]
        for _, fn in routes:                                           # warm the shapes (allocator, workspaces, position table)
            fn()
        res, outs, split = {n: [] for n, _ in routes}, {}, []
        for _ in range(a.rounds):
            for n, fn in routes:
                ms, out = timed(fn)
                res[n].append(ms)
                outs[n] = out
            split.append(dict(rstats))
        n_tok = tr["n_tokens"].cpu()
        exist = int((tr["len"] > 0).sum())
        same = sum(g["tokens"] == r["tokens"] for g, r in zip(outs["generate"], outs["rescore"]))
        say(f"{name}: B = {B}, W = nbest = {W}, max_length = {ml}")
        say(f"  n-best lengths: min {int(n_tok.min())}, median {int(n_tok.float().median())}, max {int(n_tok.max())} tokens; pass of {B * W} rows x U = {tr['U']} positions "
            f"= {B * W * tr['U']} decoder rows, {exist} of {B * W} hypotheses exist; generate enqueued {gstats.get('steps')} token steps (route {gstats.get('route')})")
        for n, _ in routes:
            v = res[n]
            say(f"  {n:9s} ms per call: median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}")
        med = lambda k: statistics.median(s[k] for s in split)
        say("  rescore split (device ms, medians): " + ", ".join(f"{k} {med(k + '_ms'):.2f}" for k in ("encoder", "ctc_beam", "decoder_pass", "select")))
        g, r = statistics.median(res["generate"]), statistics.median(res["rescore"])
        spread = max(max(v) - min(v) for v in res.values())
        say(f"  rescore vs generate: {g / r:.1f}x ({g - r:+.1f} ms; larger spread of the rounds {spread:.1f} ms) -> "
            f"{'rescore FASTER beyond the spread' if g - r > spread else 'rescore NOT faster beyond the spread'}")
        say(f"  rescored top-1 == generate()'s top-1: {same} of {B} utterances (share {same / B:.2f}; reported, not asserted)")
    say("word error rate: not measured (no trained model, no data)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
