"""Beam search at the reference's evaluation-recipe settings (recipes_v0.0.1/librispeech_aed/decoding/*_beam_decode.sh: --num_beams=60 --max_length=512, eval batch 16;
ebranchformer_english/decoding: 10 beams; training recipes' --override_for_evaluation: ctc_weight 0.3, 10 beams) on the DeCRED_base-size model of tests/config5_model.py:
B = 16 clips of 10 s, W in {10, 60}, max_length 512, ctc_weight 0, plus 0.3 at W = 10.

Two routes for the same request, alternated in one process, `--rounds` times each:
  new     decoder.generate                 the device-resident loop (mi_beam_step / mi_beam_step_wide by decoder.beam_loop_route), hypotheses sharing their utterance's
                                           cross K/V when the step has more than 8 rows
  parent  decoder.generate_stepwise(share_cross_kv=False)
                                           what such a request ran before mi_beam_step_wide: the host loop (for W = 10 at max_length 512 the parent ran the device loop
                                           with replicated K/V; that route is `generate(share_cross_kv=False)` and is reported as well) over K/V replicated per beam
Reports ms per decode (median, min, max of the rounds), ms per token step, peak device memory of a decode, the cross K/V bytes of each arrangement
(decoder.cross_kv_layout: exact, from the shapes), and mi_beam_step_wide alone in microseconds per launch at the same (B, W, V).

    python tools/wide_beam_bench.py [--rounds 3] [--max-length 512] [--batch 16] [--out profiles/wide_beam_bench.txt]

The structured weights (tests/config5_model.py) never favour the end-of-sequence token, so every decode runs all max_length - 1 token steps: ms per token = ms / steps."""
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
from huggingface_asr_amd import _lib, ops, synth  # noqa: E402
from huggingface_asr_amd.decoder import JointAEDEngine, _step_denoms, beam_loop_route, cross_kv_layout, generate, generate_stepwise  # noqa: E402

DEV = "cuda:0"


def kernel_alone(B, W, V, max_length, with_ctc, reps=30):
    """mi_beam_step_wide at step max_length / 2 behind a kernel that rewrites the logits: median microseconds per call (both launches)"""
    L = _lib.lib()
    n, Lmax, cur = B * W, max_length + 1, max_length // 2
    g = torch.Generator().manual_seed(W)
    Vp = (V + 7) // 8 * 8
    logits = (torch.randn(n, Vp, generator=g) * 2).to(DEV)[:, :V]
    ctc = (torch.randn(n, V, generator=g) * 3 - 5).to(DEV) if with_ctc else None
    ids = torch.full((n, Lmax), V - 1, dtype=torch.long, device=DEV)
    ids[:, 0] = 2
    denom, heur = _step_denoms(cur, max_length, 1.0, False)
    ts = []
    for _ in range(reps):
        bs = -(torch.arange(n, device=DEV) % W).float()
        done, nfin = torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)
        fs, fl = torch.zeros(B, W, device=DEV), torch.zeros(B, W, dtype=torch.int32, device=DEV)
        ft = torch.full((B, W, Lmax), V - 1, dtype=torch.long, device=DEV)
        nt, bi = torch.empty(n, dtype=torch.long, device=DEV), torch.empty(n, dtype=torch.long, device=DEV)
        logits.mul_(1.0001)
        lse = ops.row_lse(logits)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _lib.check(L.mi_beam_step_wide(logits.data_ptr(), logits.stride(0), lse.data_ptr(), ctc.data_ptr() if with_ctc else None, 0.7 if with_ctc else 1.0,
                                       0.3 if with_ctc else 0.0, int(with_ctc), V - 1, 1, B, W, V, cur, max_length, Lmax, denom, heur, 0, ids.data_ptr(), bs.data_ptr(),
                                       nt.data_ptr(), bi.data_ptr(), done.data_ptr(), nfin.data_ptr(), fs.data_ptr(), fl.data_ptr(), ft.data_ptr(), None, None, None,
                                       None, 0, None, 0.0, torch.cuda.current_stream().cuda_stream), "mi_beam_step_wide")
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, torch.cuda.max_memory_allocated() / 2 ** 30, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-length", type=int, default=512)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, ml, V = a.batch, a.max_length, M.V
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    eng = JointAEDEngine(M.ENC_CFG, M.DEC_CFG, M.JCFG, DEV)
    eng.load_state_dict(M.state_dict(0, structured=True))
    x = torch.from_numpy(synth.normal(7, "wide_beam_bench/feats", (B, 1000, 80), 1.0)).to(DEV)        # 10 s of 10 ms frames per clip
    fl = torch.full((B,), 1000, dtype=torch.int32, device=DEV)
    T2 = eng.encode(x, fl)[2]
    say(f"wide_beam_bench: B = {B}, 10-s clips (T' = {T2}), V = {V}, max_length = {ml}, {a.rounds} rounds per route, alternated; {torch.cuda.get_device_name(0)}")
    for W, cw in ((10, 0.0), (10, 0.3), (60, 0.0)):
        kw = dict(num_beams=W, max_length=ml, ctc_weight=cw, eos_token_id=1)
        route = beam_loop_route(W, V, ml)
        routes = [("new", lambda: generate(eng, x, fl, stats=stats, **kw)), ("parent", lambda: generate_stepwise(eng, x, fl, share_cross_kv=False, **kw))]
        if route == "device":                                          # the parent ran this request on the device loop, K/V replicated
            routes.insert(1, ("parent_device", lambda: generate(eng, x, fl, share_cross_kv=False, **kw)))
        res = {name: [] for name, _ in routes}
        mem, outs, stats = {}, {}, {}
        for r in range(a.rounds):
            for name, fn in routes:
                ms, gib, out = timed(fn)
                res[name].append(ms)
                mem[name] = max(mem.get(name, 0.0), gib)
                outs[name] = out
        steps = stats.get("steps", ml - 1)
        lens = {name: max(len(h["tokens"]) for h in out) for name, out in outs.items()}
        same = all([h["hypotheses"] for h in outs["new"]] == [h["hypotheses"] for h in out] for out in outs.values())
        sh, rep = cross_kv_layout(B, W, T2, M.D, M.L), cross_kv_layout(B, W, T2, M.D, M.L, share=False)
        say(f"W = {W}, ctc_weight = {cw}: route {route}, {steps} token steps enqueued, longest hypothesis {lens}, all routes return the same hypotheses: {same}")
        say(f"  cross K/V bytes (derived from the shapes): shared {sh['bytes'] / 1e6:.1f} MB (beams = {sh['beams']}), replicated {rep['bytes'] / 1e6:.1f} MB")
        for name, _ in routes:
            v = res[name]
            say(f"  {name:14s} ms per decode: median {statistics.median(v):9.1f}  min {min(v):9.1f}  max {max(v):9.1f}  spread {max(v) - min(v):8.1f}   "
                f"ms per token {statistics.median(v) / max(steps, 1):7.3f}   peak memory {mem[name]:6.2f} GiB")
        new, par = res["new"], res["parent"]
        margin = statistics.median(par) - statistics.median(new)
        spread = max(max(new) - min(new), max(par) - min(par))
        say(f"  new vs parent: margin {margin:9.1f} ms, larger spread {spread:8.1f} ms -> {'FASTER beyond the spread' if margin > spread else 'NOT faster beyond the spread'}")
        med, lo = kernel_alone(B, W, V, ml, cw > 0)
        say(f"  mi_beam_step_wide alone (B = {B}, W = {W}, V = {V}, cur_len = {ml // 2}): median {med:.1f} us per call, min {lo:.1f} us")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
