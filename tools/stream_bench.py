"""Streaming step time of the causal encoder + CTC head (EncoderStream / mi_ebf_stream_step) against the full forward of the same audio.

    python tools/stream_bench.py --out profiles/stream_bench.txt
    python tools/stream_bench.py --beams 5,10,64 --out profiles/stream_bench.txt      # appends: the step without / with engine.stream(beams=W), the beam part alone

small-causal and base-causal (relative positions, synthetic weights), B in {1, 16} streams, C in {4, 16} encoder frames per step.  A step's cost depends on the
cache length (attention) and, at the start of a stream, on how many layers already have input (the L*r frames of lookahead), so the steady state is timed: the
streams are fed to `--fill` encoder frames first, then `--steps` steps are timed as one interval between two events.  One feature frame is 10 ms, so a step
carries 40*C ms of audio per stream: rtf = step time / audio time.  The split: with the library's launch timing on (mi_profile_*), the share of the step spent in
dense contractions (GEMMs and the conv GEMM) — everything else (LayerNorms, row copies, chunk attention, the stateful convs, head argmax, collapse) is the rest.
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from huggingface_asr_amd import _lib, shapes, synth  # noqa: E402
from huggingface_asr_amd.engine import EBranchformerEngine  # noqa: E402

DEV = "cuda:0"


def _time(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def _median(v):
    return sorted(v)[len(v) // 2]


def beams_table(args):
    """--beams: ms per step of engine.stream(...) without and with beams=W, the two alternated in one process (ROUNDS rounds of `--steps` - 1 steps each — one step
    of the count is the untimed one that fetches a step's logits —, the median per side), and the beam part alone (mi_ctc_beam_cut + mi_ctc_beam_stream_walk on a step's logits, fed to an ops.CtcBeamStream at the same fill).  Appended to --out."""
    from huggingface_asr_amd import ops
    ROUNDS = 3
    widths = [int(v) for v in args.beams.split(",")]
    timed = args.steps - 1
    lines = [f"# tools/stream_bench.py --beams {args.beams}: fill {args.fill} frames, {ROUNDS} alternated rounds of {timed} steps, medians; ms per step",
             "# expected from profiles/ctc_beam_bench.txt (one-shot walk 6.6-7.1 us / frame at 5-10 beams, 19 us at 64): C = 16 adds about 0.1-0.3 ms to a 2-5 ms step",
             "model        B   C  beams  step_ms(plain)  step_ms(beams)  added_ms   beam_alone_ms (cut + walk)   us/frame  state_MiB/stream"]
    for name, base in (("small-causal", shapes.SMALL), ("base-causal", shapes.BASE)):
        cfg = dict(base, is_causal=True)
        sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 7).items()}
        eng = EBranchformerEngine(cfg, DEV)
        eng.load_state_dict(sd)
        for B in (1, 16):
            for Cf in (4, 16):
                n_fill = args.fill // Cf
                total = (n_fill + ROUNDS * args.steps + 2) * Cf
                x = torch.from_numpy(synth.normal(7, "bench", (B, 4 * Cf, 80), 1.0)).to(DEV)
                for W in widths:
                    plain, beam = eng.stream(B, Cf, total), eng.stream(B, Cf, total, beams=W)
                    alone = ops.CtcBeamStream(B, total, beams=W, blank=cfg["vocab_size"], pad_id=-1, dtype=torch.int32)
                    for _ in range(n_fill):
                        plain.feed(x)
                        alone.feed(beam.feed(x)["logits"])
                    logits = plain.feed(x)["logits"]
                    beam.feed(x)
                    assert logits.shape[1] == Cf                           # past the lookahead: a step emits C frames
                    t_plain, t_beam, t_alone = [], [], []
                    for _ in range(ROUNDS):
                        t_plain.append(_time(lambda: plain.feed(x), timed))
                        t_beam.append(_time(lambda: beam.feed(x), timed))
                        t_alone.append(_time(lambda: alone.feed(logits), timed))
                    a, b, c = _median(t_plain), _median(t_beam), _median(t_alone)
                    lines.append(f"{name:12s} {B:2d}  {Cf:2d}  {W:5d}  {a:14.3f}  {b:14.3f}  {b - a:8.3f}   {c:12.3f}                 {1e3 * c / Cf:8.1f}  "
                                 f"{alone.state_bytes / B / 2**20:8.1f}")
                    print(lines[-1], flush=True)
                    del plain, beam, alone
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)
    print(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--fill", type=int, default=400, help="encoder frames in the caches when the timing starts")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--beams", default=None, help="comma-separated beam widths, e.g. 5,10,64: time the step with and without the prefix beam search on the stream "
                                                  "(engine.stream(..., beams=W)) and append that table to --out instead of writing the step table")
    args = ap.parse_args()
    if args.beams:
        return beams_table(args)
    lines = [f"# tools/stream_bench.py: fill {args.fill} frames, {args.steps} timed steps; ms per step, audio per step = 40*C ms per stream",
             "model        B   C  lookahead  step_ms  rtf     dense_ms(share)   state_MiB/stream  full_forward_ms(same audio)  stream_total_ms"]
    L = _lib.lib()
    for name, base in (("small-causal", shapes.SMALL), ("base-causal", shapes.BASE)):
        cfg = dict(base, is_causal=True)
        sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 7).items()}
        eng = EBranchformerEngine(cfg, DEV)
        eng.load_state_dict(sd)
        for B in (1, 16):
            for Cf in (4, 16):
                n_fill = args.fill // Cf
                total = (n_fill + args.steps + 2) * Cf
                st = eng.stream(B, Cf, total)
                x = torch.from_numpy(synth.normal(7, "bench", (B, 4 * Cf, 80), 1.0)).to(DEV)
                for _ in range(n_fill):
                    st.feed(x)
                ms = _time(lambda: st.feed(x), args.steps)
                # the dense share of one more step
                L.mi_profile_create(4096); L.mi_profile_reset(); L.mi_profile_enable(1)
                st.feed(x)
                torch.cuda.synchronize()
                L.mi_profile_enable(0)
                tm, fl = C.c_double(), C.c_double()
                L.mi_profile_summary(C.byref(tm), C.byref(fl))
                frames = st.n_feat // 4
                audio = torch.from_numpy(synth.normal(7, "full", (B, 4 * frames, 80), 1.0)).to(DEV)
                eng.forward(audio, None)
                full = _time(lambda: eng.forward(audio, None), 5)
                rtf = ms / (40.0 * Cf)
                lines.append(f"{name:12s} {B:2d}  {Cf:2d}  {st.lookahead:4d} fr    {ms:7.3f}  {rtf:6.4f}  {tm.value:6.3f} ({tm.value / ms:4.0%})      "
                             f"{st.state_bytes() / B / 2**20:8.1f}          {full:8.3f} ({frames} frames)         {ms * frames / Cf:9.1f}")
                print(lines[-1], flush=True)
                del st
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
