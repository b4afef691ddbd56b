"""Streaming step time of the causal encoder + CTC head (EncoderStream / mi_ebf_stream_step) against the full forward of the same audio.

    python tools/stream_bench.py --out profiles/stream_bench.txt

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--fill", type=int, default=400, help="encoder frames in the caches when the timing starts")
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
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
