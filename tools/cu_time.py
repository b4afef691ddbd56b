"""CU time per kernel family from a ONE-step-at-a-time kernel trace: the check on the model "with steps in flight the wall per step is the sum over launches of
(CUs a launch holds x its duration) / 256, not the sum of the launch durations".

    python tools/cu_time.py <kernel_trace.csv> [--wall-ms <timed four-lane ms per step>] [first_step] [n_steps]
    (trace of `bench.py --streams 1 --wide-tiles 1 --steps K --warmup W --no-kernel-events --no-secondary --no-cpu-baseline`; steps delimited by the fbank kernel)

A launch's blocks come from the trace's own grid / workgroup columns.  It holds min(blocks, 256) CUs for its duration: a launch of more blocks than CUs runs in
rounds on all of them.  For the dense kernels (one 512-thread block with 128 KiB of LDS per CU) that is exact; for the small-block kernels (LayerNorm, depthwise convs,
attention: several blocks per CU, and other lanes' blocks can share the CU) it is an upper bound, so the sum is one too.
"""
import collections
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lanes_trace import family

CUS = 256


def blocks_of(r):
    n = 1
    for ax in "XYZ":
        g, w = r.get(f"Grid_Size_{ax}"), r.get(f"Workgroup_Size_{ax}")
        if g and w:
            n *= max(1, int(g) // max(1, int(w)))
    return n


def table(path, first=2, n=None):
    """-> (steps, {family: [launches, blocks, ns, cu_ns]}, wall ns per step) over steps [first, first + n) of the trace"""
    rows = list(csv.DictReader(open(path)))
    fb = sorted(int(r["Start_Timestamp"]) for r in rows if "fbank_kernel" in r["Kernel_Name"])
    if n is None:
        n = len(fb) - first - 1
    t0, t1 = fb[first], fb[first + n]
    fam = collections.defaultdict(lambda: [0, 0, 0, 0])
    for r in rows:
        s = int(r["Start_Timestamp"])
        if not t0 <= s < t1:
            continue
        b, dur = blocks_of(r), int(r["End_Timestamp"]) - s
        v = fam[family(r["Kernel_Name"], b)]
        v[0] += 1; v[1] += b; v[2] += dur; v[3] += min(b, CUS) * dur
    return n, fam, (t1 - t0) / n


def main():
    a = sys.argv[1:]
    wall = None
    if "--wall-ms" in a:
        i = a.index("--wall-ms"); wall = float(a[i + 1]); del a[i:i + 2]
    n, fam, step_ns = table(a[0], int(a[1]) if len(a) > 1 else 2, int(a[2]) if len(a) > 2 else None)
    tot = sum(v[3] for v in fam.values())
    print(f"{n} steps, one at a time: wall {step_ns / 1e3:.1f} us per step, kernel time {sum(v[2] for v in fam.values()) / n / 1e3:.1f} us per step")
    print("launches/step x avg blocks x avg us = CU-us per step (min(blocks, 256) x us)   share   family")
    for k, v in sorted(fam.items(), key=lambda kv: -kv[1][3]):
        print(f"{v[0] / n:7.1f} x {v[1] / v[0]:7.0f} x {v[2] / v[0] / 1e3:8.2f} us = {v[3] / n / 1e3:10.0f} CU-us  {100 * v[3] / tot:5.1f} %  {k}")
    line = f"sum {tot / n / 1e3:.0f} CU-us per step; over {CUS} CUs = {tot / n / 1e6 / CUS:.3f} ms per step"
    if wall is not None:
        line += f"; timed wall with steps in flight {wall:.3f} ms per step (model / wall = {tot / n / 1e6 / CUS / wall:.2f})"
    print(line)


if __name__ == "__main__":
    main()
