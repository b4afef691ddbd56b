"""Step time of the streaming session pool (engine.stream_pool / mi_ebf_stream_step_slots) against the two forms it stands between.

    python tools/stream_pool_bench.py --out profiles/stream_pool_bench.txt

base-causal (relative positions, synthetic weights), C in {4, 16} encoder frames per chunk (tools/stream_bench.py's), S in {1, 4, 16} sessions.  One schedule per S:
session i opens at step i, lasts 30 + (5 i mod 17) chunks plus a tail of 7 frames, and its slot is reopened the step after it finishes with the next length of the
sequence — unequal lengths, staggered by one chunk, slot reuse.  Three forms walk it:
  pool      one StreamPool(S): a step = one pool.step() over whatever sessions are open
  separate  S EncoderStream(1) objects stepped round-robin on the same schedule (today's only way): a step = one feed / finish per open session
  lockstep  one EncoderStream(S) on equal-length, equal-start sessions of the schedule's mean length (feed .. finish, reset, again): the bound the pool cannot beat
  pool-eq   the StreamPool(S) on the lock-step form's schedule (all slots open, feed and finish together): what the pool's mechanism costs at equal work
The forms are alternated in one process after a warm-up (ROUNDS rounds of --steps steps each, the median per form).  One feature frame is 10 ms: the aggregate
real-time factor is step time / audio fed in the step, summed over the sessions.  Launches per step: the driver's call list in the steady state (12 front-end + 20 per
layer + 3 for the head, one kernel each where a GEMM is one launch) times the driver calls of the step — 1 for the pool and the lock-step batch, one per open session
for the separate streams; a finish adds the resets of that form (not counted).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from huggingface_asr_amd import shapes, synth  # noqa: E402
from huggingface_asr_amd.engine import EBranchformerEngine  # noqa: E402

DEV = "cuda:0"
ROUNDS = 3
TAIL = 7


def lengths(i):
    return 30 + (5 * i) % 17


class Schedule:
    """per step: {slot: "feed" | "finish"}; slot i opens at step i, reopens the step after it finishes"""

    def __init__(self, S):
        self.S, self.t, self.k = S, 0, S
        self.left = [None] * S                  # chunks still to feed
        self.n = [lengths(i) for i in range(S)]

    def next(self):
        acts = {}
        for s in range(self.S):
            if self.left[s] is None:
                if self.t >= s:
                    self.left[s] = self.n[s]
                else:
                    continue
            if self.left[s] > 0:
                acts[s] = "feed"
                self.left[s] -= 1
            else:
                acts[s] = "finish"
                self.left[s] = None
                self.n[s] = lengths(self.k)
                self.k += 1
        self.t += 1
        return acts


class PoolForm:
    def __init__(self, eng, S, Cf, Lmax, x):
        self.pool, self.sched, self.x, self.sid = eng.stream_pool(S, Cf, Lmax), Schedule(S), x, {}

    def step(self):
        acts = self.sched.next()
        for s in acts:
            if s not in self.sid:
                self.sid[s] = self.pool.open()
        feed = {self.sid[s]: self.x for s, a in acts.items() if a == "feed"}
        fin = {self.sid[s]: self.x[:TAIL] for s, a in acts.items() if a == "finish"}
        self.pool.step(feed, fin)
        for s, a in acts.items():
            if a == "finish":
                del self.sid[s]
        return sum(self.x.shape[0] if a == "feed" else TAIL for a in acts.values()), 1 if acts else 0


class SeparateForm:
    def __init__(self, eng, S, Cf, Lmax, x):
        self.st, self.sched, self.x = [eng.stream(1, Cf, Lmax) for _ in range(S)], Schedule(S), x[None]

    def step(self):
        acts = self.sched.next()
        for s, a in acts.items():
            if a == "feed":
                self.st[s].feed(self.x)
            else:
                self.st[s].finish(self.x[:, :TAIL])
                self.st[s].reset()
        return sum(self.x.shape[1] if a == "feed" else TAIL for a in acts.values()), len(acts)


class LockstepForm:
    def __init__(self, eng, S, Cf, Lmax, x):
        self.st, self.S, self.x, self.left = eng.stream(S, Cf, Lmax), S, x[None].expand(S, -1, -1).contiguous(), None
        self.n = round(sum(lengths(i) for i in range(17)) / 17)

    def step(self):
        if self.left is None:
            self.left = self.n
        if self.left > 0:
            self.st.feed(self.x)
            self.left -= 1
            return self.S * self.x.shape[1], 1
        self.st.finish(self.x[:, :TAIL])
        self.st.reset()
        self.left = None
        return self.S * TAIL, 1


class PoolEqualForm:
    def __init__(self, eng, S, Cf, Lmax, x):
        self.pool, self.S, self.x, self.left, self.sid = eng.stream_pool(S, Cf, Lmax), S, x, None, []
        self.n = round(sum(lengths(i) for i in range(17)) / 17)

    def step(self):
        if self.left is None:
            self.left, self.sid = self.n, [self.pool.open() for _ in range(self.S)]
        if self.left > 0:
            self.pool.step(feed={s: self.x for s in self.sid})
            self.left -= 1
            return self.S * self.x.shape[0], 1
        self.pool.step(finish={s: self.x[:TAIL] for s in self.sid})
        self.left = None
        return self.S * TAIL, 1


def _timed(form, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    done = [form.step() for _ in range(n)]
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n, 10.0 * sum(d[0] for d in done) / n, sum(d[1] for d in done) / n           # ms per step, ms of audio per step, driver calls per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=40, help="steps of every form before the timing: past the sessions' staggered starts and their lookahead")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--chunks", default="4,16")
    ap.add_argument("--sessions", default="1,4,16")
    args = ap.parse_args()
    cfg = dict(shapes.BASE, is_causal=True)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 7).items()}
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(sd)
    lines = [f"# tools/stream_pool_bench.py: base-causal, warm-up {args.warmup} steps, {ROUNDS} alternated rounds of {args.steps} steps, medians",
             "# step_ms: one step of the form; audio_ms: audio fed in it, all sessions; rtf = step_ms / audio_ms (aggregate); launches: kernel launches per step",
             " C   S  form      step_ms  audio_ms     rtf  launches"]
    for Cf in (int(v) for v in args.chunks.split(",")):
        x = torch.from_numpy(synth.normal(7, "bench", (4 * Cf, 80), 1.0)).to(DEV)
        Lmax = (max(lengths(i) for i in range(17)) + 2) * Cf
        for S in (int(v) for v in args.sessions.split(",")):
            forms = {"pool": PoolForm(eng, S, Cf, Lmax, x), "separate": SeparateForm(eng, S, Cf, Lmax, x), "lockstep": LockstepForm(eng, S, Cf, Lmax, x),
                     "pool-eq": PoolEqualForm(eng, S, Cf, Lmax, x)}
            for f in forms.values():
                _timed(f, args.warmup)
            ms = {k: [] for k in forms}
            for _ in range(ROUNDS):
                for k, f in forms.items():
                    ms[k].append(_timed(f, args.steps))
            for k, f in forms.items():
                t, audio, calls = sorted(ms[k])[ROUNDS // 2]
                lines.append(f"{Cf:2d}  {S:2d}  {k:8s}  {t:7.3f}  {audio:8.1f}  {t / audio:6.4f}  {calls * (15 + 20 * cfg['num_hidden_layers']):8.0f}")
                print(lines[-1], flush=True)
            del forms
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
