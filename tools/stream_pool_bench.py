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

    python tools/stream_pool_bench.py --beams 5,10,64 --out profiles/stream_pool_bench.txt      # APPENDS to --out

The prefix beam search on the pool (StreamPool.with_beams; csrc/ctc_beam_pool.hip), per beam width W, on the same staggered schedule:
  pool       the StreamPool(S) without beams, as above
  pool+beam  the same pool after with_beams(W): every step also runs the token cut over its compact logits and one walk block per named slot, and copies the counts (+3 launches)
  beam-only  those two launches alone (ops.CtcBeamPool.step) on the schedule's records — each slot's rows are what streaming.plan emits for it — over N(0, 3) logits
  sep+beam   S EncoderStream(1, beams=W) stepped round-robin: what the pool's refusal used to recommend (+2 launches per open session)
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
    def __init__(self, eng, S, Cf, Lmax, x, beams=None):
        self.pool, self.sched, self.x, self.sid = eng.stream_pool(S, Cf, Lmax), Schedule(S), x, {}
        if beams is not None:
            self.pool.with_beams(beams)

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
    def __init__(self, eng, S, Cf, Lmax, x, beams=None):
        self.st, self.sched, self.x = [eng.stream(1, Cf, Lmax, beams=beams) for _ in range(S)], Schedule(S), x[None]

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


class BeamOnlyForm:
    """the beam's two launches on the schedule's records: host bookkeeping as StreamPool's (streaming.plan per slot), no encoder"""

    def __init__(self, eng, S, Cf, Lmax, x, beams):
        from huggingface_asr_amd import ops
        c = eng.cfg
        self.C, self.L, self.r, self.W = Cf, c["num_hidden_layers"], (c.get("merge_conv_kernel", 31) - 1) // 2, x.shape[0]
        self.bp = ops.CtcBeamPool(S, Lmax, beams=beams, blank=c["vocab_size"], pad_id=-1, dtype=torch.int32, return_frames=True)
        self.sched, self.n_feat = Schedule(S), {}
        g = torch.Generator().manual_seed(7)
        self.logits = (torch.randn((S * (self.L * self.r + Cf + 2), c["vocab_size"] + 1), generator=g) * 3.0).to(DEV)

    def step(self):
        from huggingface_asr_amd.streaming import plan
        acts = self.sched.next()
        recs, at, audio = [], 0, 0
        for s, a in acts.items():
            if s not in self.n_feat:
                self.bp.open(s)
                self.n_feat[s] = 0
            n = self.W if a == "feed" else TAIL
            lo, hi = plan(self.n_feat[s] + n, self.C, self.L, self.r, a == "finish", n_prev=self.n_feat[s])[-1]
            recs.append((s, at, hi - lo, a == "finish", False))
            at += hi - lo
            audio += n
            self.n_feat[s] += n
            if a == "finish":
                del self.n_feat[s]
        if recs:
            self.bp.step(self.logits[:at], recs)
        return audio, 1 if acts else 0


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
    ap.add_argument("--beams", default=None, help="beam widths, e.g. 5,10,64: measure the pool with the prefix beam search instead, and APPEND to --out")
    args = ap.parse_args()
    cfg = dict(shapes.BASE, is_causal=True)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 7).items()}
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(sd)
    if args.beams:
        return beams_main(args, cfg, eng)
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


def beams_main(args, cfg, eng):
    per_call = 15 + 20 * cfg["num_hidden_layers"]
    lines = ["", f"# tools/stream_pool_bench.py --beams {args.beams}: base-causal, the staggered schedule, warm-up {args.warmup} steps, {ROUNDS} alternated rounds of {args.steps} steps, medians",
             "# step_ms: one step of the form; beam_ms: step_ms less the same form without beams (beam-only: itself); launches: kernel launches per step",
             " C   S   W  form       step_ms  beam_ms  audio_ms     rtf  launches"]
    for Cf in (int(v) for v in args.chunks.split(",")):
        x = torch.from_numpy(synth.normal(7, "bench", (4 * Cf, 80), 1.0)).to(DEV)
        Lmax = (max(lengths(i) for i in range(17)) + 2) * Cf
        for S in (int(v) for v in args.sessions.split(",")):
            for W in (int(v) for v in args.beams.split(",")):
                forms = {"pool": PoolForm(eng, S, Cf, Lmax, x), "pool+beam": PoolForm(eng, S, Cf, Lmax, x, W), "beam-only": BeamOnlyForm(eng, S, Cf, Lmax, x, W),
                         "separate": SeparateForm(eng, S, Cf, Lmax, x), "sep+beam": SeparateForm(eng, S, Cf, Lmax, x, W)}
                for f in forms.values():
                    _timed(f, args.warmup)
                ms = {k: [] for k in forms}
                for _ in range(ROUNDS):
                    for k, f in forms.items():
                        ms[k].append(_timed(f, args.steps))
                med = {k: sorted(v)[ROUNDS // 2] for k, v in ms.items()}
                base = {"pool": None, "pool+beam": "pool", "beam-only": None, "separate": None, "sep+beam": "separate"}
                for k in forms:
                    t, audio, calls = med[k]
                    beam = t if k == "beam-only" else (t - med[base[k]][0] if base[k] else 0.0)
                    n = calls * {"pool": per_call, "pool+beam": per_call + 3, "beam-only": 2, "separate": per_call, "sep+beam": per_call + 2}[k]
                    lines.append(f"{Cf:2d}  {S:2d}  {W:2d}  {k:9s}  {t:7.3f}  {beam:7.3f}  {audio:8.1f}  {t / audio:6.4f}  {n:8.0f}")
                    print(lines[-1], flush=True)
                del forms
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
