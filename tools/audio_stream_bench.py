"""Step time of the session pool fed audio (engine.audio_pool: csrc/fbank_stream.hip in front of mi_ebf_stream_step_slots) against the same step fed features and
against the composition a caller had to write before.

    python tools/audio_stream_bench.py --out profiles/audio_stream_bench.txt

base-causal (relative positions, synthetic weights), global normalisation, C in {4, 16} encoder frames per chunk, S in {1, 16} sessions.  All S sessions are open and
every call brings each of them one chunk's worth of audio (4 C x 160 samples); after --chunks-per-session calls they finish and reopen.  Three forms, alternated in one
process after a warm-up, the median of ROUNDS rounds per form:
  audio     pool.push(audio={sid: samples}): one push launch for all slots, one pop, one pool step
  features  the wrapped StreamPool.step fed precomputed feature chunks: the floor
  composed  per session a torch.cat of the carried samples and the new ones, fbank_gpu (mi_fbank_f64 + mi_cmvn_global) on it, slicing of the new carry and of the
            chunk; then the same StreamPool.step
and alone, on a FbankStream of S slots: push (S x one chunk's worth of samples) and pop (S chunks), each with its record upload.
Launches per call, counted from the drivers' call lists: the pool step's 15 + 20 L (tools/stream_pool_bench.py); audio adds 2 kernels (push, pop) and 2 record uploads;
composed adds per session 1 cat + 2 kernels (fbank, global norm) + the fill of fbank_gpu's output + the stack of the chunks.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from huggingface_asr_amd import fbank as FB  # noqa: E402
from huggingface_asr_amd import shapes, synth  # noqa: E402
from huggingface_asr_amd.engine import EBranchformerEngine  # noqa: E402

DEV = "cuda:0"
ROUNDS = 5


class AudioForm:
    def __init__(self, eng, S, Cf, Lmax, wave, n, stats):
        self.pool, self.S, self.wave, self.n, self.i, self.sid = eng.audio_pool(S, Cf, Lmax, **stats), S, wave, n, 0, None
        self.m = 4 * Cf * 160

    def step(self):
        if self.sid is None:
            self.sid, self.i = [self.pool.open() for _ in range(self.S)], 0
        piece = self.wave[self.i * self.m:(self.i + 1) * self.m]
        self.i += 1
        if self.i < self.n:
            self.pool.push(audio={s: piece for s in self.sid})
        else:
            self.pool.push(finish={s: piece[:1000] for s in self.sid})
            self.sid = None


class FeatureForm:
    def __init__(self, eng, S, Cf, Lmax, x, n):
        self.pool, self.S, self.x, self.n, self.i, self.sid = eng.stream_pool(S, Cf, Lmax), S, x, n, 0, None

    def step(self):
        if self.sid is None:
            self.sid, self.i = [self.pool.open() for _ in range(self.S)], 0
        self.i += 1
        if self.i < self.n:
            self.pool.step(feed={s: self.x for s in self.sid})
        else:
            self.pool.step(finish={s: self.x[:7] for s in self.sid})
            self.sid = None


class ComposedForm:
    """what a caller of stream_pool wrote before audio_pool: carry, fbank, normalisation and chunking per session, outside the library"""

    def __init__(self, eng, S, Cf, Lmax, wave, n, stats, tables):
        self.pool, self.S, self.wave, self.n, self.i, self.sid = eng.stream_pool(S, Cf, Lmax), S, wave, n, 0, None
        self.m, self.W, self.tb = 4 * Cf * 160, 4 * Cf, tables
        self.stats = dict(normalize="global", global_means=torch.as_tensor(stats["global_means"]).to(DEV), global_stds=torch.as_tensor(stats["global_stds"]).to(DEV))

    def _extract(self, k, new):
        buf = torch.cat([self.carry[k], new])
        T = FB.num_frames(buf.numel())
        if T:
            f, _ = FB.fbank_gpu(buf[None], self.tb, **self.stats)
            self.fifo[k] = torch.cat([self.fifo[k], f[0]])
        self.carry[k] = buf[160 * T:]

    def step(self):
        if self.sid is None:
            self.sid, self.i = [self.pool.open() for _ in range(self.S)], 0
            self.carry = [self.wave[:0] for _ in range(self.S)]
            self.fifo = [torch.zeros((0, 80), device=DEV) for _ in range(self.S)]
        piece = self.wave[self.i * self.m:(self.i + 1) * self.m]
        self.i += 1
        last = self.i >= self.n
        for k in range(self.S):
            self._extract(k, piece[:1000] if last else piece)
        if last:
            while self.fifo[0].shape[0] > self.W:
                self._feed()
            self.pool.step(finish={s: self.fifo[k] for k, s in enumerate(self.sid)})
            self.sid = None
        elif self.fifo[0].shape[0] >= self.W:
            self._feed()

    def _feed(self):
        self.pool.step(feed={s: self.fifo[k][:self.W] for k, s in enumerate(self.sid)})
        self.fifo = [f[self.W:] for f in self.fifo]


class FrontEndForm:
    """push and pop alone"""

    def __init__(self, S, Cf, wave, stats, tables, what):
        self.fb = FB.FbankStream(S, 4 * Cf, 4 * Cf * 160, tables, device=DEV, **stats)
        self.S, self.W, self.what, self.piece = S, 4 * Cf, what, wave[:4 * Cf * 160]
        for s in range(S):
            self.fb.open(s)
        self.fb.push({s: wave[:400] for s in range(S)})           # one frame behind: from here every push of a chunk's samples completes a chunk
        self.fb.pop([(s, 1) for s in range(S)])
        self.flat, self.spans = self.piece.repeat(S), {s: (s * self.piece.numel(), self.piece.numel()) for s in range(S)}

    def step(self):
        fb = self.fb
        if self.what == "push":
            fb.push_flat(self.flat, self.spans)
            for s in range(self.S):                                # host bookkeeping of a pop, no launch: the ring never fills
                fb.r[s] = (fb.r[s] + fb.count[s]) % fb.R
                fb.count[s] = 0
        else:
            for s in range(self.S):                                # host bookkeeping of a push, no launch
                fb.count[s] = self.W
            fb.pop([(s, self.W) for s in range(self.S)])


def _timed(form, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        form.step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=24)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--chunks-per-session", type=int, default=24)
    ap.add_argument("--chunks", default="4,16")
    ap.add_argument("--sessions", default="1,16")
    args = ap.parse_args()
    cfg = dict(shapes.BASE, is_causal=True)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 7).items()}
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(sd)
    tables = FB.FbankTables(80)
    stats = dict(normalize="global", global_means=synth.normal(7, "means", (80,), 1.0) + 10.0, global_stds=abs(synth.normal(7, "stds", (80,), 1.0)) + 1.0)
    n = args.chunks_per_session
    launches = 15 + 20 * cfg["num_hidden_layers"]
    lines = [f"# tools/audio_stream_bench.py: base-causal, global normalisation, warm-up {args.warmup} calls, {ROUNDS} alternated rounds of {args.steps} calls, medians",
             "# call_ms: one call of the form = one chunk's worth of audio for each of the S sessions; audio_ms: that audio, all sessions; launches: kernels per call",
             "# (steady state; audio: + 2 record uploads; composed: + S cats, S fills, a stack); push / pop: the front end's two launches alone, with their upload",
             " C   S  form      call_ms  audio_ms     rtf  launches"]
    for Cf in (int(v) for v in args.chunks.split(",")):
        wave = torch.from_numpy(synth.waveforms(7, 1, (n + 1) * 4 * Cf * 160)[0]).to(DEV)
        x = torch.from_numpy(synth.normal(7, "bench", (4 * Cf, 80), 1.0)).to(DEV)
        Lmax = (n + 2) * Cf
        for S in (int(v) for v in args.sessions.split(",")):
            forms = {"audio": AudioForm(eng, S, Cf, Lmax, wave, n, stats), "features": FeatureForm(eng, S, Cf, Lmax, x, n),
                     "composed": ComposedForm(eng, S, Cf, Lmax, wave, n, stats, tables), "push": FrontEndForm(S, Cf, wave, stats, tables, "push"),
                     "pop": FrontEndForm(S, Cf, wave, stats, tables, "pop")}
            count = {"audio": launches + 2, "features": launches, "composed": launches + 2 * S, "push": 1, "pop": 1}
            for f in forms.values():
                _timed(f, args.warmup)
            ms = {k: [] for k in forms}
            for _ in range(ROUNDS):
                for k, f in forms.items():
                    ms[k].append(_timed(f, args.steps))
            audio = 10.0 * 4 * Cf * S
            for k in forms:
                t = sorted(ms[k])[ROUNDS // 2]
                lines.append(f"{Cf:2d}  {S:2d}  {k:8s}  {t:7.3f}  {audio:8.1f}  {t / audio:6.4f}  {count[k]:8d}")
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
