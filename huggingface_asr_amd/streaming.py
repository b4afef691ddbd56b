"""Streaming inference for the causal E-Branchformer + CTC models: the host side of csrc/stream.hip (whose header states the semantics).

    stream = engine.stream(batch=B, chunk_frames=C, max_frames=1500)       # EBranchformerEngine or Wav2Vec2EBranchformerForCTC
    out = stream.feed(feats)            # (B, 4*C, F) fp32 -> dict(logits (B, n_out, V+1), n_out, total, ids (B, n_out) int32 then -1, n_ids (B) int32)
    out = stream.finish(tail, lengths)  # the last 0 .. 4*C frames, per-stream valid counts; flushes the L*r frames of lookahead; adds n_valid / totals (B)

Concatenated over the calls, stream b's logits are those of `engine.forward` on that utterance alone (rounding points of the un-folded layer).  A layer of the
reference's causal model still looks r = (merge_conv_kernel - 1) / 2 frames ahead (depthwise_conv_fusion keeps its symmetric padding), so frame t becomes final only
once the front end has produced frame t + L*r: `plan` gives the per-layer row ranges of a step, the device never reports a count back.

    stream = engine.stream(B, C, 1500, beams=10, nbest=4)      # also walks the CTC prefix beam search over the emitted frames (ops.CtcBeamStream)
    out["beam"]                         # per step: committed / committed_frames (B, max_frames) int32 then -1, n_committed, n_new (B); at finish also the n-best

Sessions that start, idle and end on their own share one state as a pool of slots (csrc/stream_pool.hip; `StreamPool`, `pool_table` below):

    pool = engine.stream_pool(slots=S, chunk_frames=C, max_frames=1500)
    sid = pool.open()                   # a free slot, started on the device without touching the others
    out = pool.step(feed={sid: chunk (4*C, F)}, finish={other: tail (0..4*C, F) or None})      # -> {slot: dict(logits (n_out, V+1), ids, n_ids, n_out, total, final)}

The pool walks the same prefix beam search per slot once it is switched on (csrc/ctc_beam_pool.hip; ops.CtcBeamPool), for audio pools too:

    pool = engine.stream_pool(S, C, 1500).with_beams(10, nbest=4)         # before the first open()
    out[sid]["beam"]                    # per step: committed / committed_frames (max_frames) int32 then -1, n_committed, n_new; at finish or with partial= also the n-best

Both take audio instead of feature frames through the stateful log-mel front end (csrc/fbank_stream.hip; `AudioStream`, `AudioPool`, `audio_pieces` below):

    pool = engine.audio_pool(slots=S, chunk_frames=C, max_frames=1500, normalize="global", global_means=m, global_stds=s)
    out = pool.push(audio={sid: samples (n) fp32 / int16, any n}, finish={other: tail or None})  # -> {slot: [the dicts of the steps the slot took]}
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .packing import relative_position_table, rotary_tables

SUBSAMPLING = 4          # product of the two conv strides


def causal_out_frames(n: int) -> int:
    """frames behind the two causal 3 / stride-2 convs after n input frames: frame i of a conv exists once input 2i does"""
    return ((n + 1) // 2 + 1) // 2


def frontiers(n_feat: int, L: int, r: int, finish: bool) -> list:
    """a_0 .. a_L after n_feat feature frames: a_0 = out_frames(n_feat), a_{l+1} = max(0, a_l - r); in `finish` every frontier is a_0"""
    a = [causal_out_frames(n_feat)]
    for _ in range(L):
        a.append(a[-1] if finish else max(0, a[-1] - r))
    return a


def plan(n_feat: int, C: int, L: int, r: int, finish: bool, n_prev: int | None = None) -> list:
    """Row ranges of the step that brings a stream batch from n_prev to n_feat feature frames (n_prev defaults to n_feat - 4*C, a whole chunk; `finish` steps pass it):
    L + 1 pairs (lo, hi) — entry l < L the input rows of layer l, entry L the rows the last layer emits.  Layer l emits entry l + 1.  Pure host arithmetic."""
    if n_prev is None:
        n_prev = n_feat - SUBSAMPLING * C
    if n_prev < 0 or n_prev % (SUBSAMPLING * C) or not 0 <= n_feat - n_prev <= SUBSAMPLING * C or (not finish and n_feat - n_prev != SUBSAMPLING * C):
        raise ValueError(f"plan: a step feeds one chunk of {SUBSAMPLING * C} frames (the last one 0..{SUBSAMPLING * C}) after whole chunks, got {n_prev} -> {n_feat}")
    before, after = frontiers(n_prev, L, r, False), frontiers(n_feat, L, r, finish)
    return list(zip(before, after))


def _check_streamable(engine, n, chunk_frames, max_frames, what, count):
    """the refusals of `engine.stream` / `engine.stream_pool`, before any launch -> engine.cfg"""
    c = engine.cfg
    if not c.get("is_causal", False):
        raise ValueError(f"{what}: the model is not causal (is_causal=False): its layers see the whole utterance, there is nothing to stream")
    if engine.precision != "bf16":
        raise NotImplementedError(f"{what}: precision='fp32' has no streaming path: use the default precision='bf16'")
    if engine.mix or engine.extra:
        raise NotImplementedError(f"{what}: the BEST-RQ fine-tuning head (finetune_with_layer_mixing / finetune_with_additional_layer) has no streaming path")
    if (c["conv_kernel"][0], c["conv_stride"][0], c["conv_padding"][0]) != (3, 2, 1):
        raise NotImplementedError(f"{what}: the front-end state is that of the 3 x 3 / stride 2 / padding 1 Conv2d sub-sampling")
    hd = c["hidden_size"] // c["num_attention_heads"]
    if hd not in (16, 64, 128):
        raise NotImplementedError(f"{what}: head size {hd} (mi_attention_chunk_bf16 takes 16, 64, 128)")
    if n < 1 or chunk_frames < 1 or max_frames < 1 or max_frames > 8192:
        raise ValueError(f"{what}: {count}, chunk_frames >= 1 and 1 <= max_frames <= 8192")
    return c


def _tail_lengths(tail_lengths, B: int, n: int, what: str) -> list:
    """`tail_lengths` of a finish -> B counts in 0..n (default: n each)"""
    lens = [n] * B if tail_lengths is None else [int(v) for v in (tail_lengths.tolist() if isinstance(tail_lengths, torch.Tensor) else tail_lengths)]
    if len(lens) != B or min(lens) < 0 or max(lens) > n:
        raise ValueError(f"{what}: tail_lengths must be {B} counts in 0..{n}")
    return lens


class _StreamState:
    """What `EncoderStream` (n = B streams) and `StreamPool` (n = S slots) hold alike: the geometry of a step, the config struct and the device state of
    mi_ebf_stream_state_bytes / mi_ebf_stream_reset with its position table."""

    def __init__(self, engine, n: int, chunk_frames: int, max_frames: int, what: str, count: str):
        c = _check_streamable(engine, n, chunk_frames, max_frames, what, count)
        self.engine, self._n, self.C, self.max_frames = engine, int(n), int(chunk_frames), int(max_frames)
        self.L = c["num_hidden_layers"]
        self.r = (c.get("merge_conv_kernel", 31) - 1) // 2
        self.F = c.get("num_fbanks", 80)
        self.lookahead = self.L * self.r                # encoder frames between a frame and the last one it depends on
        self._state = self._cs = self._pos = None

    def state_bytes(self) -> int:
        return int(_lib.lib().mi_ebf_stream_state_bytes(C.byref(self._config()), self.C, self.max_frames))

    def _config(self):
        if self._cs is None:
            cs = self.engine._config_struct(self._n, SUBSAMPLING * self.C, self.F)
            cs.ln_fold = cs.wide_tiles = cs.branch_overlap = 0
            cs.logits_f32 = 1
            self._cs = cs
        return self._cs

    def _may_rebuild(self):
        """called before a state is built again because the engine's weights changed: raise to refuse"""

    def _ensure_state(self):
        e = self.engine
        if e._table is None:
            raise RuntimeError(f"{type(self).__name__}: load_state_dict() on the engine first")
        if self._state is not None and self._version == e.weights_version:
            return
        if self._state is not None:
            self._may_rebuild()
        c, dev = e.cfg, e.device
        nbytes = self.state_bytes()
        if nbytes == 0:
            raise RuntimeError("mi_ebf_stream_state_bytes refused the configuration")
        self._state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        d, H = c["hidden_size"], c["num_attention_heads"]
        ptype = c.get("position_embeddings_type", "relative")
        self._pos = None
        if ptype == "relative":       # row `dist` = the sinusoid of relative position +dist: the first max_frames rows of the (2T-1)-row table, reversed
            self._pos = relative_position_table(self.max_frames, d)[: self.max_frames].flip(0).to(dev).to(torch.bfloat16).contiguous()
        elif ptype == "rotary":
            cos, sin = rotary_tables(self.max_frames, d // H, c.get("rotary_embedding_base", 10000))
            self._pos = torch.cat([cos.reshape(-1), sin.reshape(-1)]).to(dev).contiguous()
        self._version = e.weights_version
        self._reset_device()

    def _reset_device(self):
        rc = _lib.lib().mi_ebf_stream_reset(C.byref(self._config()), self.engine._table, self.C, self.max_frames, None if self._pos is None else self._pos.data_ptr(),
                                            self._state.data_ptr(), self._state.numel(), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mi_ebf_stream_reset")


class EncoderStream(_StreamState):
    """State of B streams advanced in lock-step through a causal encoder + CTC head (mi_ebf_stream_step).  Created by `EBranchformerEngine.stream`."""

    def __init__(self, engine, batch: int, chunk_frames: int, max_frames: int, *, beams=None, token_topk=None, nbest=1, bias=None):
        super().__init__(engine, batch, chunk_frames, max_frames, "stream()", "batch")
        engine._check_bias("stream()", bias, beams)     # bias= (ctc_bias.CtcBias): contextual biasing of the beam search; "beam" then holds credit beside the n-best
        self.B, c = self._n, engine.cfg
        self.n_feat = 0
        self.total = 0                                  # frames emitted so far (per stream, lock-step)
        self.finished = False
        self.beam = None                                # beams=W: the prefix beam search walks the emitted frames too (ops.CtcBeamStream)
        if beams is not None:
            from . import ops
            self.beam = ops.CtcBeamStream(self.B, self.max_frames, beams=beams, token_topk=token_topk, nbest=nbest, blank=c["vocab_size"], pad_id=-1, dtype=torch.int32,
                                          return_frames=True, bias=bias)
        elif token_topk is not None or nbest != 1:
            raise ValueError("stream(): token_topk and nbest belong to beams=")

    def reset(self):
        """back to the start of B new streams (histories and caches zero, no carried class)"""
        self.n_feat = self.total = 0
        self.finished = False
        if self._state is not None:
            self._reset_device()
        if self.beam is not None:
            self.beam.reset()

    # ------------------------------------------------------------------ steps
    def _step(self, feats, n_now, finish, ends, partial=False):
        rows = plan(n_now, self.C, self.L, self.r, finish, n_prev=self.n_feat)
        if rows[0][1] > self.max_frames:
            raise RuntimeError(f"EncoderStream: {rows[0][1]} encoder frames exceed max_frames={self.max_frames}")
        if not feats.is_cuda:
            raise RuntimeError("EncoderStream needs device tensors (no CPU fallback)")
        self._ensure_state()
        e, cs = self.engine, self._config()
        B, V1 = self.B, e.cfg["vocab_size"] + 1
        n_out = rows[-1][1] - rows[-1][0]
        dev = e.device
        lbuf = torch.empty((B, n_out, cs.logits_ld), dtype=torch.float32, device=dev)
        best = torch.empty((B, n_out), dtype=torch.int32, device=dev)
        ids = torch.empty((B, n_out), dtype=torch.int32, device=dev)
        n_ids = torch.zeros((B,), dtype=torch.int32, device=dev)
        flat = (C.c_int * (2 * len(rows)))(*[v for lo_hi in rows for v in lo_hi])
        p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        rc = _lib.lib().mi_ebf_stream_step(C.byref(cs), e._table, self.C, self.max_frames, p(self._pos), self._state.data_ptr(), self._state.numel(), feats.data_ptr(),
                                           flat, p(ends), p(lbuf), p(best), p(ids), p(n_ids), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mi_ebf_stream_step")
        out = dict(logits=lbuf[..., :V1], n_out=n_out, total=self.total + n_out, ids=ids, n_ids=n_ids, best=best, rows=rows)
        if self.beam is not None:                       # the step's fp32 logits as they lie in the padded buffer; in finish, rows past a stream's end do not count
            out["beam"] = self.beam.feed(out["logits"], None if ends is None else ends - self.total, final=finish, partial=partial)
        self.n_feat = n_now
        self.total += n_out
        return out

    def _check_open(self, what):
        if self.finished:
            raise RuntimeError(f"EncoderStream.{what}: the streams are finished; reset() starts new ones")

    def feed(self, feats: torch.Tensor, *, partial: bool = False) -> dict:
        """one whole chunk: feats (B, 4*C, F) fp32 -> the frames that became final: dict(logits (B, n_out, V+1) fp32, n_out, total, ids, n_ids, best).  A stream created
        with beams= adds "beam": ops.CtcBeamStream.feed's dict over these frames — the committed tokens (pad -1) and counts, with partial=True also the n-best so far."""
        self._check_open("feed")
        if partial and self.beam is None:
            raise ValueError("EncoderStream.feed: partial=True asks for the beam search's n-best: create the stream with beams=")
        want = (self.B, SUBSAMPLING * self.C, self.F)
        if tuple(feats.shape) != want:
            raise ValueError(f"EncoderStream.feed: a chunk is {want} (batch, 4 * chunk_frames, features), got {tuple(feats.shape)}; the last, shorter piece goes to finish()")
        return self._step(feats.to(torch.float32).contiguous(), self.n_feat + SUBSAMPLING * self.C, False, None, partial)

    def finish(self, tail: torch.Tensor | None = None, tail_lengths=None) -> dict:
        """the last 0 .. 4*C frames of every stream (tail (B, n, F), n <= 4*C; tail_lengths (B): valid frames of each stream, default n) and the flush: every frame
        still inside the lookahead becomes final.  Adds n_valid (B): how many of the n_out rows are frames of stream b, and totals (B) = out_frames(frames of stream b).
        With beams=, "beam" holds the full n-best of every stream (tokens (B, nbest, max_frames) int32 then -1, n_tokens, scores, frames) and its committed buffers, which
        now equal hypothesis 0."""
        self._check_open("finish")
        B, W = self.B, SUBSAMPLING * self.C
        n = 0 if tail is None else int(tail.shape[1])
        if tail is not None and (tail.dim() != 3 or tail.shape[0] != B or tail.shape[2] != self.F or n > W):
            raise ValueError(f"EncoderStream.finish: the tail is ({B}, 0..{W}, {self.F}), got {tuple(tail.shape)}")
        lens = _tail_lengths(tail_lengths, B, n, "EncoderStream.finish")
        dev = self.engine.device
        buf = torch.zeros((B, W, self.F), dtype=torch.float32, device=dev)
        if n:
            keep = torch.arange(n, device=dev)[None, :, None] < torch.tensor(lens, device=dev)[:, None, None]
            buf[:, :n] = tail.to(device=dev, dtype=torch.float32) * keep          # frames beyond a stream's end never reach a conv
        ends = [causal_out_frames(self.n_feat + v) for v in lens]
        if max(ends) > self.max_frames:
            raise RuntimeError(f"EncoderStream: {max(ends)} encoder frames exceed max_frames={self.max_frames}")
        base = self.total
        out = self._step(buf, self.n_feat + max(lens), True, torch.tensor(ends, dtype=torch.int32, device=dev))
        self.finished = True
        out["totals"] = torch.tensor(ends, dtype=torch.int32)
        out["n_valid"] = out["totals"] - base
        return out


# ---------------------------------------------------------------------------------------------------- session pool (csrc/stream_pool.hip states the semantics)
def pool_table(actions, C: int, L: int, r: int):
    """The descriptor records of one pool step.  actions: the active slots in order, each (slot, n_prev, n, finish) — the slot has had n_prev feature frames and now gets n
    (a whole chunk of 4*C, or as `finish` a tail of 0 .. 4*C).  -> (records, totals): record i = [slot, end, lo_0, hi_0, off_0, .. lo_L, hi_L, off_L] with (lo_l, hi_l) =
    plan(n_prev + n, C, L, r, finish, n_prev=n_prev)[l] of that slot alone (in a finish the frontiers are its own end), off_l the sum of the earlier records' hi_l - lo_l
    (the slot's first row in the step's compact buffers), end = the slot's frame count when it finishes, else -1; totals[l] = the rows of all records at entry l.
    Pure host arithmetic."""
    totals = [0] * (L + 1)
    records = []
    for slot, n_prev, n, finish in actions:
        rows = plan(n_prev + n, C, L, r, bool(finish), n_prev=n_prev)
        rec = [int(slot), rows[0][1] if finish else -1]
        for l, (lo, hi) in enumerate(rows):
            rec += [lo, hi, totals[l]]
            totals[l] += hi - lo
        records.append(rec)
    return records, totals


class StreamPool(_StreamState):
    """S slots over one stream state, each a session with a position of its own: `open` a slot, `step` any subset of the open slots — each feeds a chunk or finishes, the
    others stay idle and untouched —, a finished slot is free again.  Created by `EBranchformerEngine.stream_pool`.

        pool = engine.stream_pool(slots=16, chunk_frames=C, max_frames=1500)
        sid = pool.open()
        out = pool.step(feed={sid: chunk (4*C, F)}, finish={other: tail (0..4*C, F) or None})      # -> {sid: dict(logits (n_out, V+1) fp32, ids, n_ids, total, final)}

    Concatenated over its calls, a session's logits and ids are those of `engine.stream(1, C, max_frames)` fed the same pieces, whatever the other slots do."""

    def __init__(self, engine, slots: int, chunk_frames: int, max_frames: int, *, beams=None):
        super().__init__(engine, slots, chunk_frames, max_frames, "stream_pool()", "slots")
        if beams is not None:
            raise NotImplementedError("stream_pool(): beams= is not a constructor keyword of the pool: the prefix beam search per slot is switched on by a method, "
                                      "stream_pool(...).with_beams(beams, token_topk=None, nbest=1), before the first session is opened")
        self.S = self._n
        self.is_open = [False] * self.S
        self.n_feat = [0] * self.S                      # feature frames the slot's session has had
        self.total = [0] * self.S                       # frames it has emitted
        self.beam = None                                # with_beams(): the prefix beam search walks every slot's emitted frames too (ops.CtcBeamPool)

    def with_beams(self, beams, *, token_topk=None, nbest=1, bias=None):
        """Switches on the CTC prefix beam search per slot (ops.CtcBeamPool, csrc/ctc_beam_pool.hip) -> the pool itself.  Every session then walks `beams` (1..64)
        hypotheses over the `token_topk` best classes of the frames it emits, as `engine.stream(1, C, max_frames, beams=, token_topk=, nbest=)` would for the same
        pieces — bit for bit —, and `step` adds "beam" to every named slot's dict.  Allowed only while no session is open (RuntimeError); the checks are those of
        `engine.stream(beams=)` (ValueError / TypeError; max_frames * beams < 2^22 - 2).  Nothing is allocated before the first device step.  Per step the beam adds
        two kernels (the token cut over the step's compact logits and one walk block per named slot), one small copy (the step's counts) and no transfer: its records
        ride behind the descriptor table.  bias (a ctc_bias.CtcBias): contextual biasing, one context for the pool, shared by all slots (csrc/ctc_beam_bias_pool.hip);
        a slot's "beam" then holds credit (nbest) beside its n-best."""
        self.engine._check_bias("with_beams", bias, beams)
        if any(self.is_open):
            raise RuntimeError("StreamPool.with_beams: sessions are open; the beam search is switched on before the first open()")
        from . import ops
        self.beam = ops.CtcBeamPool(self.S, self.max_frames, beams=beams, token_topk=token_topk, nbest=nbest, blank=self.engine.cfg["vocab_size"], pad_id=-1,
                                    dtype=torch.int32, return_frames=True, bias=bias)
        return self

    def _may_rebuild(self):
        if any(self.is_open):
            raise RuntimeError("StreamPool: the engine's weights changed while sessions were open")

    # ------------------------------------------------------------------ sessions
    def open(self) -> int:
        """-> a free slot, started: zero histories and rings, no carried class (a per-slot reset on the device, enqueued on the current stream); after with_beams()
        also the slot's beam at its start and its committed row cleared"""
        free = [s for s in range(self.S) if not self.is_open[s]]
        if not free:
            raise RuntimeError(f"StreamPool.open: all {self.S} slots hold open sessions")
        sid = free[0]
        if self.engine._table is not None and torch.device(self.engine.device).type == "cuda":      # else: no state yet — it is created whole, every slot at a stream start
            self._ensure_state()
            rc = _lib.lib().mi_ebf_stream_reset_slot(C.byref(self._config()), self.C, self.max_frames, self._state.data_ptr(), self._state.numel(), sid,
                                                     torch.cuda.current_stream().cuda_stream)
            _lib.check(rc, "mi_ebf_stream_reset_slot")
        if self.beam is not None:
            self.beam.open(sid)
        self.is_open[sid] = True
        self.n_feat[sid] = self.total[sid] = 0
        return sid

    def _check_named(self, sid, first, finish, what, first_name):
        """slot `sid` of a step's or push's two dicts: named once, and holding an open session"""
        if sid in first and sid in finish:
            raise ValueError(f"{what}: slot {sid} is named in both {first_name} and finish")
        if not isinstance(sid, int) or not 0 <= sid < self.S or not self.is_open[sid]:
            raise RuntimeError(f"{what}: slot {sid} holds no open session (free or finished): open() starts one")

    def actions(self, feed=None, finish=None):
        """the checked actions of a step, ordered by slot -> [(slot, n_prev, n, finish, tensor or None)]"""
        feed, finish = dict(feed or {}), dict(finish or {})
        W = SUBSAMPLING * self.C
        acts = []
        for sid in sorted(set(feed) | set(finish)):
            self._check_named(sid, feed, finish, "StreamPool.step", "feed")
            if sid in feed:
                x = feed[sid]
                if x is None or tuple(x.shape) != (W, self.F):
                    raise ValueError(f"StreamPool.step: a chunk is ({W}, {self.F}) (4 * chunk_frames, features), got {None if x is None else tuple(x.shape)}; the last, "
                                     "shorter piece goes to finish=")
                n = W
            else:
                x = finish[sid]
                n = 0 if x is None else int(x.shape[0])
                if x is not None and (x.dim() != 2 or x.shape[1] != self.F or n > W):
                    raise ValueError(f"StreamPool.step: the tail is (0..{W}, {self.F}), got {tuple(x.shape)}")
            self._check_room(sid, self.n_feat[sid] + n)
            acts.append((sid, self.n_feat[sid], n, sid in finish, x))
        return acts

    def _check_room(self, sid, n_feat):
        if causal_out_frames(n_feat) > self.max_frames:
            raise RuntimeError(f"StreamPool: {causal_out_frames(n_feat)} encoder frames of slot {sid} exceed max_frames={self.max_frames}")

    def _advance(self, acts, records):
        """host bookkeeping after a step -> per slot (n_out, total, final)"""
        res = {}
        for (sid, n_prev, n, fin, _), rec in zip(acts, records):
            n_out = rec[-2] - rec[-3]
            self.n_feat[sid] = n_prev + n
            self.total[sid] += n_out
            res[sid] = (n_out, self.total[sid], fin)
            if fin:
                self.is_open[sid] = False
        return res

    def _partial(self, partial, what):
        """`partial` of step / push -> None (nobody), True (every named slot) or the set of slot ids"""
        if partial is None or partial is False:
            return None
        if self.beam is None:
            raise ValueError(f"{what}: partial asks for the beam search's n-best: switch it on with with_beams() first")
        if partial is True:
            return True
        if isinstance(partial, (str, bytes, torch.Tensor)) or not hasattr(partial, "__iter__"):
            raise TypeError(f"{what}: partial is True or a collection of slot ids")
        ids = set(partial)
        if not all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v < self.S for v in ids):
            raise ValueError(f"{what}: partial names slots in [0, {self.S}), got {sorted(ids, key=repr)}")
        return ids

    def step(self, feed=None, finish=None, partial=False) -> dict:
        """feed {slot: chunk (4*C, F)}, finish {slot: tail (0..4*C, F) or None}; every other slot is idle.  -> {slot: dict(logits (n_out, V+1) fp32, ids (n_out) int32 =
        the greedy tokens newly emitted then -1, n_ids (0-d int32), n_out, total, final)} for the named slots.  A finished slot is free after the call.
        After with_beams() every named slot's dict also holds "beam": dict(committed (max_frames) int32 then -1, committed_frames, n_committed, n_new (0-d int32)) — the
        tokens every hypothesis of the slot's beam begins with, the frame each entered at, how many there are and how many this step appended.  committed and
        committed_frames are VIEWS of the pool's row for that slot: append-only during a session — the first n_committed entries of a step never change, later steps
        write behind them — and reset by the slot's next session (open()), so copy what must outlive that.  The two counts are the step's own.  For a finishing slot, and for those `partial` names (True: every named slot; or a collection of slot ids), "beam" also holds the n-best: tokens (nbest, max_frames)
        int32 then -1, n_tokens (nbest), scores (nbest) fp32, frames (nbest, max_frames); after a finish committed[:n_committed] is hypothesis 0."""
        partial = self._partial(partial, "StreamPool.step")
        acts = self.actions(feed, finish)
        if not acts:
            return {}
        e = self.engine
        if not torch.device(e.device).type == "cuda" or any(a[4] is not None and not a[4].is_cuda for a in acts):
            raise RuntimeError("StreamPool needs device tensors (no CPU fallback)")
        dev, W = e.device, SUBSAMPLING * self.C
        zero = lambda n: torch.zeros((n, self.F), dtype=torch.float32, device=dev)
        feats = torch.stack([x.to(torch.float32) if n == W else (zero(W) if n == 0 else torch.cat([x.to(torch.float32), zero(W - n)])) for _, _, n, _, x in acts])   # a tail zero-padded
        return self._run(acts, feats, partial)

    def _run(self, acts, feats, partial=None) -> dict:
        """the step of checked actions [(slot, n_prev, n, finish, _)] on their compact chunks feats (A, 4*C, F) fp32, tails zero-padded (AudioPool hands over
        fbank.FbankStream.pop's buffer as it is); partial: `_partial`'s None, True or set of slots"""
        e = self.engine
        if not torch.device(e.device).type == "cuda":
            raise RuntimeError("StreamPool needs device tensors (no CPU fallback)")
        self._ensure_state()
        dev, cs, lib = e.device, self._config(), _lib.lib()
        W, A, V1 = SUBSAMPLING * self.C, len(acts), e.cfg["vocab_size"] + 1
        records, totals = pool_table([a[:4] for a in acts], self.C, self.L, self.r)
        rec = torch.tensor(records, dtype=torch.int32)
        words = lib.mi_ebf_stream_slots_table(C.byref(cs), self.C, self.max_frames, rec.data_ptr(), A, None, 0)
        _lib.check(min(words, 0), "mi_ebf_stream_slots_table")
        n_out = totals[-1]
        brecs = None
        if self.beam is not None:                       # a slot's rows in the step's compact logits: (off_L, hi_L - lo_L) of its record; checked before any launch
            wanted = lambda sid: partial is True or (partial is not None and sid in partial)
            beam_in = [(a[0], r[-1], r[-2] - r[-3], bool(a[3]), wanted(a[0])) for a, r in zip(acts, records)]
            brecs, _ = self.beam.records(beam_in, n_out)
        extra = 0 if brecs is None else A * self.beam.REC_WORDS
        host = torch.empty((words + extra,), dtype=torch.int32, pin_memory=True)
        _lib.check(min(lib.mi_ebf_stream_slots_table(C.byref(cs), self.C, self.max_frames, rec.data_ptr(), A, host.data_ptr(), words), 0), "mi_ebf_stream_slots_table")
        if extra:
            host[words:] = torch.tensor(brecs, dtype=torch.int32).reshape(-1)      # the beam's records ride behind the table
        table = host.to(dev, non_blocking=True)         # the step's one host-to-device transfer
        lbuf = torch.empty((n_out, cs.logits_ld), dtype=torch.float32, device=dev)
        best = torch.empty((n_out,), dtype=torch.int32, device=dev)
        ids = torch.empty((n_out,), dtype=torch.int32, device=dev)
        n_ids = torch.zeros((A,), dtype=torch.int32, device=dev)
        p = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        rc = lib.mi_ebf_stream_step_slots(C.byref(cs), e._table, self.C, self.max_frames, p(self._pos), self._state.data_ptr(), self._state.numel(), feats.data_ptr(),
                                          rec.data_ptr(), A, table.data_ptr(), words, p(lbuf), p(best), p(ids), n_ids.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mi_ebf_stream_step_slots")
        bout = None if self.beam is None else self.beam.step(lbuf[:, :V1], beam_in, records_dev=table[words:])
        counts = None if bout is None else torch.stack((bout["n_committed"], bout["n_new"]))      # this step's own copy: a push may run several steps before it returns
        out = {}
        for i, (sid, (n, total, fin)) in enumerate(self._advance(acts, records).items()):
            off = records[i][-1]
            out[sid] = dict(logits=lbuf[off:off + n, :V1], ids=ids[off:off + n], n_ids=n_ids[i], best=best[off:off + n], n_out=n, total=total, final=fin)
            if bout is not None:
                b = dict(committed=bout["committed"][sid], committed_frames=bout["committed_frames"][sid], n_committed=counts[0, sid], n_new=counts[1, sid])
                if sid in bout["rows"]:
                    row = bout["rows"][sid]
                    b.update(tokens=bout["tokens"][row], n_tokens=bout["n_tokens"][row], scores=bout["scores"][row], frames=bout["frames"][row])
                    if "credit" in bout:
                        b["credit"] = bout["credit"][row]
                out[sid]["beam"] = b
        return out


# ---------------------------------------------------------------------------------------------------- audio in (csrc/fbank_stream.hip states the front end's semantics)
SAMPLE_RATE, HOP_SAMPLES = 16000, 160


def seconds(frame: int) -> float:
    """start time of encoder frame `frame` in its session's audio: a frame is 4 feature frames of 160 samples at 16 kHz"""
    return frame * SUBSAMPLING * HOP_SAMPLES / SAMPLE_RATE


def audio_pieces(n_prev: int, n_new, fed: int, C: int, finish: bool = False) -> list:
    """The steps that a push of n_new samples brings about in a stream that has had n_prev samples and has fed `fed` of its feature frames to the encoder:
    -> [(lo, hi, finish)], the feature frames [lo, hi) of each step in order.  Pure host arithmetic; AudioStream and AudioPool run exactly these steps, and a stream
    fed features directly in these pieces gives the same bits.
      * a stream that goes on feeds one whole chunk of 4*C frames for as long as it holds that many unfed frames (fbank.num_frames(n_prev + n_new) - fed of them);
      * a stream that finishes with R unfed frames feeds k = max(0, ceil(R / 4C) - 1) whole chunks and finishes with the remaining 0 .. 4*C frames (R > 0: 1 .. 4*C);
      * lock-step streams end inside one call: n_new is then the list of every stream's last sample count (finish only), k is taken from the largest R_b, the finish
        step's hi is the list of every stream's end, and min R_b >= 4*C*k is required — else ValueError: a stream that ends more than a chunk before another cannot
        share its steps; the session pool (audio_pool) lets every session end on its own."""
    from .fbank import num_frames
    W = SUBSAMPLING * C
    lock = not isinstance(n_new, int)
    news = [int(v) for v in n_new] if lock else [n_new]
    if lock and not finish:
        raise ValueError("audio_pieces: per-stream sample counts belong to the finishing call (lock-step streams are pushed equal counts before it)")
    if n_prev < 0 or fed < 0 or fed % W or not news or min(news) < 0:
        raise ValueError(f"audio_pieces: counts >= 0 and whole chunks fed, got n_prev={n_prev}, n_new={n_new}, fed={fed}")
    ready = [num_frames(n_prev + n) - fed for n in news]
    if min(ready) < 0:
        raise ValueError(f"audio_pieces: {fed} frames fed, but {n_prev} + {min(news)} samples hold only {min(ready) + fed}")
    k = max(0, -(-max(ready) // W) - 1) if finish else ready[0] // W
    if min(ready) < W * k:
        raise ValueError(f"audio_pieces: lock-step streams end inside one call, but they hold {ready} unfed frames: the longest still feeds {k} whole chunk(s) of {W} "
                         f"frames that the shortest does not have.  Sessions of lengths this far apart belong in the session pool (audio_pool), where each ends on its own")
    steps = [(fed + i * W, fed + (i + 1) * W, False) for i in range(k)]
    if finish:
        ends = [fed + R for R in ready]
        steps.append((fed + k * W, ends if lock else ends[0], True))
    return steps


def extractor_settings(feature_extractor, num_fbanks: int) -> dict:
    """what a `CustomFeatureExtractor` asks of the streaming front end -> dict(normalize, global_means, global_stds, tables); refuses what cannot stream"""
    fe = feature_extractor
    if getattr(fe, "norm_type", None) == "utterance" and getattr(fe, "do_ceptral_normalize", False):
        raise NotImplementedError("audio streaming: the feature extractor normalises per utterance (norm_type='utterance' with do_ceptral_normalize): utterance CMVN needs "
                                  "the whole utterance, so it cannot stream; global statistics (norm_type='global') or no normalisation stream exactly")
    if fe.feature_size != num_fbanks:
        raise ValueError(f"audio streaming: the feature extractor gives feature_size={fe.feature_size} values per frame, the model takes num_fbanks={num_fbanks}")
    if getattr(fe, "norm_type", None) == "global":
        return dict(normalize="global", global_means=fe.global_means, global_stds=fe.global_stds, tables=fe._get_tables())
    return dict(normalize=None, tables=fe._get_tables())


def _front_end(engine, slots, C, F, normalize, global_means, global_stds, max_push_samples, tables, what):
    from .fbank import FbankStream, FbankTables
    tables = FbankTables(F) if tables is None else tables
    if tables.num_mel != F:
        raise ValueError(f"{what}: the filterbank gives {tables.num_mel} values per frame (feature_size), the model takes num_fbanks={F}")
    W = SUBSAMPLING * C
    return FbankStream(slots, W, 2 * W * HOP_SAMPLES if max_push_samples is None else max_push_samples, tables, normalize=normalize, global_means=global_means,
                       global_stds=global_stds, device=engine.device)


def _drive(fb, flat, spans, queues, run, lockstep=False):
    """Pushes spans {slot: (offset, n)} of `flat` in pieces of at most fb.max_push samples — one launch per piece for all slots — and after each piece calls
    run({slot: (lo, hi, finish)}) for as long as some slot's next step (queues: audio_pieces' lists) has its frames; a finish step waits for the slot's last sample.
    lockstep: only when every slot is due.  The ring never overruns: a slot holds at most 4*C unfed frames before a piece."""
    done = {s: 0 for s in spans}
    if torch.device(fb.device).type == "cuda":
        flat = flat.to(fb.device)                       # a host tensor is copied once, by torch, not once per piece
    while True:
        piece = {s: (off + done[s], min(fb.max_push, n - done[s])) for s, (off, n) in spans.items() if n > done[s]}
        if piece:
            fb.push_flat(flat, piece)
            for s, (_, n) in piece.items():
                done[s] += n
        while True:
            due = {s: q[0] for s, q in queues.items() if q and q[0][1] <= fb.frames(s) and (not q[0][2] or done[s] == spans[s][1])}
            if not due or (lockstep and len(due) < sum(1 for q in queues.values() if q)):
                break
            run(due)
            for s in due:
                queues[s].pop(0)
        if not piece:
            return


class AudioStream:
    """`EncoderStream` fed audio: B lock-step streams take samples in pieces of any size (the same count for all), the stateful log-mel front end (fbank.FbankStream)
    turns them into the features `fbank_gpu` gives for the whole utterance — bit for bit — and the wrapped stream is fed the chunks `audio_pieces` names.  Created by
    `EBranchformerEngine.audio_stream`.

        s = engine.audio_stream(B, C, 1500, normalize="global", global_means=m, global_stds=sd)
        outs = s.push(samples (B, n))                   # fp32 in [-1, 1] or int16 PCM, host or device, any n >= 0 -> the feed() dicts of the steps it ran (maybe none)
        outs = s.finish(tail (B, n) or None, lengths)   # -> the step dicts, the last one finish()'s

    The reference's dataloader-side `default_transform` (strip leading / trailing zero samples, pad to 8000) is an utterance-level step and no part of a stream: the
    offline equivalent of a streamed session is `extract_on_device(..., default_transform=False)`."""

    def __init__(self, engine, batch, chunk_frames, max_frames, *, normalize=None, global_means=None, global_stds=None, beams=None, token_topk=None, nbest=1,
                 max_push_samples=None, tables=None, bias=None):
        self.stream = EncoderStream(engine, batch, chunk_frames, max_frames, beams=beams, token_topk=token_topk, nbest=nbest, bias=bias)
        self.B, self.C = self.stream.B, self.stream.C
        self.fb = _front_end(engine, self.B, self.C, self.stream.F, normalize, global_means, global_stds, max_push_samples, tables, "audio_stream()")
        self.n = 0                                      # samples every stream has had
        for b in range(self.B):
            self.fb.open(b)

    seconds = staticmethod(seconds)

    def reset(self):
        self.stream.reset()
        self.n = 0
        for b in range(self.B):
            self.fb.open(b)

    def _samples(self, x, what):
        from .fbank import check_samples
        check_samples(x, what)
        if x.dim() != 2 or x.shape[0] != self.B:
            raise ValueError(f"{what}: audio is ({self.B}, n) samples, the same n for every stream, got {tuple(x.shape)}")
        return x.contiguous()

    def _room(self, n_samples):
        from .fbank import num_frames
        if causal_out_frames(num_frames(n_samples)) > self.stream.max_frames:
            raise RuntimeError(f"AudioStream: {causal_out_frames(num_frames(n_samples))} encoder frames exceed max_frames={self.stream.max_frames}")

    def _run(self, flat, n, lens, steps):
        W, outs = SUBSAMPLING * self.C, []
        queues = {b: [(lo, hi[b] if isinstance(hi, list) else hi, fin) for lo, hi, fin in steps] for b in range(self.B)}

        def run(due):
            lo, _, fin = due[0]
            if not fin:
                outs.append(self.stream.feed(self.fb.pop([(b, W) for b in range(self.B)])))
            else:
                tails = [due[b][1] - lo for b in range(self.B)]
                feats = self.fb.pop([(b, tails[b]) for b in range(self.B)])
                outs.append(self.stream.finish(feats[:, :max(tails)], tails))
        _drive(self.fb, flat, {b: (b * n, lens[b]) for b in range(self.B)}, queues, run, lockstep=True)
        return outs

    def push(self, samples: torch.Tensor) -> list:
        """samples (B, n), any n >= 0 -> the feed() dicts of the whole chunks that became ready, in order (an empty list when none did)"""
        self.stream._check_open("feed")
        samples = self._samples(samples, "AudioStream.push")
        n = int(samples.shape[1])
        self._room(self.n + n)
        steps = audio_pieces(self.n, n, self.stream.n_feat, self.C)
        outs = self._run(samples.reshape(-1), n, [n] * self.B, steps)
        self.n += n
        return outs

    def finish(self, tail: torch.Tensor | None = None, tail_lengths=None) -> list:
        """the last samples of every stream (tail (B, n) or None; tail_lengths (B): valid samples of each stream, default n) and the flush -> the dicts of the steps:
        whole chunks first (feed()'s), then finish()'s.  Streams whose ends lie more than a chunk apart raise ValueError before any launch (audio_pieces)."""
        self.stream._check_open("finish")
        if tail is None:
            tail = torch.zeros((self.B, 0), dtype=torch.float32)
        tail = self._samples(tail, "AudioStream.finish")
        n = int(tail.shape[1])
        lens = _tail_lengths(tail_lengths, self.B, n, "AudioStream.finish")
        self._room(self.n + max(lens))
        steps = audio_pieces(self.n, lens, self.stream.n_feat, self.C, finish=True)
        return self._run(tail.reshape(-1), n, lens, steps)


class AudioPool:
    """`StreamPool` fed audio: sessions that start and end on their own push samples in pieces of any size.  Created by `EBranchformerEngine.audio_pool`.

        pool = engine.audio_pool(S, C, 1500, normalize="global", global_means=m, global_stds=sd)
        sid = pool.open()
        out = pool.push(audio={sid: samples (n)}, finish={other: tail (n) or None})     # -> {sid: [StreamPool.step's dicts of the steps the slot took, maybe none]}

    One push launch covers all named slots; `StreamPool`'s step then runs as often as some slot has a step due (`audio_pieces`), each time over exactly the slots that
    are due, their chunks gathered by one pop.  A session's logits and ids are bit for bit those of `engine.stream(1, ...)` fed `fbank_gpu`'s features of its whole
    audio in the same pieces."""

    def __init__(self, engine, slots, chunk_frames, max_frames, *, normalize=None, global_means=None, global_stds=None, beams=None, max_push_samples=None, tables=None):
        self.pool = StreamPool(engine, slots, chunk_frames, max_frames, beams=beams)
        self.S, self.C = self.pool.S, self.pool.C
        self.fb = _front_end(engine, self.S, self.C, self.pool.F, normalize, global_means, global_stds, max_push_samples, tables, "audio_pool()")

    seconds = staticmethod(seconds)

    def with_beams(self, beams, *, token_topk=None, nbest=1, bias=None):
        """`StreamPool.with_beams` on the wrapped pool -> this pool: every step dict of a slot then holds "beam"; `push(..., partial=)` asks for the n-best so far"""
        self.pool.with_beams(beams, token_topk=token_topk, nbest=nbest, bias=bias)
        return self

    def open(self) -> int:
        sid = self.pool.open()
        self.fb.open(sid)
        return sid

    def push(self, audio=None, finish=None, partial=False) -> dict:
        """audio {slot: samples (n)}, finish {slot: tail (n) or None} -> {slot: [StreamPool.step's dicts of the steps the slot took]}.  partial (after with_beams():
        True or a collection of slot ids) goes to every step the push runs: those slots' "beam" dicts then hold the n-best so far."""
        from .fbank import num_frames
        partial = self.pool._partial(partial, "AudioPool.push")
        audio, finish = dict(audio or {}), dict(finish or {})
        pieces = {}
        for sid in sorted(set(audio) | set(finish)):
            self.pool._check_named(sid, audio, finish, "AudioPool.push", "audio")
            pieces[sid] = audio[sid] if sid in audio else finish[sid]
        if not pieces:
            return {}
        given = [x for x in pieces.values() if x is not None]
        none = torch.zeros(0, dtype=given[0].dtype if given and isinstance(given[0], torch.Tensor) else torch.float32)      # a missing tail takes the call's dtype
        pieces = {sid: none if x is None else x for sid, x in pieces.items()}
        flat, spans = self.fb.flatten(pieces, "AudioPool.push")
        queues = {}
        for sid, (_, n) in spans.items():
            self.pool._check_room(sid, num_frames(self.fb.n[sid] + n))
            queues[sid] = audio_pieces(self.fb.n[sid], n, self.pool.n_feat[sid], self.C, finish=sid in finish)
        out = {sid: [] for sid in pieces}

        def run(due):
            sids = sorted(due)
            acts = [(sid, self.pool.n_feat[sid], due[sid][1] - due[sid][0], due[sid][2], None) for sid in sids]
            res = self.pool._run(acts, self.fb.pop([(a[0], a[2]) for a in acts]), partial)
            for sid in sids:
                out[sid].append(res[sid])
        _drive(self.fb, flat, spans, queues, run)
        return out
