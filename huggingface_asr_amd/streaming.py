"""Streaming inference for the causal E-Branchformer + CTC models: the host side of csrc/stream.hip (whose header states the semantics).

    stream = engine.stream(batch=B, chunk_frames=C, max_frames=1500)       # EBranchformerEngine or Wav2Vec2EBranchformerForCTC
    out = stream.feed(feats)            # (B, 4*C, F) fp32 -> dict(logits (B, n_out, V+1), n_out, total, ids (B, n_out) int32 then -1, n_ids (B) int32)
    out = stream.finish(tail, lengths)  # the last 0 .. 4*C frames, per-stream valid counts; flushes the L*r frames of lookahead; adds n_valid / totals (B)

Concatenated over the calls, stream b's logits are those of `engine.forward` on that utterance alone (rounding points of the un-folded layer).  A layer of the
reference's causal model still looks r = (merge_conv_kernel - 1) / 2 frames ahead (depthwise_conv_fusion keeps its symmetric padding), so frame t becomes final only
once the front end has produced frame t + L*r: `plan` gives the per-layer row ranges of a step, the device never reports a count back.

    stream = engine.stream(B, C, 1500, beams=10, nbest=4)      # also walks the CTC prefix beam search over the emitted frames (ops.CtcBeamStream)
    out["beam"]                         # per step: committed / committed_frames (B, max_frames) int32 then -1, n_committed, n_new (B); at finish also the n-best
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


class EncoderStream:
    """State of B streams advanced in lock-step through a causal encoder + CTC head (mi_ebf_stream_step).  Created by `EBranchformerEngine.stream`."""

    def __init__(self, engine, batch: int, chunk_frames: int, max_frames: int, *, beams=None, token_topk=None, nbest=1):
        c = engine.cfg
        if not c.get("is_causal", False):
            raise ValueError("stream(): the model is not causal (is_causal=False): its layers see the whole utterance, there is nothing to stream")
        if engine.precision != "bf16":
            raise NotImplementedError("stream(): precision='fp32' has no streaming path: use the default precision='bf16'")
        if engine.mix or engine.extra:
            raise NotImplementedError("stream(): the BEST-RQ fine-tuning head (finetune_with_layer_mixing / finetune_with_additional_layer) has no streaming path")
        if (c["conv_kernel"][0], c["conv_stride"][0], c["conv_padding"][0]) != (3, 2, 1):
            raise NotImplementedError("stream(): the front-end state is that of the 3 x 3 / stride 2 / padding 1 Conv2d sub-sampling")
        hd = c["hidden_size"] // c["num_attention_heads"]
        if hd not in (16, 64, 128):
            raise NotImplementedError(f"stream(): head size {hd} (mi_attention_chunk_bf16 takes 16, 64, 128)")
        if batch < 1 or chunk_frames < 1 or max_frames < 1 or max_frames > 8192:
            raise ValueError("stream(): batch, chunk_frames >= 1 and 1 <= max_frames <= 8192")
        self.engine, self.B, self.C, self.max_frames = engine, int(batch), int(chunk_frames), int(max_frames)
        self.L = c["num_hidden_layers"]
        self.r = (c.get("merge_conv_kernel", 31) - 1) // 2
        self.F = c.get("num_fbanks", 80)
        self.lookahead = self.L * self.r                # encoder frames between a frame and the last one it depends on
        self.n_feat = 0
        self.total = 0                                  # frames emitted so far (per stream, lock-step)
        self.finished = False
        self._state = None
        self._cs = None
        self.beam = None                                # beams=W: the prefix beam search walks the emitted frames too (ops.CtcBeamStream)
        if beams is not None:
            from . import ops
            self.beam = ops.CtcBeamStream(self.B, self.max_frames, beams=beams, token_topk=token_topk, nbest=nbest, blank=c["vocab_size"], pad_id=-1, dtype=torch.int32,
                                          return_frames=True)
        elif token_topk is not None or nbest != 1:
            raise ValueError("stream(): token_topk and nbest belong to beams=")

    # ------------------------------------------------------------------ state
    def state_bytes(self) -> int:
        return int(_lib.lib().mi_ebf_stream_state_bytes(C.byref(self._config()), self.C, self.max_frames))

    def _config(self):
        if self._cs is None:
            cs = self.engine._config_struct(self.B, SUBSAMPLING * self.C, self.F)
            cs.ln_fold = cs.wide_tiles = cs.branch_overlap = 0
            cs.logits_f32 = 1
            self._cs = cs
        return self._cs

    def _ensure_state(self):
        e = self.engine
        if e._table is None:
            raise RuntimeError("EncoderStream: load_state_dict() on the engine first")
        if self._state is not None and self._version == e.weights_version:
            return
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
        lens = [n] * B if tail_lengths is None else [int(v) for v in (tail_lengths.tolist() if isinstance(tail_lengths, torch.Tensor) else tail_lengths)]
        if len(lens) != B or min(lens) < 0 or max(lens) > n:
            raise ValueError(f"EncoderStream.finish: tail_lengths must be {B} counts in 0..{n}")
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
