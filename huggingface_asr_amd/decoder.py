"""GPT-2 cross-attention decoder + joint CTC/attention forward on the HIP kernels.

Host-side orchestration (one C-ABI call per op) of
  * reference `src/models/decoders/multi_head_gpt2.py:80-170` (GPT2LMMultiHeadModel: auxiliary lm heads on intermediate
    hidden states, shifted label-smoothed CE),
  * the transformers GPT-2 block it inherits (ln_1 -> causal self-attn -> ln_cross_attn -> cross-attn over the encoder
    frames -> ln_2 -> gelu_new MLP; Conv1D weights are stored (in, out) and are transposed once at pack time),
  * reference `src/models/embeddings.py` (fixed sinusoidal positions + sqrt(d)-scaled embedding when `pos_emb_fixed`),
  * reference `src/models/ctc_encoder_plus_autoregressive_decoder.py:237-358` (JointAED: encoder CTC loss, enc_to_dec_proj,
    cross mask from the OUTER length formula, shift_tokens_right, loss = w*CTC + (1-w)*CE).
Eval-mode semantics; the fp32 residual stream / bf16 GEMM operands precision model is the encoder's.
`precision="fp32"` (engine.py's switch, DESIGN.md §4 'fp32 inference mode'): every packed tensor, the cross K/V tables, the KV cache and the token step stay fp32
(csrc/decoder_f32.hip) — what the reference's decode recipes, which carry no --bf16, compute.
"""
from __future__ import annotations

import ctypes as C
import time

import torch

from . import _lib, ops, ops_f32
from .engine import PRECISIONS, EBranchformerEngine
from .packing import _dec_map, _lm_map, decoder_specs, head_fold, head_taps, lm_specs, mapped_fp32, mixes_heads, packed

BF16 = torch.bfloat16


def _sinusoid_table(n: int, d: int, device) -> torch.Tensor:
    """rows [0, n) of the fixed sinusoidal positions (reference src/models/embeddings.py:65-90); row i does not depend on n"""
    inv = 1 / (10000 ** (torch.arange(0.0, d, 2.0) / d))
    s = torch.outer(torch.arange(n).float(), inv)
    return torch.cat([s.sin(), s.cos()], -1).to(device).contiguous()


def _check_precision(who: str, precision: str) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"{who}: precision must be one of {PRECISIONS}, got {precision!r}")
    return precision


class GPT2DecoderEngine:
    precision = "bf16"          # (engines that build themselves without this constructor run the default mode)

    def __init__(self, cfg: dict, device="cuda:0", precision="bf16"):
        self.precision = _check_precision("GPT2DecoderEngine", precision)
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        if precision == "fp32" and mixes_heads(cfg):
            raise NotImplementedError("precision='fp32' does not cover the mixing decoder (GPT2LMMultiHeadModelMixing's mixing_mode, average_logits: the folded multi-tap "
                                      "head): use the default precision='bf16'")
        d, H = cfg["n_embd"], cfg["n_head"]
        if d // H not in (64, 128):
            raise NotImplementedError("HIP decoder attention supports head sizes 64 and 128 (the reference's GPT-2 configs use 64)")
        if cfg.get("activation_function", "gelu_new") != "gelu_new":
            raise NotImplementedError("decoder MLP activation other than gelu_new")
        self.w = None

    # ------------------------------------------------------------------ weights
    def load_state_dict(self, sd: dict, prefix: str = "decoder."):
        """every packed parameter of packing.decoder_specs (Conv1D weights transposed to (out, in) there), matrices in bf16, the rest in fp32.
        precision="fp32": the same tensors in the same slots, every one of them fp32; a tied head is `wte` itself."""
        c, dev = self.cfg, self.device
        f32 = self.precision == "fp32"
        d, L = c["n_embd"], c["n_layer"]
        m = _dec_map(c, False, prefix)
        specs = decoder_specs(c, d, False)
        F = {s.name: t for s, t in packed(specs, m, mapped_fp32(m, sd, dev))}               # fp32 on the device: what the head fold reads
        P = {s.name: (F[s.name].to(BF16) if s.mat and s.name != "wte" and not f32 else F[s.name]).contiguous() for s in specs}      # wte stays fp32: the embedding gather reads it
        fixed = c.get("pos_emb_fixed", False)
        w = dict(wte=P["wte"], scale=float(d) ** 0.5 if fixed else 1.0, pos=_sinusoid_table(c.get("n_positions", 1024), d, dev) if fixed else P["wpe"],
                 lnf=(P["lnf_g"], P["lnf_b"]), heads=[P[f"head{k}"] for k in range(len(c.get("head_locations") or []))],
                 lm_head=P["lm_head"] if "lm_head" in P else (P["wte"] if f32 else P["wte"].to(BF16)))      # tied: the token embedding is the head
        w["layers"] = [dict({n: P[f"h{l}.{n}"] for n in ("wqkv", "bqkv", "wo", "bo", "wq", "bq", "wkv", "bkv", "wco", "bco", "wfc", "bfc", "wpr", "bpr")},
                            **{n: (P[f"h{l}.{n}_g"], P[f"h{l}.{n}_b"]) for n in ("ln1", "lnc", "ln2")}) for l in range(L)]
        self.w = w
        # pointer table of mi_gpt2_step (csrc/decoder_step.hip): 5 globals, then 18 per layer
        ptrs = [w["wte"], w["pos"], w["lnf"][0], w["lnf"][1], w["lm_head"]]
        for lw in w["layers"]:
            ptrs += [lw["ln1"][0], lw["ln1"][1], lw["wqkv"], lw["bqkv"], lw["wo"], lw["bo"], lw["lnc"][0], lw["lnc"][1], lw["wq"], lw["bq"],
                     lw["wco"], lw["bco"], lw["ln2"][0], lw["ln2"][1], lw["wfc"], lw["bfc"], lw["wpr"], lw["bpr"]]
        self._wtable = (C.c_void_p * len(ptrs))(*[t.data_ptr() for t in ptrs])
        self._gcfg = _lib.Gpt2Config(d=d, H=c["n_head"], L=L, V=w["lm_head"].shape[0], eps=float(c.get("layer_norm_epsilon", 1e-5)))
        self._step_ws = None
        # decode-time logits from several heads (every mixing mode of GPT2LMMultiHeadModelMixing, `average_logits`): ONE head over the row [tap_0 | ... | ln_f(x)], its
        # matrix folded here in fp32 from the fp32 parameters and rounded to bf16 once (packing.head_fold); every load folds again
        w["taps"] = None
        if mixes_heads(c):
            taps = head_taps(c)
            heads = [F[f"head{k}"] for k in range(len(taps) - 1)] + [F["lm_head"] if "lm_head" in F else F["wte"]]
            fold, bias = head_fold(c, heads, F)
            w.update(taps=taps, head_fold=fold.to(BF16).contiguous(), head_bias=bias.contiguous() if bias is not None else None,
                     mix={k: F[k] for k in ("mix", "mix_w", "mix_b") if k in F})
            ptrs[4] = w["head_fold"]
            self._wtable_taps = (C.c_void_p * len(ptrs))(*[t.data_ptr() for t in ptrs])      # mi_decoder_step_taps: the same table with the folded head in slot 4
            self._taps = (C.c_int * len(taps))(*taps)

    def ensure_positions(self, n: int):
        """Positions [0, n) must have rows in the table the kernels read (they take row `past + u` unchecked).  Fixed sinusoidal positions exist for every position in
        the reference: the table grows, and the C step's pointer table follows it.  A learned wpe has n_positions rows (the reference fails with an index error past
        them): refused here, on the host, before any launch."""
        have = self.w["pos"].shape[0]
        if n <= have:
            return
        if not self.cfg.get("pos_emb_fixed", False):
            raise ValueError(f"decoding needs {n} positions but the learned position table (wpe) has n_positions = {have} rows")
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)        # (rare: once per longer cache) no queued step still reads the old table when it is released
        self.w["pos"] = _sinusoid_table(n, self.cfg["n_embd"], self.device)
        self._wtable[1] = self.w["pos"].data_ptr()
        if self.w.get("taps"):
            self._wtable_taps[1] = self.w["pos"].data_ptr()

    # ------------------------------------------------------------------ building blocks
    def cross_kv(self, enc_bf16: torch.Tensor):
        """Per-layer cross-attention keys/values of the encoder frames: list of (B*T', 2d) bf16 (computed once per utterance); fp32 in and out with precision="fp32"."""
        if self.precision == "fp32":
            return [ops_f32.gemm(enc_bf16, lw["wkv"], lw["bkv"]) for lw in self.w["layers"]]
        return [ops.gemm(enc_bf16, lw["wkv"], lw["bkv"]) for lw in self.w["layers"]]

    def _logits(self, hid_bf16, head_w, bias=None):
        V = head_w.shape[0]
        Vp = (V + 7) // 8 * 8
        buf = torch.empty((hid_bf16.shape[0], Vp), device=self.device, dtype=torch.float32)
        (ops_f32.gemm if self.precision == "fp32" else ops.gemm)(hid_bf16, head_w, bias, out=buf[:, :V])
        return buf[:, :V]

    def _head_input(self, taps: dict, hid):
        """the folded head's input rows [tap_0 | ... | ln_f(x)] (rows, H d) bf16: `taps` loc -> fp32 stream after loc blocks (loc < n_layer), `hid` bf16 ln_f output"""
        locs, d = self.w["taps"], self.cfg["n_embd"]
        cat = torch.empty((hid.shape[0], len(locs) * d), device=self.device, dtype=BF16)
        for h, loc in enumerate(locs):
            cat[:, h * d:(h + 1) * d] = ops.cast_bf16(taps[loc]) if loc in taps else hid
        return cat

    def _mixed_logits_fp32(self, per_head):
        """the reference's mix of the H per-head fp32 logit matrices (rows, V) in fp32 — the loss path; decoding runs the folded head instead"""
        c, mix = self.cfg, self.w["mix"]
        V = per_head[0].shape[1]
        buf = torch.empty((per_head[0].shape[0], (V + 7) // 8 * 8), device=self.device, dtype=torch.float32)
        out = buf[:, :V]
        if c["mixing_mode"] == "full":
            out.copy_(torch.cat(per_head, 1) @ mix["mix_w"].t() + mix["mix_b"])
        else:
            m = mix["mix"] if c["mixing_mode"] == "linear" else mix["mix"][:, None]
            out.copy_(sum(m[h] * per_head[h] for h in range(len(per_head))))
        return out

    def _block(self, l, x, B, U, kv, T_enc, enc_len, self_k=None, self_v=None, past=0, Lmax=0, beams=1):
        """One GPT-2 block on the fp32 stream x (B*U, d).  With a KV cache (self_k/self_v (B, Lmax, d)) U new tokens are
        appended at position `past` and attend to past+U keys.  `beams` (teacher-forced, no cache): the B sequences are B / beams utterances whose hypotheses share
        one cross table `kv` (B / beams * T_enc rows) each — cross-attention runs as B / beams batches of beams * U queries (it is not causal: the same kernel)."""
        c, lw = self.cfg, self.w["layers"][l]
        d, H, eps = c["n_embd"], c["n_head"], c.get("layer_norm_epsilon", 1e-5)
        M = x.shape[0]
        a = torch.empty((M, d), device=self.device, dtype=BF16)
        ops.layernorm_chain(x, lna=lw["ln1"], eps2=eps, outa=a)
        qkv = ops.gemm(a, lw["wqkv"], lw["bqkv"])
        if self_k is None:
            ctx = ops.attention_general(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], B, U, U, H, causal=True)
        else:
            self_k[:, past:past + U] = qkv[:, d:2 * d].reshape(B, U, d)
            self_v[:, past:past + U] = qkv[:, 2 * d:].reshape(B, U, d)
            ctx = ops.attention_general(qkv[:, :d], self_k.view(B * Lmax, d), self_v.view(B * Lmax, d), B, U, past + U, H,
                                        causal=True, kv_bstride=Lmax * d)
        ops.gemm(ctx, lw["wo"], lw["bo"], out=x, resid=x, alpha=1.0)
        ops.layernorm_chain(x, lna=lw["lnc"], eps2=eps, outa=a)
        qq = ops.gemm(a, lw["wq"], lw["bq"])
        ctx = ops.attention_general(qq, kv[:, :d], kv[:, d:], B // beams, beams * U, T_enc, H, lengths=enc_len)
        ops.gemm(ctx, lw["wco"], lw["bco"], out=x, resid=x, alpha=1.0)
        ops.layernorm_chain(x, lna=lw["ln2"], eps2=eps, outa=a)
        m = ops.gemm(a, lw["wfc"], lw["bfc"], act="gelu_new")
        ops.gemm(m, lw["wpr"], lw["bpr"], out=x, resid=x, alpha=1.0)
        return x

    def _block_f32(self, l, x, B, U, kv, T_enc, enc_len, self_k=None, self_v=None, past=0, Lmax=0, beams=1):
        """`_block` with every operand fp32 (ops_f32); `beams`: the B sequences are B / beams utterances whose hypotheses share one cross table `kv` each"""
        c, lw = self.cfg, self.w["layers"][l]
        d, H, eps = c["n_embd"], c["n_head"], c.get("layer_norm_epsilon", 1e-5)
        qkv = ops_f32.gemm(ops_f32.layernorm(x, *lw["ln1"], eps), lw["wqkv"], lw["bqkv"])
        if self_k is None:
            ctx = ops_f32.attention_general(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], B, U, U, H, causal=True)
        else:
            self_k[:, past:past + U] = qkv[:, d:2 * d].reshape(B, U, d)
            self_v[:, past:past + U] = qkv[:, 2 * d:].reshape(B, U, d)
            ctx = ops_f32.attention_general(qkv[:, :d], self_k.view(B * Lmax, d), self_v.view(B * Lmax, d), B, U, past + U, H, causal=True, kv_bstride=Lmax * d)
        ops_f32.gemm(ctx, lw["wo"], lw["bo"], out=x, resid=x)
        qq = ops_f32.gemm(ops_f32.layernorm(x, *lw["lnc"], eps), lw["wq"], lw["bq"])
        ctx = ops_f32.attention_general(qq, kv[:, :d], kv[:, d:], B, U, T_enc, H, lengths=enc_len, beams=beams)
        ops_f32.gemm(ctx, lw["wco"], lw["bco"], out=x, resid=x)
        m = ops_f32.gemm(ops_f32.layernorm(x, *lw["ln2"], eps), lw["wfc"], lw["bfc"], act="gelu_new")
        ops_f32.gemm(m, lw["wpr"], lw["bpr"], out=x, resid=x)
        return x

    # ------------------------------------------------------------------ teacher-forced forward
    def _forward_f32(self, ids, enc, T_enc, enc_len, labels):
        """`forward` with precision="fp32": LayerNorms, GEMMs and attention of ops_f32, the auxiliary heads of `head_locations` read the fp32 stream"""
        c, w = self.cfg, self.w
        B, U = ids.shape
        L, eps = c["n_layer"], c.get("layer_norm_epsilon", 1e-5)
        x = ops.embed_tokens(ids, w["wte"], w["pos"], scale=w["scale"])
        kvs = self.cross_kv(enc)
        locs = list(c.get("head_locations") or [])
        taps = {0: x.clone()} if 0 in locs else {}
        for l in range(L):
            x = self._block_f32(l, x, B, U, kvs[l], T_enc, enc_len)
            if (l + 1) in locs and l + 1 < L:
                taps[l + 1] = x.clone()
        hid = ops_f32.layernorm(x, *w["lnf"], eps)
        logits = self._logits(hid, w["lm_head"]).view(B, U, -1)
        loss = None
        if labels is not None:
            weights = list(c.get("head_weights") or [1.0])
            lsm = c.get("lsm_factor", 0.0)
            loss = weights[-1] * ops.ce_label_smoothing(logits, labels, shift=1, eps=lsm)
            for k, loc in enumerate(locs):
                lg = self._logits(taps[loc] if loc in taps else hid, w["heads"][k]).view(B, U, -1)
                loss = loss + weights[k] * ops.ce_label_smoothing(lg, labels, shift=1, eps=lsm)
        return dict(logits=logits, loss=loss)

    def forward(self, ids: torch.Tensor, enc_bf16: torch.Tensor, T_enc: int, enc_len, labels=None):
        """ids (B,U) int64; enc_bf16 (B*T', d) bf16 (already projected to the decoder width; fp32 with precision="fp32"); enc_len (B) int32 valid frames
        or None.  Returns dict(logits (B,U,V) fp32, loss | None) = GPT2LMMultiHeadModel.forward."""
        c, w = self.cfg, self.w
        B, U = ids.shape
        d, L, eps = c["n_embd"], c["n_layer"], c.get("layer_norm_epsilon", 1e-5)
        self.ensure_positions(U)
        if self.precision == "fp32":
            return self._forward_f32(ids, enc_bf16, T_enc, enc_len, labels)
        x = ops.embed_tokens(ids, w["wte"], w["pos"], scale=w["scale"])
        kvs = self.cross_kv(enc_bf16)
        locs = list(c.get("head_locations") or [])
        taps = {}
        if 0 in locs:
            taps[0] = x.clone()
        for l in range(L):
            x = self._block(l, x, B, U, kvs[l], T_enc, enc_len)
            if (l + 1) in locs and l + 1 < L:
                taps[l + 1] = x.clone()
        hid = torch.empty((B * U, d), device=self.device, dtype=BF16)
        ops.layernorm_chain(x, lna=w["lnf"], eps2=eps, outa=hid)
        if labels is None and w.get("taps"):                   # mixing modes / average_logits (multi_head_gpt2.py:129-136): the folded multi-tap head
            return dict(logits=self._logits(self._head_input(taps, hid), w["head_fold"], w["head_bias"]).view(B, U, -1), loss=None)
        if labels is not None and c.get("mixing_mode") is not None:
            # GPT2LMMultiHeadModelMixing with labels: the plain shifted cross-entropy of the mixed logits over every non-ignored position of the batch — the reference's
            # formula where the reference is defined (multi_head_gpt2_mixing.py:125-131 indexes `lm_logits[-1]`, the last utterance: B = 1)
            heads = list(w["heads"]) + [w["lm_head"]]
            per_head = [self._logits(ops.cast_bf16(taps[loc]) if loc in taps else hid, heads[h]) for h, loc in enumerate(w["taps"])]
            logits = self._mixed_logits_fp32(per_head).view(B, U, -1)
            return dict(logits=logits, loss=ops.ce_label_smoothing(logits, labels, shift=1, eps=0.0))
        logits = self._logits(hid, w["lm_head"]).view(B, U, -1)
        loss = None
        if labels is not None:
            weights = list(c.get("head_weights") or [1.0])
            loss = weights[-1] * ops.ce_label_smoothing(logits, labels, shift=1, eps=c.get("lsm_factor", 0.0))
            for k, loc in enumerate(locs):
                hb = ops.cast_bf16(taps[loc]) if loc in taps else hid
                lg = self._logits(hb, w["heads"][k]).view(B, U, -1)
                loss = loss + weights[k] * ops.ce_label_smoothing(lg, labels, shift=1, eps=c.get("lsm_factor", 0.0))
        return dict(logits=logits, loss=loss)

    # ------------------------------------------------------------------ teacher-forced scoring of given hypotheses (two-pass decoding)
    NLL_SCRATCH_BYTES = 64 << 20          # precision="fp32": the head's logits go through a scratch of at most this size, in row chunks

    def token_nll(self, ids: torch.Tensor, labels: torch.Tensor, enc, T_enc: int, enc_len, hyps_per_utt: int = 1):
        """Per-position negative log-likelihood of given hypotheses under the DECODING head: ids, labels (rows, U) int64 (`ops.rescore_pack`: labels[r, u] is the token
        that follows ids[r, :u + 1], negative = ignored), rows = B * hyps_per_utt with an utterance's hypotheses adjacent; enc (B*T', d) the utterance's encoder states
        (bf16; fp32 with precision="fp32"), enc_len (B) or None.  -> nll (rows * U) fp32 = lse - logit[label], exactly 0 on ignored positions.
        The blocks of `forward()`, laid out so that an utterance's cross K / V are computed and read once: self-attention over rows causal batches of U queries,
        cross-attention over B batches of hyps_per_utt * U queries.  Head: `lm_head`, or the folded multi-tap head of the mixing / average_logits decoders — what
        `step()` decodes with.  bf16: ops.gemm_ce, no (rows * U, V) logits are written; fp32: ops_f32.gemm into a bounded scratch, ops.row_lse, ops.rows_nll."""
        c, w = self.cfg, self.w
        rows, U = ids.shape
        N = int(hyps_per_utt)
        if labels.shape != ids.shape or N < 1 or rows % N or enc.shape[0] != rows // N * T_enc or (enc_len is not None and enc_len.numel() != rows // N):
            raise ValueError(f"token_nll: {tuple(ids.shape)} ids, {tuple(labels.shape)} labels, {N} hypotheses per utterance over {enc.shape[0]} encoder rows (T_enc = {T_enc})")
        d, L, eps = c["n_embd"], c["n_layer"], c.get("layer_norm_epsilon", 1e-5)
        self.ensure_positions(U)
        flat = labels.reshape(-1)
        x = ops.embed_tokens(ids, w["wte"], w["pos"], scale=w["scale"])
        kvs = self.cross_kv(enc)
        if self.precision == "fp32":
            for l in range(L):
                x = self._block_f32(l, x, rows, U, kvs[l], T_enc, enc_len, beams=N)
            hid = ops_f32.layernorm(x, *w["lnf"], eps)
            V = w["lm_head"].shape[0]
            Vp = (V + 7) // 8 * 8
            M = rows * U
            chunk = max(1, min(M, self.NLL_SCRATCH_BYTES // (4 * Vp)))
            buf = torch.empty((chunk, Vp), device=self.device, dtype=torch.float32)
            out = []
            for lo in range(0, M, chunk):
                n = min(chunk, M - lo)
                lg = ops_f32.gemm(hid[lo:lo + n], w["lm_head"], out=buf[:n, :V])
                out.append(ops.rows_nll(lg, ops.row_lse(lg), flat[lo:lo + n]))
            return out[0] if len(out) == 1 else torch.cat(out)
        locs = w.get("taps") or []
        taps = {0: x.clone()} if 0 in locs else {}
        for l in range(L):
            x = self._block(l, x, rows, U, kvs[l], T_enc, enc_len, beams=N)
            if (l + 1) in locs and l + 1 < L:
                taps[l + 1] = x.clone()
        hid = torch.empty((rows * U, d), device=self.device, dtype=BF16)
        ops.layernorm_chain(x, lna=w["lnf"], eps2=eps, outa=hid)
        if locs:
            return ops.gemm_ce(self._head_input(taps, hid), w["head_fold"], flat, bias=w["head_bias"])[2]
        return ops.gemm_ce(hid, w["lm_head"], flat)[2]

    # ------------------------------------------------------------------ incremental decoding
    def init_cache(self, B: int, Lmax: int):
        """KV cache: two sets of (B, Lmax, d) tensors per layer (beam re-ordering copies set A -> set B in one kernel and swaps); fp32 with precision="fp32"."""
        d, L = self.cfg["n_embd"], self.cfg["n_layer"]
        if self.cfg.get("pos_emb_fixed", False):
            self.ensure_positions(Lmax)
        # one allocation and one fill for all 4 L tensors.  Zero, not empty: the MFMA attention kernel stages whole 32-key tiles, and a V row past the last key meets a
        # probability of exactly 0 — which only gives 0 if the row holds finite numbers
        buf = torch.zeros((4, L, B, Lmax, d), device=self.device, dtype=torch.float32 if self.precision == "fp32" else BF16)
        cache = dict(k=list(buf[0].unbind(0)), v=list(buf[1].unbind(0)), k2=list(buf[2].unbind(0)), v2=list(buf[3].unbind(0)), past=0, Lmax=Lmax)
        self._cache_tables(cache)
        return cache

    @staticmethod
    def _cache_tables(cache):
        tab = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        cache["tk"], cache["tv"], cache["tk2"], cache["tv2"] = tab(cache["k"]), tab(cache["v"]), tab(cache["k2"]), tab(cache["v2"])

    def reorder_cache(self, cache, beam_idx: torch.Tensor):
        """transformers' `_reorder_cache`: every layer's K and V rows follow their beam (one kernel for all 2L tensors)."""
        L = len(cache["k"])
        B, Lmax, d = cache["k"][0].shape
        d *= cache["k"][0].element_size() // 2               # the kernel copies rows of `d` 2-byte elements: an fp32 cache is the same copy at twice the width
        beam_idx = beam_idx.to(device=self.device, dtype=torch.long).contiguous()
        _lib.check(_lib.lib().mi_kv_cache_reorder(cache["tk"], cache["tv"], cache["tk2"], cache["tv2"], beam_idx.data_ptr(), L, B, cache["past"], Lmax, d,
                                                  torch.cuda.current_stream().cuda_stream), "mi_kv_cache_reorder")
        cache["k"], cache["k2"] = cache["k2"], cache["k"]
        cache["v"], cache["v2"] = cache["v2"], cache["v"]
        cache["tk"], cache["tk2"] = cache["tk2"], cache["tk"]
        cache["tv"], cache["tv2"] = cache["tv2"], cache["tv"]

    def step(self, ids_new: torch.Tensor, cache, kvs, T_enc: int, enc_len, beams: int = 1):
        """ids_new (B, U_new) -> logits (B, V) of the LAST new position; appends to the KV cache.  One C call (mi_gpt2_step).
        `beams` > 1: the B rows are B / beams utterances x `beams` hypotheses that share their utterance's encoder frames — `kvs` are (B / beams * T_enc, 2d) and
        `enc_len` (B / beams) (mi_decoder_step_beams; one new token per row).
        precision="fp32": mi_decoder_step_f32 on fp32 caches and tables, which always reads the cross tables as shared by `beams` hypotheses (1: one table per row)."""
        c, w = self.cfg, self.w
        ids_new = ids_new.contiguous()
        B, U = ids_new.shape
        past, Lmax = cache["past"], cache["Lmax"]
        self.ensure_positions(past + U)
        L_ = _lib.lib()
        if self.precision == "fp32":
            if beams < 1 or B % beams or kvs[0].shape[0] != B // beams * T_enc or (enc_len is not None and enc_len.numel() != B // beams):
                raise ValueError(f"step(beams={beams}): {B} rows of {U} new tokens over cross tables of {kvs[0].shape[0]} rows (T_enc = {T_enc})")
            if kvs[0].dtype != torch.float32 or cache["k"][0].dtype != torch.float32:
                raise TypeError("precision='fp32': the cross K/V tables and the KV cache must be fp32 (cross_kv / init_cache of this engine)")
            nbytes = L_.mi_decoder_step_f32_workspace_bytes(C.byref(self._gcfg), B, U)
            if self._step_ws is None or self._step_ws.numel() < nbytes:
                self._step_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            if cache.get("kv_id") != id(kvs):
                cache["tkv"] = (C.c_void_p * len(kvs))(*[t.data_ptr() for t in kvs])
                cache["kv_id"] = id(kvs)
            V = self._gcfg.V
            Vp = (V + 7) // 8 * 8
            buf = torch.empty((B, Vp), device=self.device, dtype=torch.float32)
            _lib.check(L_.mi_decoder_step_f32(C.byref(self._gcfg), self._wtable, ids_new.data_ptr(), B, beams, U, past, Lmax, cache["tk"], cache["tv"], cache["tkv"], T_enc,
                                              enc_len.data_ptr() if enc_len is not None else None, float(w["scale"]), None, self._step_ws.data_ptr(),
                                              self._step_ws.numel(), buf.data_ptr(), Vp, torch.cuda.current_stream().cuda_stream), "mi_decoder_step_f32")
            cache["past"] = past + U
            return buf[:, :V]
        taps = w.get("taps")
        nbytes = L_.mi_decoder_step_taps_workspace_bytes(C.byref(self._gcfg), B, U, len(taps)) if taps else L_.mi_gpt2_step_workspace_bytes(C.byref(self._gcfg), B, U)
        if self._step_ws is None or self._step_ws.numel() < nbytes:
            self._step_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if cache.get("kv_id") != id(kvs):                              # pointer table of the per-layer encoder K/V
            cache["tkv"] = (C.c_void_p * len(kvs))(*[t.data_ptr() for t in kvs])
            cache["kv_id"] = id(kvs)
        V = self._gcfg.V
        Vp = (V + 7) // 8 * 8
        buf = torch.empty((B, Vp), device=self.device, dtype=torch.float32)
        if beams != 1:
            if beams < 1 or B % beams or U != 1 or kvs[0].shape[0] != B // beams * T_enc or (enc_len is not None and enc_len.numel() != B // beams):
                raise ValueError(f"step(beams={beams}): {B} rows of {U} new tokens over cross tables of {kvs[0].shape[0]} rows (T_enc = {T_enc})")
        if taps:                                                       # the multi-tap head (mixing modes, average_logits): the same step, taps written as their layers complete
            hb = w["head_bias"]
            _lib.check(L_.mi_decoder_step_taps(C.byref(self._gcfg), self._wtable_taps, ids_new.data_ptr(), B, beams, U, past, Lmax, cache["tk"], cache["tv"], cache["tkv"], T_enc,
                                               enc_len.data_ptr() if enc_len is not None else None, float(w["scale"]), hb.data_ptr() if hb is not None else None,
                                               self._taps, len(taps), self._step_ws.data_ptr(), self._step_ws.numel(), buf.data_ptr(), Vp,
                                               torch.cuda.current_stream().cuda_stream), "mi_decoder_step_taps")
            cache["past"] = past + U
            return buf[:, :V]
        if beams != 1:
            _lib.check(L_.mi_decoder_step_beams(C.byref(self._gcfg), self._wtable, ids_new.data_ptr(), B, beams, U, past, Lmax, cache["tk"], cache["tv"], cache["tkv"], T_enc,
                                                enc_len.data_ptr() if enc_len is not None else None, float(w["scale"]), None, self._step_ws.data_ptr(),
                                                self._step_ws.numel(), buf.data_ptr(), Vp, torch.cuda.current_stream().cuda_stream), "mi_decoder_step_beams")
            cache["past"] = past + U
            return buf[:, :V]
        _lib.check(L_.mi_gpt2_step(C.byref(self._gcfg), self._wtable, ids_new.data_ptr(), B, U, past, Lmax, cache["tk"], cache["tv"], cache["tkv"], T_enc,
                                   enc_len.data_ptr() if enc_len is not None else None, float(w["scale"]), self._step_ws.data_ptr(), self._step_ws.numel(),
                                   buf.data_ptr(), Vp, torch.cuda.current_stream().cuda_stream), "mi_gpt2_step")
        cache["past"] = past + U
        return buf[:, :V]

    def step_py(self, ids_new: torch.Tensor, cache, kvs, T_enc: int, enc_len, beams: int = 1):
        """same step driven op by op from Python (kept as the cross-check of the C driver); precision="fp32": the same operations through ops_f32 (`beams` as in `step`)"""
        c, w = self.cfg, self.w
        B, U = ids_new.shape
        d, L, eps = c["n_embd"], c["n_layer"], c.get("layer_norm_epsilon", 1e-5)
        past, Lmax = cache["past"], cache["Lmax"]
        self.ensure_positions(past + U)
        x = ops.embed_tokens(ids_new, w["wte"], w["pos"], scale=w["scale"], pos_offset=past)
        if self.precision == "fp32":
            for l in range(L):
                x = self._block_f32(l, x, B, U, kvs[l], T_enc, enc_len, cache["k"][l], cache["v"][l], past, Lmax, beams)
            cache["past"] = past + U
            return self._logits(ops_f32.layernorm(x.view(B, U, d)[:, -1].contiguous(), *w["lnf"], eps), w["lm_head"])
        if beams != 1:
            raise ValueError("step_py(beams > 1) is the fp32 cross-check; the bf16 one reads one cross table per row")
        locs = w.get("taps") or []
        last_of = lambda t: t.view(B, U, d)[:, -1].clone()             # a copy: the blocks update the stream in place
        taps = {0: last_of(x)} if 0 in locs else {}
        for l in range(L):
            x = self._block(l, x, B, U, kvs[l], T_enc, enc_len, cache["k"][l], cache["v"][l], past, Lmax)
            if (l + 1) in locs and l + 1 < L:
                taps[l + 1] = last_of(x)
        cache["past"] = past + U
        last = last_of(x)
        hid = torch.empty((B, d), device=self.device, dtype=BF16)
        ops.layernorm_chain(last, lna=w["lnf"], eps2=eps, outa=hid)
        if locs:
            return self._logits(self._head_input(taps, hid), w["head_fold"], w["head_bias"])
        return self._logits(hid, w["lm_head"])


def lm_cfg_dict(c) -> dict:
    """the fields of a transformers `GPT2Config` that `GPT2LMEngine` reads"""
    return dict(vocab_size=c.vocab_size, n_embd=c.n_embd, n_layer=c.n_layer, n_head=c.n_head, n_positions=c.n_positions, n_inner=getattr(c, "n_inner", None),
                layer_norm_epsilon=c.layer_norm_epsilon, activation_function=c.activation_function,
                scale_attn_weights=bool(getattr(c, "scale_attn_weights", True)),
                scale_attn_by_inverse_layer_idx=bool(getattr(c, "scale_attn_by_inverse_layer_idx", False)),
                reorder_and_upcast_attn=bool(getattr(c, "reorder_and_upcast_attn", False)), add_cross_attention=bool(getattr(c, "add_cross_attention", False)))


class GPT2LMEngine(GPT2DecoderEngine):
    """transformers' `GPT2LMHeadModel` as a KV-cached token step on the HIP path: the external language model of shallow fusion (reference
    src/decoding/shallow_fussion.py:41-53, which re-runs the LM over the whole prefix for every token).  `GPT2DecoderEngine` without the cross parts: the same pointer
    table with the six cross entries of a layer null, `mi_gpt2_step` called without encoder K/V; cache, beam re-ordering and the position check are inherited."""

    def __init__(self, cfg: dict, device="cuda:0", precision="bf16"):
        if _check_precision("GPT2LMEngine", precision) == "fp32":
            raise NotImplementedError("precision='fp32' does not cover GPT2LMEngine (shallow fusion, generate(lm=...)): use the default precision='bf16'")
        super().__init__(cfg, device)                      # head size 64 / 128, gelu_new
        d = cfg["n_embd"]
        if cfg.get("n_inner") not in (None, 4 * d):
            raise NotImplementedError(f"GPT-2 LM with n_inner = {cfg['n_inner']}: the HIP block has a 4 * n_embd MLP")
        if not cfg.get("scale_attn_weights", True):
            raise NotImplementedError("GPT-2 LM with scale_attn_weights = False")
        for k in ("scale_attn_by_inverse_layer_idx", "reorder_and_upcast_attn", "add_cross_attention"):
            if cfg.get(k, False):
                raise NotImplementedError(f"GPT-2 LM with {k} = True is not implemented on the HIP path")

    def load_state_dict(self, sd: dict, prefix: str = ""):
        """every packed parameter of packing.lm_specs; a state dict without `lm_head.weight` has the token embedding as its head"""
        c, dev = self.cfg, self.device
        d, L = c["n_embd"], c["n_layer"]
        c = dict(c, tie_word_embeddings=(prefix + "lm_head.weight") not in sd)
        m = _lm_map(c, prefix)
        P = {s.name: (t.to(BF16) if s.mat and s.name != "wte" else t).contiguous() for s, t in packed(lm_specs(c), m, mapped_fp32(m, sd, dev))}
        w = dict(wte=P["wte"], scale=1.0, pos=P["wpe"], lnf=(P["lnf_g"], P["lnf_b"]), lm_head=P["lm_head"] if "lm_head" in P else P["wte"].to(BF16))
        w["layers"] = [dict({n: P[f"h{l}.{n}"] for n in ("wqkv", "bqkv", "wo", "bo", "wfc", "bfc", "wpr", "bpr")},
                            **{n: (P[f"h{l}.{n}_g"], P[f"h{l}.{n}_b"]) for n in ("ln1", "ln2")}) for l in range(L)]
        self.w = w
        ptr = lambda t: t.data_ptr()
        ptrs = [ptr(w["wte"]), ptr(w["pos"]), ptr(w["lnf"][0]), ptr(w["lnf"][1]), ptr(w["lm_head"])]
        for lw in w["layers"]:                             # mi_gpt2_step's 18 slots per layer, the six cross entries null
            ptrs += [ptr(lw["ln1"][0]), ptr(lw["ln1"][1]), ptr(lw["wqkv"]), ptr(lw["bqkv"]), ptr(lw["wo"]), ptr(lw["bo"]), None, None, None, None, None, None,
                     ptr(lw["ln2"][0]), ptr(lw["ln2"][1]), ptr(lw["wfc"]), ptr(lw["bfc"]), ptr(lw["wpr"]), ptr(lw["bpr"])]
        self._wtable = (C.c_void_p * len(ptrs))(*ptrs)
        self._gcfg = _lib.Gpt2Config(d=d, H=c["n_head"], L=L, V=w["lm_head"].shape[0], eps=float(c.get("layer_norm_epsilon", 1e-5)))
        self._step_ws = None

    def step(self, ids_new: torch.Tensor, cache):
        """ids_new (rows, U_new) -> fp32 logits (rows, V) of the LAST new position; appends to the KV cache.  One C call (mi_gpt2_step without cross-attention)."""
        ids_new = ids_new.contiguous()
        B, U = ids_new.shape
        past, Lmax = cache["past"], cache["Lmax"]
        self.ensure_positions(past + U)
        L_ = _lib.lib()
        nbytes = L_.mi_gpt2_step_workspace_bytes(C.byref(self._gcfg), B, U)
        if self._step_ws is None or self._step_ws.numel() < nbytes:
            self._step_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        V = self._gcfg.V
        Vp = (V + 7) // 8 * 8
        buf = torch.empty((B, Vp), device=self.device, dtype=torch.float32)
        _lib.check(L_.mi_gpt2_step(C.byref(self._gcfg), self._wtable, ids_new.data_ptr(), B, U, past, Lmax, cache["tk"], cache["tv"], None, 0, None, 1.0,
                                   self._step_ws.data_ptr(), self._step_ws.numel(), buf.data_ptr(), Vp, torch.cuda.current_stream().cuda_stream), "mi_gpt2_step")
        cache["past"] = past + U
        return buf[:, :V]


def lm_engine_for(lm, device) -> GPT2LMEngine:
    """the HIP engine of a transformers `GPT2LMHeadModel` module on `device` (its parameters are copied there by the load, as the reference's `.to(device)` does): one per
    module, cached on it, rebuilt when a parameter was replaced, moved or written in place (keyed like whisper._decoder_engine_for)"""
    params = list(lm.parameters())
    key = (str(torch.device(device)), tuple((p.data_ptr(), p._version) for p in params))
    cached = lm.__dict__.get("_hfasr_lm_engine")
    if cached is not None and cached[0] == key:
        return cached[1]
    eng = GPT2LMEngine(lm_cfg_dict(lm.config), device)
    eng.load_state_dict(lm.state_dict())
    lm.__dict__["_hfasr_lm_engine"] = (key, eng)
    return eng


def shift_tokens_right(labels: torch.Tensor, pad_id: int, start_id: int) -> torch.Tensor:
    out = labels.new_zeros(labels.shape)
    out[:, 1:] = labels[:, :-1]
    out[:, 0] = start_id
    return out.masked_fill(out == -100, pad_id)


class JointAEDEngine:
    """JointCTCAttentionEncoderDecoder.forward (eval) on the HIP path."""

    def __init__(self, enc_cfg: dict, dec_cfg: dict, joint_cfg: dict, device="cuda:0", precision="bf16"):
        """precision="fp32": both engines in that mode (what either refuses keeps raising from its constructor), fp32 encoder states, tables, caches and token step"""
        self.precision = _check_precision("JointAEDEngine", precision)
        self.enc = EBranchformerEngine(enc_cfg, device, precision=precision)
        self.dec = GPT2DecoderEngine(dec_cfg, device, precision=precision)
        self.jcfg = dict(joint_cfg)
        self.device = torch.device(device)
        self.proj = None

    def load_state_dict(self, sd: dict):
        self.enc.load_state_dict({k[len("encoder."):]: v for k, v in sd.items() if k.startswith("encoder.")})
        self.dec.load_state_dict(sd, "decoder.")
        if "enc_to_dec_proj.weight" in sd:
            self.proj = (sd["enc_to_dec_proj.weight"].detach().to(self.device, torch.float32).to(torch.float32 if self.precision == "fp32" else BF16).contiguous(),
                         sd["enc_to_dec_proj.bias"].detach().to(self.device, torch.float32).contiguous())

    def encode(self, feats, feat_len):
        """-> (encoder out dict, encoder states for the decoder (B*T', d_dec) bf16 — fp32 with precision="fp32" —, T', cross-attention key lengths)."""
        out = self.enc.forward(feats, feat_len, want_hidden=True)
        B, T2, d = out["last_hidden"].shape
        hid = out["last_hidden"].reshape(B * T2, d)
        if self.precision == "fp32":
            enc_bf = ops_f32.gemm(hid, self.proj[0], self.proj[1]) if self.proj is not None else hid
        elif self.proj is not None:
            enc_bf = ops.gemm(ops.cast_bf16(hid), self.proj[0], self.proj[1])       # ctc_encoder_plus...:289-293
        else:
            enc_bf = ops.cast_bf16(hid)
        # cross mask uses the OUTER (un-padded) length formula, quirk 8' (:296-301); no attention_mask -> all frames
        key_len = torch.clamp(out["outer_len"], max=T2) if feat_len is not None else None
        return out, enc_bf, T2, key_len

    def transcribe(self, *args, **kwargs):
        """the joint model's CTC head decoded on its own: `EBranchformerEngine.transcribe` of the encoder engine (greedy, or prefix beam search with `beams=`)"""
        return self.enc.transcribe(*args, **kwargs)

    def align(self, *args, **kwargs):
        """CTC forced alignment with the joint model's CTC head: `EBranchformerEngine.align` of the encoder engine"""
        return self.enc.align(*args, **kwargs)

    def forward(self, feats, feat_len, labels):
        c = self.jcfg
        enc_out, enc_bf, T2, key_len = self.encode(feats, feat_len)
        enc_loss, _, _ = ops.ctc_loss(enc_out["logits"], labels, enc_out["outer_len"],
                                      reduction=self.enc.cfg.get("ctc_loss_reduction", "mean"),
                                      zero_infinity=self.enc.cfg.get("ctc_zero_infinity", False), lse=enc_out.get("lse"))
        dec_ids = shift_tokens_right(labels, c["pad_token_id"], c["decoder_start_token_id"])
        d = self.dec.forward(dec_ids, enc_bf, T2, key_len, labels)
        w = c["ctc_weight"]
        return dict(loss=w * enc_loss + (1 - w) * d["loss"], enc_loss=enc_loss, dec_loss=d["loss"], logits=d["logits"],
                    encoder_logits=enc_out["logits"], encoder_hidden=enc_bf)


# ---------------------------------------------------------------------------------------------------------------------
# Joint CTC/attention decoding (config 5 of BASELINE.json): greedy (W = 1) and beam search with the device-side CTC
# prefix scorer.  Mirrors what the reference obtains from GenerationMixin.generate + its logits processors
# (ctc_encoder_plus_autoregressive_decoder.py:360-482, hf_shared_models/ED_small.py:20-22: ctc_weight 0.3, num_beams 5):
# scores = log_softmax(decoder logits) -> [CTC processor: pad masked, (1-w)*att + w*ctc] -> + running beam score -> top 2W over W*V ->
# candidates that stop (EOS, or max_length reached) among the first W ranks join the kept hypotheses with sum_logprob / generated_tokens**length_penalty,
# the best W are kept; the first W that did not stop run on; the early-stop rule compares the best running beam with the worst kept hypothesis
# (transformers/generation/utils.py `_beam_search` of the installed 5.x — the loop the reference's generate() runs here; pinned by tests/golden/gen_*.npz,
# restated in oracle/generate_ref.py).
_ES_MODE = {False: 0, True: 1, "never": 2}


def _step_denoms(cur_len, max_length, length_penalty, early_stopping, prompt_len=1):
    """(closing denominator, early-stop denominator) of the step that extends prefixes of `cur_len` tokens (`prompt_len` of them the prompt: the start token), as fp32
    values: generated tokens of a hypothesis closed now = cur_len + 1 - prompt_len; hypothetical length of the early-stop rule = the same, or max_length - prompt_len for
    "never" with a positive penalty."""
    import numpy as np
    gen = cur_len + 1 - prompt_len
    hyp = (max_length - prompt_len) if (early_stopping == "never" and length_penalty > 0.0) else gen
    return float(np.float32(gen ** length_penalty)), float(np.float32(hyp ** length_penalty))


def _stop_rule(num_beams, cur_len, max_length, length_penalty, early_stopping):
    """(closing denominator, early-stop denominator, early-stop mode) of a step.  One beam is transformers' greedy loop, which the reference runs for num_beams = 1: it
    stops at the first EOS whatever `early_stopping` and `length_penalty` say.  The beam rules give that with mode False and the early-stop denominator equal to the
    closing one (the running beam, ranked behind the EOS candidate, cannot beat it); "never" with a positive penalty would keep the runner-up alive."""
    denom, heur = _step_denoms(cur_len, max_length, length_penalty, early_stopping)
    if num_beams == 1:
        return denom, denom, 0
    return denom, heur, _ES_MODE[early_stopping]


def check_lm_args(lm_vocab, lm_positions, dec_vocab, max_length):
    """what shallow fusion needs of the LM, checked on the host before anything is enqueued: the decoder's vocabulary (the two score rows are added token by token) and a
    learned position table that reaches the last step (position max_length - 2)"""
    if lm_vocab != dec_vocab:
        raise ValueError(f"the language model has {lm_vocab} tokens, the decoder {dec_vocab}: shallow fusion needs one vocabulary")
    if lm_positions < max_length - 1:
        raise ValueError(f"decoding to max_length = {max_length} needs {max_length - 1} positions but the language model's position table (wpe) has n_positions = {lm_positions} rows")


def _check_generate_args(joint, num_beams, max_length, early_stopping, lm=None, lm_weight=0.0):
    """-> the LM engine to use (None when the term is off)"""
    if early_stopping not in _ES_MODE:
        raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")
    if lm is not None and lm_weight > 0 and getattr(joint, "precision", "bf16") == "fp32":
        raise NotImplementedError("precision='fp32' does not cover shallow fusion (generate(lm=...): GPT2LMEngine is bf16-only): decode without lm, or with precision='bf16'")
    if num_beams < 1 or max_length < 2:
        raise ValueError(f"num_beams >= 1 and max_length >= 2 required, got {num_beams}, {max_length}")
    joint.dec.ensure_positions(max_length - 1)           # the last step feeds position max_length - 2: a learned table too short is refused before decoding starts
    if lm is None or not lm_weight > 0:                   # the reference appends its LM processor only for lm_weight > 0 (ctc_encoder_plus_autoregressive_decoder.py:398)
        return None
    if not isinstance(lm, GPT2LMEngine):
        raise TypeError(f"lm must be a GPT2LMEngine (decoder.lm_engine_for(module, device)), got {type(lm)}")
    check_lm_args(lm.w["lm_head"].shape[0], lm.w["pos"].shape[0], joint.dec.w["lm_head"].shape[0], max_length)
    return lm


BEAM_STEP_MAXW, BEAM_STEP_LDS, BEAM_WIDE_MAXW, BEAM_MAX_CANDIDATES = 16, 96 * 1024, 64, 1 << 24        # csrc/beam_step.hip (BS_MAXW, its id buffers in LDS), csrc/beam_step_wide.hip
SKINNY_MAX_ROWS = 8                        # csrc/decoder_step.hip SK_MAXM: up to here the token step is the fused / GEMV form, which indexes the cross tables by row


def beam_loop_route(W: int, V: int, max_length: int, eos_space_trick: bool = False) -> str:
    """Which loop serves a decoding request: "device" (`generate` with mi_beam_step / mi_beam_step_lm: W <= 16 and the utterance's two id buffers within 96 KiB of LDS),
    "device_wide" (`generate` with mi_beam_step_wide: W <= 64, any max_length) or "host" (`generate_stepwise`: the eos / space trick, which lives in the processor the host
    loop calls; more than 64 beams; W * V >= 2^24 candidates, whose indices the kernels keep in 24 bits)."""
    if eos_space_trick or W > BEAM_WIDE_MAXW or W * V >= BEAM_MAX_CANDIDATES:
        return "host"
    if W <= BEAM_STEP_MAXW and W * (max_length + max_length + 1) * 8 <= BEAM_STEP_LDS:
        return "device"
    return "device_wide"


def cross_kv_layout(B: int, W: int, T_enc: int, d: int, n_layer: int, share=None) -> dict:
    """How the W hypotheses of each of B utterances see their encoder K/V in the token step: `beams` = 1 — every row has its own copy of its utterance's tables (B * W
    * T_enc rows per layer) — or `beams` = W — one table per utterance (B * T_enc rows), shared (`GPT2DecoderEngine.step(beams=W)`).  Shared when the step has more than 8
    rows, the rule by which it leaves its fused / GEMV forms (which index the tables by row; config 5 keeps its kernels and its bits); `share` = True / False overrides.
    `bytes`: bf16 K and V of all layers."""
    if share is None:
        share = B * W > SKINNY_MAX_ROWS
    share = bool(share) and W > 1
    kv_rows = (B if share else B * W) * T_enc
    return dict(beams=W if share else 1, kv_rows=kv_rows, bytes=kv_rows * 2 * d * 2 * n_layer)


def _beam_cross_kv(joint, enc_bf, key_len, B, W, T2, share=None):
    """-> (per-layer cross K/V, key lengths, `beams` of the token step) for B utterances x W hypotheses: the arrangement `generate` and `generate_stepwise` both decode on
    (the same step on the same tables: that is what keeps the two loops bit-identical to each other).  precision="fp32": always the shared layout, the only one its step has"""
    d = enc_bf.shape[1]
    if getattr(joint, "precision", "bf16") == "fp32":
        share = True
    lay = cross_kv_layout(B, W, T2, joint.dec.cfg["n_embd"], joint.dec.cfg["n_layer"], share)
    if lay["beams"] > 1:
        return joint.dec.cross_kv(enc_bf), key_len, lay["beams"]
    enc_rep = enc_bf.view(B, T2, d).repeat_interleave(W, 0).reshape(B * W * T2, d)          # every beam attends to its utterance's encoder frames
    key_rep = key_len.repeat_interleave(W) if key_len is not None else None
    return joint.dec.cross_kv(enc_rep), key_rep, 1


def generate(joint: "JointAEDEngine", feats, feat_len, *, num_beams=1, max_length=64, ctc_weight=0.3, length_penalty=1.0, early_stopping=False,
             eos_token_id=1, pad_token_id=None, start_token_id=None, space_token_id=-1, apply_eos_space_trick=False, eos_space_trick_weight=1.0,
             run_ahead=2, stats=None, trace=None, lm=None, lm_weight=0.0, lm_side_stream=False, share_cross_kv=None):
    """Device-resident decoding loop: per token the decoder step (one C call), the row log-sum-exp and ONE launch that mixes the CTC prefix scores in, takes the top 2W
    candidates, applies the beam loop's rules and moves ids / beam scores / kept hypotheses on the device (csrc/beam_step.hip).  The CTC prefix scorer of step t
    depends on the prefixes only, not on the decoder's logits: it runs on a second stream beside the decoder step.  Nothing is copied to the host until decoding ends, except
    the per-utterance `done` flags (the kernel writes them into pinned, device-mapped memory): the host stays at most `run_ahead` steps in front of the GPU and stops enqueuing once every utterance is done.
    Returns per utterance dict(tokens, score, hypotheses = the kept (score, tokens), best first, at most W).  Same hypotheses, scores and order as `generate_stepwise`
    (same arithmetic, operation for operation).  `stats` (a dict) receives the host time spent enqueuing the token loop and the number of steps enqueued; `trace` (a list)
    receives per step the (B, 2W) candidate values and indices the kernel walked and the (B) done flags before the step (device tensors).
    Shallow fusion (`lm`: a GPT2LMEngine, `lm_weight` > 0; reference src/decoding/shallow_fussion.py): the LM is one more KV-cached token step on the same new tokens, its
    cache follows the same `beam_idx`, and the kernel adds lm_weight * (lm logits - their row log-sum-exp) behind the CTC mix (`mi_beam_step_lm`); the candidate values of
    `trace` include it.  The LM step reads only what the decoder step reads: `lm_side_stream` runs it on a stream of its own beside the decoder step (off by default: not
    measured).
    `beam_loop_route` picks the step kernel (mi_beam_step / mi_beam_step_lm within their limits, mi_beam_step_wide up to 64 beams and any max_length) or hands the request
    to `generate_stepwise`; `cross_kv_layout` decides whether the hypotheses share their utterance's cross K/V (`share_cross_kv` = True / False overrides its rule)."""
    from .decoding import CTCRescorerLogitsProcessor
    lm = _check_generate_args(joint, num_beams, max_length, early_stopping, lm, lm_weight)
    dev = joint.device
    c = joint.jcfg
    pad = c["pad_token_id"] if pad_token_id is None else pad_token_id
    start = c["decoder_start_token_id"] if start_token_id is None else start_token_id
    W = num_beams
    L_ = _lib.lib()
    main = torch.cuda.current_stream()
    V = joint.dec.w["lm_head"].shape[0]
    Lmax = max_length + 1
    route = beam_loop_route(W, V, max_length, bool(apply_eos_space_trick))
    if route == "host":
        # the eos / space trick (ctc_scorer.py:333-349) lives in the processor the host loop calls; beyond the step kernels' limits (beams, candidates) the bookkeeping
        # runs on the host as well (still the HIP kernels for everything else) — decided here, not by an error in the middle of a decode
        return generate_stepwise(joint, feats, feat_len, num_beams=num_beams, max_length=max_length, ctc_weight=ctc_weight, length_penalty=length_penalty,
                                 early_stopping=early_stopping, eos_token_id=eos_token_id, pad_token_id=pad_token_id, start_token_id=start_token_id,
                                 space_token_id=space_token_id, apply_eos_space_trick=apply_eos_space_trick, eos_space_trick_weight=eos_space_trick_weight,
                                 lm=lm, lm_weight=lm_weight, share_cross_kv=share_cross_kv)
    enc_out, enc_bf, T2, key_len = joint.encode(feats, feat_len)
    B = feats.shape[0]
    kvs, key_rep, kv_beams = _beam_cross_kv(joint, enc_bf, key_len, B, W, T2, share_cross_kv)
    cache = joint.dec.init_cache(B * W, Lmax)
    lm_cache = lm.init_cache(B * W, Lmax) if lm is not None else None
    lm_st = torch.cuda.Stream(device=dev) if (lm is not None and lm_side_stream) else None       # the LM step beside the decoder step (event discipline of the CTC scorer's stream)
    w_lm = float(lm_weight)
    lm_idx = None                              # beam_idx of the previous step: the LM's cache follows it before the LM's next step, on the stream the LM runs on
    proc, side = None, None
    if ctc_weight > 0:
        lens = enc_out["outer_len"].clamp(max=T2)
        proc = CTCRescorerLogitsProcessor(enc_out["logits"], lens, pad, eos_token_id, 0, ctc_weight, W, space_token_id, False, 1.0)
        if proc.O != V:
            raise ValueError(f"CTC head has {proc.O} classes, the decoder {V}: joint decoding needs one vocabulary")
        # beside the decoder step the scorer competes with it for the memory system (its step is a chain of latency-bound launches: 358 -> 409 us per token at W = 1 with the
        # scorer running): the form that re-runs the selected chains moves a tenth of the bytes of the form that keeps every chain (425 us), so it is the one used here —
        # for a processor called in sequence (HF generate, generate_stepwise) the single-scan form is the faster one (tools/decode_step_timing.py)
        proc.FULL_STATE_BYTES = 0
        side = torch.cuda.Stream(device=dev)                 # a higher stream priority for the scorer was measured: no better (21.4 -> 25 ms and erratic)
    n_bh = B * W
    ids = torch.full((n_bh, Lmax), pad, dtype=torch.long, device=dev)
    ids[:, 0] = start
    beam_scores = torch.zeros((B, W), device=dev)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1).contiguous()
    done = torch.zeros((B,), dtype=torch.int32, device=dev)
    nfin = torch.zeros((B,), dtype=torch.int32, device=dev)
    fin_score = torch.zeros((B, W), dtype=torch.float32, device=dev)
    fin_len = torch.zeros((B, W), dtype=torch.int32, device=dev)
    fin_tok = torch.full((B, W, Lmax), pad, dtype=torch.long, device=dev)
    done_host = torch.zeros((max_length, B), dtype=torch.int32).pin_memory()
    new_tok = ids[:, :1].contiguous()
    flags = []                                 # (event, step) of the done-flag copies
    ev_ids = torch.cuda.Event()
    ev_ids.record(main)
    cur_len, steps = 1, 0
    w_att, w_ctc = float(1 - ctc_weight), float(ctc_weight)
    t_loop = time.perf_counter()
    while cur_len < max_length:
        if len(flags) >= run_ahead:            # bounded run-ahead: wait for the flags of step (now - run_ahead) and stop if everything is done
            ev, t = flags[len(flags) - run_ahead]
            ev.synchronize()
            if bool(done_host[t].all()):
                break
        ctc = None
        if proc is not None:                   # prefix scores of this step on the side stream (needs the ids the previous step left)
            with torch.cuda.stream(side):
                side.wait_event(ev_ids)
                ctc = proc.ctc_scores(ids[:, :cur_len])
                ev_ctc = torch.cuda.Event()
                ev_ctc.record(side)
            ctc.record_stream(main)            # allocated on the side stream, read by the main stream below: the only tensor of the loop that crosses streams
        lm_logits = lm_lse = None
        if lm_st is not None:                  # the LM's step of this token on its own stream (needs the new tokens and beam indices the previous step left)
            with torch.cuda.stream(lm_st):
                lm_st.wait_event(ev_ids)
                if lm_idx is not None:
                    lm.reorder_cache(lm_cache, lm_idx)
                lm_logits = lm.step(new_tok, lm_cache)
                lm_lse = ops.row_lse(lm_logits)
                ev_lm = torch.cuda.Event()
                ev_lm.record(lm_st)
            new_tok.record_stream(lm_st)       # allocated on the main stream, read on the LM's
            if lm_idx is not None:
                lm_idx.record_stream(lm_st)
            lm_logits.record_stream(main)      # allocated on the LM's stream, read by the main stream below
            lm_lse.record_stream(main)
        logits = joint.dec.step(new_tok, cache, kvs, T2, key_rep, beams=kv_beams)       # (B*W, V), row stride padded to 8
        lse = ops.row_lse(logits)
        if lm is not None and lm_st is None:
            if lm_idx is not None:
                lm.reorder_cache(lm_cache, lm_idx)
            lm_logits = lm.step(new_tok, lm_cache)
            lm_lse = ops.row_lse(lm_logits)
        if proc is not None:
            main.wait_event(ev_ctc)
        if lm_st is not None:
            main.wait_event(ev_lm)
        new_tok = torch.empty((n_bh, 1), dtype=torch.long, device=dev)
        beam_idx = torch.empty((n_bh,), dtype=torch.long, device=dev)
        top_s = top_i = None
        if trace is not None:
            top_s, top_i = torch.empty((B, 2 * W), device=dev), torch.empty((B, 2 * W), dtype=torch.int32, device=dev)
            trace.append((top_s, top_i, done.clone()))          # the done flags BEFORE the step
        denom, heur, es_mode = _stop_rule(W, cur_len, max_length, length_penalty, early_stopping)
        step_args = (logits.data_ptr(), logits.stride(0), lse.data_ptr(), ctc.data_ptr() if ctc is not None else None, w_att, w_ctc, int(proc is not None), pad,
                     eos_token_id, B, W, V, cur_len, max_length, Lmax, denom, heur, es_mode, ids.data_ptr(), beam_scores.data_ptr(), new_tok.data_ptr(),
                     beam_idx.data_ptr(), done.data_ptr(), nfin.data_ptr(), fin_score.data_ptr(), fin_len.data_ptr(), fin_tok.data_ptr(),
                     top_s.data_ptr() if top_s is not None else None, top_i.data_ptr() if top_i is not None else None, done_host[steps].data_ptr())
        if route == "device_wide":
            lm_args = (lm_logits.data_ptr(), lm_logits.stride(0), lm_lse.data_ptr(), w_lm) if lm is not None else (None, 0, None, 0.0)
            _lib.check(L_.mi_beam_step_wide(*step_args, *lm_args, main.cuda_stream), "mi_beam_step_wide")
        elif lm is None:
            _lib.check(L_.mi_beam_step(*step_args, main.cuda_stream), "mi_beam_step")
        else:
            _lib.check(L_.mi_beam_step_lm(*step_args, lm_logits.data_ptr(), lm_logits.stride(0), lm_lse.data_ptr(), w_lm, main.cuda_stream), "mi_beam_step_lm")
        ev_ids = torch.cuda.Event()
        ev_ids.record(main)
        if W > 1:
            joint.dec.reorder_cache(cache, beam_idx)
            lm_idx = beam_idx
        flags.append((ev_ids, steps))          # the flags of this step are in pinned memory once the step's event has fired
        cur_len += 1
        steps += 1
    if stats is not None:                      # host time spent enqueuing the token loop (the GPU may still be running it)
        stats["host_loop_ms"] = (time.perf_counter() - t_loop) * 1e3
        stats["steps"] = steps
        stats["route"] = route
        stats["kv_beams"] = kv_beams
    if side is not None:
        main.wait_stream(side)
    if lm_st is not None:
        main.wait_stream(lm_st)
    nfin_c, fs_c, fl_c, ft_c = nfin.cpu(), fin_score.cpu(), fin_len.cpu(), fin_tok.cpu()             # the first copy synchronises with everything enqueued
    out = []
    for b in range(B):                         # every utterance ends with kept hypotheses: at max_length the step's first W candidates all stop
        hyps = [(float(fs_c[b, k]), ft_c[b, k, :int(fl_c[b, k])].tolist()) for k in range(int(nfin_c[b]))]
        out.append(dict(tokens=hyps[0][1], score=hyps[0][0], hypotheses=hyps))
    return out


def generate_stepwise(joint: "JointAEDEngine", feats, feat_len, *, num_beams=1, max_length=64, ctc_weight=0.3, length_penalty=1.0, early_stopping=False,
                      eos_token_id=1, pad_token_id=None, start_token_id=None, space_token_id=-1, apply_eos_space_trick=False, eos_space_trick_weight=1.0,
                      lm=None, lm_weight=0.0, share_cross_kv=None):
    """The same decoding with the beam bookkeeping on the host, one token at a time (two device -> host copies and three host -> device copies per token): the form the
    reference's generate() has, kept as the cross-check of `generate` (tests/test_gpu_config5.py, tests/test_gpu_aed.py compare the two hypothesis for hypothesis) and as
    the route of the eos / space trick (the processor applies it, ctc_scorer.py:333-349).  With `lm` / `lm_weight` it adds the shallow-fusion term the way the reference's
    processor does (shallow_fussion.py:50-51), in the kernel's arithmetic: one fp32 subtract, one multiply, one add."""
    import numpy as np
    from .decoding import CTCRescorerLogitsProcessor
    lm = _check_generate_args(joint, num_beams, max_length, early_stopping, lm, lm_weight)
    dev = joint.device
    c = joint.jcfg
    pad = c["pad_token_id"] if pad_token_id is None else pad_token_id
    start = c["decoder_start_token_id"] if start_token_id is None else start_token_id
    W = num_beams
    enc_out, enc_bf, T2, key_len = joint.encode(feats, feat_len)
    B = feats.shape[0]
    kvs, key_rep, kv_beams = _beam_cross_kv(joint, enc_bf, key_len, B, W, T2, share_cross_kv)          # `generate`'s arrangement (share_cross_kv=False: one copy per beam)
    cache = joint.dec.init_cache(B * W, max_length + 1)
    lm_cache = lm.init_cache(B * W, max_length + 1) if lm is not None else None
    proc = None
    if ctc_weight > 0:
        lens = enc_out["outer_len"].clamp(max=T2)
        proc = CTCRescorerLogitsProcessor(enc_out["logits"], lens, pad, eos_token_id, 0, ctc_weight, W, space_token_id, bool(apply_eos_space_trick), eos_space_trick_weight)
    ids = torch.full((B * W, 1), start, dtype=torch.long, device=dev)
    beam_scores = torch.zeros((B, W), device=dev)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    kept = [[] for _ in range(B)]              # (score fp32, tokens), best first, at most W
    done = [False] * B
    new_tok = ids
    V = joint.dec.w["lm_head"].shape[0]
    NEG = np.float32(-1.0e9)
    while ids.shape[1] < max_length and not all(done):
        logits = joint.dec.step(new_tok, cache, kvs, T2, key_rep, beams=kv_beams)       # (B*W, V)
        scores = logits - ops.row_lse(logits.contiguous())[:, None]                      # log_softmax
        if proc is not None:
            scores = proc(ids, scores.clone())
        if lm is not None:                                                               # LMRescorerLogitsProcessor: scores + lm_weight * log_softmax(lm logits)
            lm_logits = lm.step(new_tok, lm_cache)
            lm_scores = lm_logits - ops.row_lse(lm_logits.contiguous())[:, None]
            scores = scores + float(lm_weight) * lm_scores
        cand = (scores + beam_scores[:, None]).view(B, W * V)
        top_s, top_i = cand.topk(2 * W, dim=1)
        top_s, top_i = top_s.cpu().numpy(), top_i.cpu().numpy()
        cur_len = ids.shape[1]
        at_max = cur_len + 1 >= max_length
        denom, heur, es_mode = _stop_rule(W, cur_len, max_length, length_penalty, early_stopping)
        denom, heur = np.float32(denom), np.float32(heur)
        nb_scores = torch.zeros((B, W)); nb_tok = torch.zeros((B, W), dtype=torch.long); nb_idx = torch.zeros((B, W), dtype=torch.long)
        ids_cpu = ids.cpu()
        for b in range(B):
            if done[b]:
                nb_scores[b] = 0; nb_tok[b] = pad; nb_idx[b] = b * W
                continue
            rows = [(np.float32(top_s[b, r]), int(top_i[b, r]) // V, int(top_i[b, r]) % V) for r in range(2 * W)]
            hit = [tok == eos_token_id or at_max for _, _, tok in rows]
            nxt = [(s, beam, tok) for (s, beam, tok), h in zip(rows, hit) if not h][:W]
            nxt += [(np.float32(s + NEG), beam, tok) for (s, beam, tok), h in zip(rows, hit) if h][:W - len(nxt)]
            for k, (s, beam, tok) in enumerate(nxt):
                nb_scores[b, k], nb_tok[b, k], nb_idx[b, k] = float(s), tok, b * W + beam
            for r in range(W):
                if hit[r]:
                    s, beam, tok = rows[r]
                    sc = np.float32(s / denom)
                    pos = len(kept[b])
                    while pos > 0 and sc > kept[b][pos - 1][0]:
                        pos -= 1
                    if pos < W:
                        kept[b].insert(pos, (sc, ids_cpu[b * W + beam].tolist() + [tok]))
                        del kept[b][W:]
            best = np.float32(nxt[0][0] / heur)
            unsat = best > (kept[b][W - 1][0] if len(kept[b]) == W else NEG)
            if (not unsat) or (es_mode == 1 and len(kept[b]) == W) or at_max:
                done[b] = True
        beam_idx = nb_idx.view(-1).to(dev)
        new_tok = nb_tok.view(-1, 1).to(dev)
        beam_scores = nb_scores.view(-1).to(dev)
        ids = torch.cat([ids.index_select(0, beam_idx), new_tok], 1)
        joint.dec.reorder_cache(cache, beam_idx)
        if lm is not None:
            lm.reorder_cache(lm_cache, beam_idx)
    return [dict(tokens=kept[b][0][1], score=float(kept[b][0][0]), hypotheses=[(float(s), t) for s, t in kept[b]]) for b in range(B)]


# ---------------------------------------------------------------------------------------------------------------------
# Two-pass joint decoding ("attention rescoring"; DESIGN.md §4 'Two-pass decoding'): the CTC head's n-best (ops.ctc_beam_decode), ONE teacher-forced decoder pass over
# all hypotheses of the batch (GPT2DecoderEngine.token_nll) and a ranking by the objective `generate` maximises,
#     score(h) = (w log p_ctc(h) + (1 - w) sum_u log p_att(h_u | h_<u, x)) / (|h| + 1) ** length_penalty        (the sum over the tokens and the closing EOS)
# (csrc/rescore.hip).  At EOS `generate`'s prefix scorer holds the full-sequence CTC probability, and a hypothesis of |h| tokens closes with the denominator
# `_step_denoms(|h| + 1, ...)`: a hypothesis gets here the score `generate` would give it, up to rounding — and up to the CTC term's source: the beam search's score is
# the mass of the alignments it kept (at most the exact probability, ops.ctc_loss's, which `score` uses), and its blank is the CTC head's last class (`generate` takes
# `pad_token_id`, the same class in every recipe).  No counterpart in the reference.
RESCORE_MAXN = 64                          # csrc/rescore.hip RS_MAXN, csrc/ctc_beam.hip's beam limit


def _check_rescore_args(joint, feats, *, num_beams, nbest, ctc_weight, max_length, num_return, who):
    """every refusal of `rescore` / `score`, on the host, before the device is touched; -> (nbest, num_return)"""
    for name, v in (("num_beams", num_beams), ("nbest", nbest), ("num_return", num_return), ("max_length", max_length)):
        if v is not None and (not isinstance(v, int) or isinstance(v, bool)):
            raise ValueError(f"{who}: {name} must be an int, got {v!r}")
    if not 1 <= num_beams <= RESCORE_MAXN:
        raise ValueError(f"{who}: num_beams must be in 1..{RESCORE_MAXN}, got {num_beams}")
    nbest = num_beams if nbest is None else nbest
    if not 1 <= nbest <= num_beams:
        raise ValueError(f"{who}: nbest must be in 1..num_beams, got {nbest} with {num_beams} beams")
    if not 0.0 <= float(ctc_weight) <= 1.0:                # (a NaN fails both comparisons)
        raise ValueError(f"{who}: ctc_weight must be in [0, 1], got {ctc_weight}")
    if max_length is None or max_length < 2:
        raise ValueError(f"{who}: max_length >= 2 required, got {max_length}")
    num_return = nbest if num_return is None else num_return
    if not 1 <= num_return <= nbest:
        raise ValueError(f"{who}: num_return must be in 1..nbest, got {num_return} with nbest = {nbest}")
    if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
        raise RuntimeError(f"{who}: inputs must be on the GPU; there is no CPU fallback")
    V, V1 = joint.dec.w["lm_head"].shape[0], joint.enc.cfg["vocab_size"] + 1
    if V1 != V:
        raise ValueError(f"CTC head has {V1} classes, the decoder {V}: joint decoding needs one vocabulary")
    return nbest, num_return


def _length_denoms(U, length_penalty):
    """denom[l] = fp32(l ** length_penalty), l = 0..U: `_step_denoms`' closing denominator of a hypothesis of l generated tokens (the closing EOS included)"""
    import numpy as np
    return [float(np.float32(float(l) ** float(length_penalty))) for l in range(U + 1)]


def ctc_term(logits, lens, hyps, lse=None):
    """log p_ctc of GIVEN hypotheses: logits (B, T, V + 1) the CTC head's (blank = the last class), lens (B) int32 the frames that count, hyps (B, N, Tt) int64 with
    negative entries as padding -> (B, N) fp32 = -ops.ctc_loss(reduction="none") per hypothesis; an infeasible one (an infinite loss; a token that is no CTC class): -inf."""
    B, N, Tt = hyps.shape
    V1 = logits.shape[2]
    if lse is None:
        lse = ops._row_lse_3d(logits) if logits.stride(2) == 1 else None
    bad = (hyps >= V1 - 1).any(-1)
    lab = hyps.clamp(max=V1 - 2)
    cols = []
    for n in range(N):
        _, nll, _ = ops.ctc_loss(logits, lab[:, n].contiguous(), lens, reduction="none", zero_infinity=False, lse=lse)
        cols.append(nll)
    out = -torch.stack(cols, 1)
    return torch.where(bad | ~torch.isfinite(out), torch.full_like(out, float("-inf")), out).contiguous()


def _rescore_pass(joint, enc_bf, T2, key_len, nb_tokens, nb_n, nb_ctc, nb_frames, *, K, ctc_weight, length_penalty, max_length, eos, pad, start, trace, marks):
    """pack -> token_nll -> select -> the per-utterance dictionaries (shared by `rescore` and `score`)"""
    B, N, _ = nb_tokens.shape
    V = joint.dec.w["lm_head"].shape[0]
    longest = int(nb_n.max())                              # the one device -> host copy before the results: it sizes the pass
    U = max(1, min(longest + 1, max_length - 1))
    joint.dec.ensure_positions(U)
    pk = ops.rescore_pack(nb_tokens, nb_n, nb_ctc, vocab=V, U=U, start_id=start, eos_id=eos, pad_id=pad)
    nll = joint.dec.token_nll(pk["ids"], pk["labels"], enc_bf, T2, key_len, N)
    marks("decoder_pass")
    denom = torch.tensor(_length_denoms(U, length_penalty), dtype=torch.float32).to(joint.device)
    w_ctc, w_att = float(ctc_weight), float(1 - ctc_weight)            # `generate`'s two weights, as it forms them
    sel = ops.rescore_select(nll, pk["len"], nb_ctc, denom, nb_tokens, w_ctc=w_ctc, w_att=w_att, K=K, eos_id=eos, pad_id=pad, frames=nb_frames)
    marks("select")
    if trace is not None:
        trace.update(tokens=nb_tokens, n_tokens=nb_n, ctc=nb_ctc, frames=nb_frames, ids=pk["ids"], labels=pk["labels"], len=pk["len"], nll=nll, U=U, denom=denom,
                     w_ctc=w_ctc, w_att=w_att, select=sel)
    c = {k: v.cpu() for k, v in sel.items()}               # the first copy synchronises with everything enqueued
    out = []
    for b in range(B):
        hyps, tlp, frs = [], [], []
        for k in range(K):
            n = int(c["n_tokens"][b, k])
            hyps.append((float(c["total"][b, k]), [start] + c["tokens"][b, k, :n + 1].tolist()))
            tlp.append(c["token_lp"][b, k, :n + 1].tolist())
            frs.append(c["frames"][b, k, :n].tolist() if "frames" in c else None)
        out.append(dict(tokens=hyps[0][1], score=hyps[0][0], hypotheses=hyps, ctc_score=c["ctc"][b].tolist(), att_score=c["att"][b].tolist(), token_logprobs=tlp,
                        frames=frs, order=c["order"][b].tolist()))
    return out


def _stage_marks(stats):
    """-> (mark(name), finish()): device-side time per stage into `stats` (events on the current stream; nothing is recorded without `stats`)"""
    if stats is None:
        return (lambda name: None), (lambda: None)
    evs = [("start", torch.cuda.Event(enable_timing=True))]
    evs[0][1].record()

    def mark(name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append((name, e))

    def finish():
        torch.cuda.current_stream().synchronize()
        for (_, a), (name, b) in zip(evs, evs[1:]):
            stats[name + "_ms"] = a.elapsed_time(b)
    return mark, finish


def rescore(joint: "JointAEDEngine", feats, feat_len, *, num_beams, nbest=None, token_topk=None, ctc_weight=0.3, length_penalty=1.0, max_length=64, num_return=None,
            eos_token_id, pad_token_id=None, start_token_id=None, stats=None, trace=None):
    """Two-pass joint decoding: `joint.encode`, the CTC prefix beam search over the encoder logits (`num_beams` hypotheses, the `nbest` best kept; lengths =
    outer_len.clamp(max=T'), what `generate` gives its prefix scorer), one teacher-forced decoder pass over all B * nbest hypotheses, ranking by the joint objective.
    U = min(longest hypothesis + 1, max_length - 1) positions; a hypothesis that does not fit is dropped (ops.rescore_pack).  Returns per utterance what `generate`
    returns — dict(tokens = [start, ..., eos], score, hypotheses = the `num_return` (default nbest) best (score, tokens), best first) — plus, aligned with `hypotheses`,
    ctc_score, att_score, token_logprobs (per token and the closing EOS), frames (the CTC search's frame per token) and order (index into the CTC n-best).  Entries past
    the hypotheses that exist: [start, eos] with score -inf (an utterance with none yields that as its result).  One device -> host copy (the longest hypothesis) before
    the results are read.  `stats` (a dict) receives the device time per stage in ms (encoder, ctc_beam, decoder_pass, select); `trace` (a dict) the device tensors of
    the pass (the n-best, the packed operands, nll, the select's outputs)."""
    nbest, num_return = _check_rescore_args(joint, feats, num_beams=num_beams, nbest=nbest, ctc_weight=ctc_weight, max_length=max_length, num_return=num_return,
                                            who="rescore")
    c = joint.jcfg
    pad = c["pad_token_id"] if pad_token_id is None else pad_token_id
    start = c["decoder_start_token_id"] if start_token_id is None else start_token_id
    mark, finish = _stage_marks(stats)
    enc_out, enc_bf, T2, key_len = joint.encode(feats, feat_len)
    mark("encoder")
    lens = enc_out["outer_len"].clamp(max=T2)
    nb = ops.ctc_beam_decode(enc_out["logits"], joint.enc.cfg["vocab_size"], pad, lens, beams=num_beams, token_topk=token_topk, nbest=nbest, return_frames=True)
    mark("ctc_beam")
    out = _rescore_pass(joint, enc_bf, T2, key_len, nb["tokens"], nb["n_tokens"], nb["scores"], nb["frames"], K=num_return, ctc_weight=ctc_weight,
                        length_penalty=length_penalty, max_length=max_length, eos=eos_token_id, pad=pad, start=start, trace=trace, marks=mark)
    finish()
    return out


def score(joint: "JointAEDEngine", feats, feat_len, hyps, *, ctc_weight=0.3, length_penalty=1.0, max_length=64, eos_token_id, pad_token_id=None, start_token_id=None,
          stats=None, trace=None):
    """The joint objective of GIVEN hypotheses: hyps (B, N, Tt) int64 on the device, N <= 64, a hypothesis' tokens first (no start / EOS), then negative entries as
    padding.  The CTC term is -ops.ctc_loss(reduction="none") (the exact full-sequence log-probability; infeasible: -inf), the decoder pass and the ranking are
    `rescore`'s with every hypothesis returned (K = N).  Returns `rescore`'s dictionaries (`order` indexes `hyps`; `frames` entries are None)."""
    if not isinstance(hyps, torch.Tensor) or hyps.dtype != torch.int64 or hyps.dim() != 3 or hyps.shape[0] != feats.shape[0] or hyps.shape[2] < 1:
        raise ValueError(f"score: hyps must be ({feats.shape[0]}, N, Tt) int64")
    N = int(hyps.shape[1])
    _check_rescore_args(joint, feats, num_beams=N, nbest=N, ctc_weight=ctc_weight, max_length=max_length, num_return=N, who="score")
    if not hyps.is_cuda:
        raise RuntimeError("score: hyps must be on the GPU; there is no CPU fallback")
    c = joint.jcfg
    pad = c["pad_token_id"] if pad_token_id is None else pad_token_id
    start = c["decoder_start_token_id"] if start_token_id is None else start_token_id
    hyps = hyps.contiguous()
    mark, finish = _stage_marks(stats)
    enc_out, enc_bf, T2, key_len = joint.encode(feats, feat_len)
    mark("encoder")
    lens = enc_out["outer_len"].clamp(max=T2)
    ctc = ctc_term(enc_out["logits"], lens, hyps, enc_out.get("lse"))
    mark("ctc_loss")
    n_tok = (hyps >= 0).sum(-1).to(torch.int32)
    out = _rescore_pass(joint, enc_bf, T2, key_len, hyps, n_tok, ctc, None, K=N, ctc_weight=ctc_weight, length_penalty=length_penalty, max_length=max_length,
                        eos=eos_token_id, pad=pad, start=start, trace=trace, marks=mark)
    finish()
    return out
