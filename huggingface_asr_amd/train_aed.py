"""Training step of the joint CTC/attention encoder-decoder on the HIP path (BASELINE config 3).

Differentiates what `huggingface_asr_amd.decoder.JointAEDEngine.forward` computes, i.e. the reference's
`JointCTCAttentionEncoderDecoder.forward` (src/models/ctc_encoder_plus_autoregressive_decoder.py:237-358) with its
`GPT2LMMultiHeadModel` decoder (src/models/decoders/multi_head_gpt2.py:80-170: auxiliary heads, shifted label-smoothed CE) and
the transformers GPT-2 block (ln_1 -> causal self-attention -> ln_cross_attn -> cross-attention over the encoder frames -> ln_2 ->
gelu_new MLP):   loss = w * CTC + (1 - w) * sum_k head_weight_k * CE_k.

The encoder side is `train.EncoderCTCTrainer`; the decoder hooks into its backward at the encoder output (`extra_hidden_grad`),
so, with `GradSync(overlap=True)`, the encoder's per-layer gradient all-reduces still overlap the remaining backward.  Same precision model and the same
restrictions as train.py; GPT-2's embd / attn / resid dropouts use the same counter-based masks (decoder layer l = stream layer 32 + l).
"""
from __future__ import annotations

from collections import namedtuple

import torch

from . import ops
from . import ops_train as T
from .decoder import _sinusoid_table, shift_tokens_right
from .packing import _dec_map, decoder_specs
from .train import BF16, F32, EncoderCTCTrainer, GradSync, ParamStore, ZeroCopyTrainer


def attention_bwd_fused(q, k, v, ctx, dctx, lse, dq, dk, dv, B, Tq, Tk, H, *, lengths=None, causal=False, drop=None):
    """Backward of `ops_train.attention_x_lse` (head size 64 / 128): ONE walk recomputes the probabilities, leaves P (dropped) and dS in bf16 and accumulates dQ = dS K on the
    way (mi_attention_x_bwd_probs); dV = P^T dctx and dK = dS^T q stay batched GEMMs over them.  Three launches where the materialised path (tests/helpers.py) has seven."""
    d = dctx.shape[1]
    hd = d // H
    prob, ds = T.attn_x_bwd_probs(q, k, v, B, Tq, Tk, H, ctx, dctx, lse, dq, lengths=lengths, causal=causal, drop=drop)
    Ts = prob.shape[-1]
    sS = (B * Tq * Ts, Tq * Ts)
    sd_, sq = dctx.stride(0), q.stride(0)
    T.bgemm(prob, (*sS, 1, Ts), dctx, (hd, Tq * sd_, 1, sd_), dv, (hd, Tk * dv.stride(0), dv.stride(0)), H, B, Tk, hd, Tq, m_valid=lengths)
    T.bgemm(ds, (*sS, 1, Ts), q, (hd, Tq * sq, 1, sq), dk, (hd, Tk * dk.stride(0), dk.stride(0)), H, B, Tk, hd, Tq, m_valid=lengths)


# what one decoder call works on: B utterances of U tokens (M = B*U rows) over T2 encoder frames (Me = B*T2 rows, `key_len` of them valid per utterance or None), the
# shifted input ids, the gradient scale, and the encoder states in bf16 as they came (hb) and at the decoder width (enc_bf)
_DecStep = namedtuple("_DecStep", "B U T2 M Me key_len ids labels gs enc_bf hb")


class JointAEDTrainer(ZeroCopyTrainer):
    """forward + backward + AdamW for JointCTCAttentionEncoderDecoder (E-Branchformer encoder + multi-head GPT-2 decoder)."""

    def __init__(self, enc_cfg: dict, dec_cfg: dict, joint_cfg: dict, device="cuda:0", *, lr=2e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, max_grad_norm=1.0, group=None, with_proj=None, dp_sync=True, seed=0):
        c = self.dcfg = dict(dec_cfg)
        self.jcfg = dict(joint_cfg)
        self.device = torch.device(device)
        d, H = c["n_embd"], c["n_head"]
        if d // H not in (64, 128):                            # the LDS-staged attention kernels' head sizes
            raise NotImplementedError("HIP decoder attention supports head sizes 64 and 128")
        if c.get("activation_function", "gelu_new") != "gelu_new":
            raise NotImplementedError("decoder MLP activation other than gelu_new")
        self.d, self.H, self.L, self.V, self.Vp = d, H, c["n_layer"], c["vocab_size"], T.pad64(c["vocab_size"])
        self.eps = float(c.get("layer_norm_epsilon", 1e-5))
        self.locs = list(c.get("head_locations") or [])
        self.weights = list(c.get("head_weights") or [1.0])
        self.lsm = float(c.get("lsm_factor", 0.0))
        self.lm_name = "wte" if c.get("tie_word_embeddings", False) else "lm_head"
        self.wdec = 1.0 - self.jcfg["ctc_weight"]
        self.pe, self.pa, self.pr = (float(c.get(k, 0.0) or 0.0) for k in ("embd_pdrop", "attn_pdrop", "resid_pdrop"))
        self.enc = EncoderCTCTrainer(enc_cfg, device, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm, group=group,
                                     dp_sync=dp_sync, seed=seed)
        enc_dim = enc_cfg["hidden_size"]
        self.with_proj = (enc_dim != d) if with_proj is None else with_proj
        self.store = ParamStore(decoder_specs(c, enc_dim, self.with_proj), self.device, _dec_map(c, self.with_proj))
        self.sync = GradSync(self.store.flat_g, group, enabled=dp_sync)
        self.hp, self._scal = self.enc.hp, self.enc._scal
        if c.get("pos_emb_fixed", False):
            self.pos_fixed, self.emb_scale = _sinusoid_table(c.get("n_positions", 1024), d, self.device), float(d) ** 0.5
        else:
            self.pos_fixed, self.emb_scale = None, 1.0

    # ------------------------------------------------------------------ weights (the encoder's reference keys carry an `encoder.` prefix)
    def _named_stores(self):
        return [("encoder.", self.enc.store), ("", self.store)]

    def syncs(self):
        return [self.enc.sync, self.sync]

    def set_frozen(self, reference_names):
        """frozen encoder parameters (freeze_encoder): their weight-gradient GEMMs are skipped and, on the native route, AdamW leaves them
        untouched (train.EncoderCTCTrainer.set_frozen); decoder parameters always train"""
        self.enc.set_frozen({k[len("encoder."):] for k in (reference_names or ()) if k.startswith("encoder.")})

    # ------------------------------------------------------------------ decoder forward + backward (called inside the encoder's backward)
    def _decoder(self, last_hidden, B, T2, key_len, labels, out, gs):
        """last_hidden (B*T2, d_enc) f32.  Fills out[...] and returns d(loss)/d(last_hidden) f32 (gradients scaled by gs)."""
        st = self.store
        x, sp = self._embed_fwd(last_hidden, B, T2, key_len, labels, gs)
        saved, taps = [], {}
        if 0 in self.locs:
            taps[0] = x
        for l in range(self.L):
            x, S = self._layer_fwd(x, l, sp)
            saved.append(S)
            if (l + 1) in self.locs and l + 1 < self.L:
                taps[l + 1] = x
        tnb = T.TnBatch()            # every weight gradient of the decoder's backward: one grouped launch at the end (46 problems, ~150 output tiles at 6 x 256)
        # first backward after zero_grad: the launch writes its targets instead of adding into the zeros (train.EncoderCTCTrainer._forward_backward); the embedding
        # gradient — the one other contribution to a matrix of this store (wte, tied to the lm head) — is therefore added AFTER the flush (_embed_bwd)
        tnb.overwrite = st.fresh
        st.fresh = False
        dx, tap_grads, dec_loss, logits = self._heads(x, taps, sp, tnb)
        denc = torch.zeros((sp.Me, self.d), device=self.device, dtype=F32)      # every layer's cross-attention adds its share, from L-1 down
        for l in range(self.L - 1, -1, -1):
            if (l + 1) in tap_grads:
                T.axpy_(dx, tap_grads[l + 1])
            self._layer_bwd(dx, denc, saved[l], l, sp, tnb)
        dh = self._embed_bwd(dx, denc, tap_grads.get(0), sp, tnb)
        out.update(dec_loss=dec_loss, logits=logits, encoder_hidden=sp.enc_bf)
        return dh

    def _e16(self, *sh):
        return torch.empty(sh, device=self.device, dtype=BF16)

    def _att_drop(self, l, site):
        """the attention-probability dropout argument of decoder layer l (site 0: self-attention, 2: cross-attention), forward and backward alike"""
        return (self.pa, self.enc.seed, self.enc._sid(32 + l, site)) if self.pa > 0 else None

    def _resid_add(self, res, a16, wname, bname, l, site):
        """res + dropout(a16 W^T + b)"""
        W, P = self.store.bf, self.store.p
        if self.pr > 0:
            return T.dropout_add(res, ops.gemm(a16, W(wname), P(bname), out_dtype=F32), 1.0, self.pr, self.enc.seed, self.enc._sid(32 + l, site))
        return ops.gemm(a16, W(wname), P(bname), out_dtype=F32, resid=res, alpha=1.0)

    def _dres(self, dx, l, site):
        """the gradient arriving at a residual branch's output, in bf16: dx through that site's dropout mask"""
        if self.pr > 0:
            return T.dropout_(dx, self.pr, self.enc.seed, self.enc._sid(32 + l, site), out=self._e16(*dx.shape))
        return T.add_cast(dx)

    def _embed_fwd(self, last_hidden, B, T2, key_len, labels, gs):
        """encoder states at the decoder width, token + position embedding, embedding dropout -> (x (M, d) f32, the call's `_DecStep` record)"""
        P, W, jc = self.store.p, self.store.bf, self.jcfg
        ids = shift_tokens_right(labels, jc["pad_token_id"], jc["decoder_start_token_id"])
        U = ids.shape[1]
        # encoder states at the decoder width (ctc_encoder_plus...:289-293)
        hb = ops.cast_bf16(last_hidden)
        enc_bf = ops.gemm(hb, W("proj_w"), P("proj_b")) if self.with_proj else hb
        pos = self.pos_fixed if self.pos_fixed is not None else P("wpe")
        x = ops.embed_tokens(ids, P("wte"), pos, scale=self.emb_scale)
        if self.pe > 0:
            T.dropout_(x, self.pe, self.enc.seed, self.enc._sid(63, 0))
        return x, _DecStep(B, U, T2, B * U, B * T2, key_len, ids, labels, gs, enc_bf, hb)

    def _layer_fwd(self, x, l, sp):
        """one GPT-2 block with cross-attention -> (output, what its backward reads)"""
        P, W = self.store.p, self.store.bf
        B, U, T2, M, d, H, eps = sp.B, sp.U, sp.T2, sp.M, self.d, self.H, self.eps
        LN = ops.layernorm_chain
        p = f"h{l}."
        S = {"x": x}
        a1 = self._e16(M, d)
        LN(x, lna=(P(p + "ln1_g"), P(p + "ln1_b")), eps2=eps, outa=a1)
        qkv = ops.gemm(a1, W(p + "wqkv"), P(p + "bqkv"))
        # fused forward with the row log-sum-exp (and the dropout mask) for the fused backward
        ctx1, lse1 = T.attention_x_lse(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], B, U, U, H, causal=True, drop=self._att_drop(l, 0))
        x1 = self._resid_add(x, ctx1, p + "wo", p + "bo", l, 1)
        a2 = self._e16(M, d)
        LN(x1, lna=(P(p + "lnc_g"), P(p + "lnc_b")), eps2=eps, outa=a2)
        qq = ops.gemm(a2, W(p + "wq"), P(p + "bq"))
        kv = ops.gemm(sp.enc_bf, W(p + "wkv"), P(p + "bkv"))
        ctx2, lse2 = T.attention_x_lse(qq, kv[:, :d], kv[:, d:], B, U, T2, H, lengths=sp.key_len, drop=self._att_drop(l, 2))
        x2 = self._resid_add(x1, ctx2, p + "wco", p + "bco", l, 3)
        a3 = self._e16(M, d)
        LN(x2, lna=(P(p + "ln2_g"), P(p + "ln2_b")), eps2=eps, outa=a3)
        mp = ops.gemm(a3, W(p + "wfc"), P(p + "bfc"))
        mm = T.act_fwd(mp, "gelu_new")
        x3 = self._resid_add(x2, mm, p + "wpr", p + "bpr", l, 4)
        S.update(a1=a1, qkv=qkv, ctx1=ctx1, lse1=lse1, x1=x1, a2=a2, qq=qq, kv=kv, ctx2=ctx2, lse2=lse2, x2=x2, a3=a3, mp=mp, mm=mm)
        return x3, S

    def _head(self, hb16, wname, weight, sp):
        """logits + CE of one head; returns (logits view, loss, dlogits bf16 (M, Vp))"""
        V, Vp = self.V, self.Vp
        buf = torch.empty((sp.B, sp.U, Vp), device=self.device, dtype=F32)
        ops.gemm(hb16, self.store.bf(wname), None, out=buf.view(sp.M, Vp))
        lg = buf[..., :V]
        acc = ops.ce_label_smoothing(lg, sp.labels, shift=1, eps=self.lsm, return_acc=True)
        dl = T.ce_label_smoothing_bwd(lg, sp.labels, acc, shift=1, eps=self.lsm, weight=weight * sp.gs, ldo=Vp)
        return lg, acc[0] / acc[1], dl

    def _heads(self, x, taps, sp, tnb):
        """final LayerNorm, the last head and the intermediate heads with their losses, and what they send back: -> (dx (M, d) f32 at the last layer's output,
        {location: f32 gradient at that tap}, decoder loss, the last head's logits)"""
        P, G, WT = self.store.p, self.store.g, self.store.bfT
        V, weights, wdec, lm_name = self.V, self.weights, self.wdec, self.lm_name
        hid = self._e16(sp.M, self.d)
        ops.layernorm_chain(x, lna=(P("lnf_g"), P("lnf_b")), eps2=self.eps, outa=hid)
        logits, ce, dl = self._head(hid, lm_name, wdec * weights[-1], sp)
        dec_loss = weights[-1] * ce
        # ---- backward of the last head
        dhid = ops.gemm(dl, WT(lm_name))
        T.gemm_tn_(G(lm_name), dl, hid, n_store=V, defer=tnb)
        tap_grads, final_dys = {}, [dhid]
        for k, loc in enumerate(self.locs):
            src16 = ops.cast_bf16(taps[loc]) if loc in taps else hid
            _, ce_k, dl_k = self._head(src16, f"head{k}", wdec * weights[k], sp)
            dec_loss = dec_loss + weights[k] * ce_k
            T.gemm_tn_(G(f"head{k}"), dl_k, src16, n_store=V, defer=tnb)
            if loc in taps:
                tap_grads[loc] = ops.gemm(dl_k, WT(f"head{k}"), out_dtype=F32)
            else:                                            # a head on the last hidden state reads ln_f's output
                final_dys.append(ops.gemm(dl_k, WT(f"head{k}")))
        dx = torch.empty((sp.M, self.d), device=self.device, dtype=F32)
        for i, dy in enumerate(final_dys):
            T.layernorm_bwd(x, P("lnf_g"), dy, dx, accumulate=i > 0, dgamma=G("lnf_g"), dbeta=G("lnf_b"), eps=self.eps)
        return dx, tap_grads, dec_loss, logits

    def _layer_bwd(self, dx, denc, S, l, sp, tnb):
        """backward of `_layer_fwd`: dx (M, d) f32 becomes the gradient at the block's input in place, the cross-attention's share of the encoder-state gradient is added
        into denc (Me, d) f32, weight gradients are recorded in tnb"""
        P, G, WT = self.store.p, self.store.g, self.store.bfT
        B, U, T2, M, d, H, eps = sp.B, sp.U, sp.T2, sp.M, self.d, self.H, self.eps
        p = f"h{l}."
        # MLP
        dyb = self._dres(dx, l, 4)
        dm = T.linear_bwd(dyb, S["mm"], WT(p + "wpr"), dw=G(p + "wpr"), db=G(p + "bpr"), defer=tnb)
        dmp = T.act_bwd(dm, S["mp"], "gelu_new")
        da3 = T.linear_bwd(dmp, S["a3"], WT(p + "wfc"), dw=G(p + "wfc"), db=G(p + "bfc"), defer=tnb)
        T.layernorm_bwd(S["x2"], P(p + "ln2_g"), da3, dx, accumulate=True, dgamma=G(p + "ln2_g"), dbeta=G(p + "ln2_b"), eps=eps)
        # cross-attention
        dyb = self._dres(dx, l, 3)
        dctx2 = T.linear_bwd(dyb, S["ctx2"], WT(p + "wco"), dw=G(p + "wco"), db=G(p + "bco"), defer=tnb)
        dqq, dkv = self._e16(M, d), self._e16(sp.Me, 2 * d)
        kv = S["kv"]
        attention_bwd_fused(S["qq"], kv[:, :d], kv[:, d:], S["ctx2"], dctx2, S["lse2"], dqq, dkv[:, :d], dkv[:, d:], B, U, T2, H, lengths=sp.key_len,
                            drop=self._att_drop(l, 2))
        da2 = T.linear_bwd(dqq, S["a2"], WT(p + "wq"), dw=G(p + "wq"), db=G(p + "bq"), defer=tnb)
        T.linear_bwd(dkv, sp.enc_bf, WT(p + "wkv"), dw=G(p + "wkv"), db=G(p + "bkv"), need_dx=False, defer=tnb)
        ops.gemm(dkv, WT(p + "wkv")[:, :2 * d], out=denc, resid=denc, alpha=1.0)
        T.layernorm_bwd(S["x1"], P(p + "lnc_g"), da2, dx, accumulate=True, dgamma=G(p + "lnc_g"), dbeta=G(p + "lnc_b"), eps=eps)
        # causal self-attention
        dyb = self._dres(dx, l, 1)
        dctx1 = T.linear_bwd(dyb, S["ctx1"], WT(p + "wo"), dw=G(p + "wo"), db=G(p + "bo"), defer=tnb)
        qkv = S["qkv"]
        dqkv = self._e16(M, 3 * d)
        attention_bwd_fused(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], S["ctx1"], dctx1, S["lse1"], dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:], B, U, U, H,
                            causal=True, drop=self._att_drop(l, 0))
        da1 = T.linear_bwd(dqkv, S["a1"], WT(p + "wqkv"), dw=G(p + "wqkv"), db=G(p + "bqkv"), defer=tnb)
        T.layernorm_bwd(S["x"], P(p + "ln1_g"), da1, dx, accumulate=True, dgamma=G(p + "ln1_g"), dbeta=G(p + "ln1_b"), eps=eps)

    def _embed_bwd(self, dx, denc, tap0, sp, tnb):
        """backward of `_embed_fwd` (tap0: the gradient of a head on the embedding output, or None); runs the recorded weight gradients and starts the all-reduce
        -> d(loss)/d(last_hidden) f32"""
        G, WT = self.store.g, self.store.bfT
        if tap0 is not None:
            T.axpy_(dx, tap0)
        if self.pe > 0:
            T.dropout_(dx, self.pe, self.enc.seed, self.enc._sid(63, 0))
        if self.with_proj:
            dh = T.linear_bwd(T.add_cast(denc), sp.hb, WT("proj_w"), dw=G("proj_w"), db=G("proj_b"), dx_dtype=F32, defer=tnb)
        else:
            dh = denc
        tnb.flush()
        # after the flush: on the first backward after zero_grad the flush OVERWRITES its targets, and wte may be one of them (tied to the lm head)
        T.embed_tokens_bwd(sp.ids, dx, G("wte"), None if self.pos_fixed is not None else G("wpe"), scale=self.emb_scale, heavy_id=self.jcfg.get("pad_token_id"))
        self.sync.launch(0, self.store.n)
        return dh

    # ------------------------------------------------------------------ mixing fine-tuning: the frozen body, forward stages only
    def forward_heads(self, feats, feat_lengths, labels):
        """The forward stages alone, in training mode (the dropouts of the configuration), no backward: what the mixing fine-tuning of the DeCRED decoder needs of the
        frozen model (model_utils.py:214-217 freezes everything but `lm_mixing`).  -> dict(enc_loss, encoder_logits, encoder_hidden, head_logits (H, B, U, Vp) f32: the
        logits of every head in `packing.head_taps` order, columns [V, Vp) padding)"""
        with ops.pinned_stream():
            labels = labels.contiguous()
            B = feats.shape[0]
            eo = self.enc._forward_backward(feats, feat_lengths, labels, backward=False, train_mode=True, keep_hidden=True)
            T2 = eo["last_hidden"].shape[1]
            key_len = torch.clamp(eo["outer_len"], max=T2) if feat_lengths is not None else None
            x, sp = self._embed_fwd(eo["last_hidden"].reshape(B * T2, -1), B, T2, key_len, labels, 1.0)
            taps = {0: x} if 0 in self.locs else {}
            for l in range(self.L):
                x, _ = self._layer_fwd(x, l, sp)
                if (l + 1) in self.locs and l + 1 < self.L:
                    taps[l + 1] = x
            hid = self._e16(sp.M, self.d)
            ops.layernorm_chain(x, lna=(self.store.p("lnf_g"), self.store.p("lnf_b")), eps2=self.eps, outa=hid)
            names = [f"head{k}" for k in range(len(self.locs))] + [self.lm_name]
            buf = torch.empty((len(names), sp.B, sp.U, self.Vp), device=self.device, dtype=F32)
            for h, (loc, name) in enumerate(zip(self.locs + [self.L], names)):
                ops.gemm(ops.cast_bf16(taps[loc]) if loc in taps else hid, self.store.bf(name), None, out=buf[h].view(sp.M, self.Vp))
            return dict(enc_loss=eo["loss"], encoder_logits=eo["logits"], encoder_hidden=sp.enc_bf, head_logits=buf)

    # ------------------------------------------------------------------ step
    def forward_backward(self, feats, feat_lengths, labels):
        with ops.pinned_stream():
            return self._forward_backward(feats, feat_lengths, labels)

    def _forward_backward(self, feats, feat_lengths, labels):
        jc = self.jcfg
        labels = labels.contiguous()
        B = feats.shape[0]
        out = {}
        w = jc["ctc_weight"]

        def hook(last_hidden, outer_len):
            T2 = last_hidden.shape[0] // B
            key_len = torch.clamp(outer_len, max=T2) if feat_lengths is not None else None     # cross mask from the OUTER lengths (quirk 8')
            return self._decoder(last_hidden, B, T2, key_len, labels, out, 1.0 / self.sync.world)

        eo = self.enc.forward_backward(feats, feat_lengths, labels, loss_scale=w, extra_hidden_grad=hook)
        out.update(enc_loss=eo["loss"], encoder_logits=eo["logits"], loss=w * eo["loss"] + (1 - w) * out["dec_loss"])
        return out
