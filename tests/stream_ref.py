"""Plain-torch restatement of the streaming recurrences of csrc/stream.hip (whose header states the semantics) on the oracle's ops.

A stream batch of B streams advanced in lock-step: `feed` takes (B, 4*C, F) feature frames, `finish` the last 0..4*C frames with a per-stream count of valid
ones.  Per layer: a K/V cache, the CSGU history of (K-1)*dil normalised rows, the merge history of 2r `cat` rows and at most r pending residual rows; layer l
consumes rows [a_l', a_l) and emits rows [a_{l+1}', a_{l+1}), a_{l+1} = max(0, a_l - r) (a_l in `finish`).  Run in float64 it must equal
R.encoder_forward + R.ctc_head of each utterance alone up to summation order (tests/test_stream_cpu.py); it models no bf16 rounding.
"""
import math

import torch
import torch.nn.functional as F

from huggingface_asr_amd.streaming import plan
from oracle import ebranchformer_ref as R


class RefStream:
    def __init__(self, sd, cfg, batch, chunk_frames, max_frames):
        assert cfg.get("is_causal", False)
        self.sd, self.cfg, self.B, self.C, self.Lmax = sd, cfg, batch, chunk_frames, max_frames
        self.L = cfg["num_hidden_layers"]
        self.r = (cfg.get("merge_conv_kernel", 31) - 1) // 2
        self.kc = cfg.get("csgu_kernel_size", 31)
        self.dil = (self.kc - 1) // 2
        d, H = cfg["hidden_size"], cfg["num_attention_heads"]
        self.ptype = cfg.get("position_embeddings_type", "relative")
        if self.ptype == "relative":          # row `dist` = the sinusoid of relative position i - j = dist (tf:531-536 slices one table around its centre)
            self.dist = R.rel_pos_table(max_frames, d)[:max_frames].flip(0)
        elif self.ptype == "rotary":
            self.rot = R.rotary_table(max_frames, d // H, cfg.get("rotary_embedding_base", 10000))
        self.reset()

    def reset(self):
        c, B = self.cfg, self.B
        d, I = c["hidden_size"], c["intermediate_size"]
        z = lambda *s: torch.zeros(*s)
        self.n_feat = 0
        self.done = False
        self.x_hist = z(B, 1, 2, c.get("num_fbanks", 80))
        self.c1_hist = None                                   # (B, C1, 2, F1) zeros, sized at the first call
        self.layers = [dict(k=z(B, 0, d), v=z(B, 0, d), csgu=z(B, (self.kc - 1) * self.dil, I // 2), cat=z(B, 2 * self.r, 2 * d), pend=z(B, 0, d))
                       for _ in range(self.L)]

    # ---- front end: CausalConv2d twice with the last two rows of each conv's input as history (zero history = the left padding)
    def _front(self, feats):
        sd, c = self.sd, self.cfg
        p = "wav2vec2.feature_extractor."
        lp = c["conv_padding"][0] * 2
        s = c["conv_stride"][0]
        h = torch.cat([self.x_hist, feats[:, None]], dim=2)
        self.x_hist = h[:, :, -2:]
        h = F.gelu(F.conv2d(F.pad(h, (lp, 0, 0, 0)), sd[p + "conv.0.0.weight"], sd[p + "conv.0.0.bias"], stride=s))
        if self.c1_hist is None:
            self.c1_hist = torch.zeros(h.shape[0], h.shape[1], 2, h.shape[3])
        h = torch.cat([self.c1_hist, h], dim=2)
        self.c1_hist = h[:, :, -2:]
        h = F.gelu(F.conv2d(F.pad(h, (lp, 0, 0, 0)), sd[p + "conv.1.0.weight"], sd[p + "conv.1.0.bias"], stride=s))
        h = h.transpose(1, 2).flatten(2, 3)
        h = F.linear(h, sd[p + "out.weight"], sd[p + "out.bias"])
        q = "wav2vec2.feature_projection."
        h = R.layer_norm(h, sd[q + "layer_norm.weight"], sd[q + "layer_norm.bias"], c.get("layer_norm_eps", 1e-5))
        return F.linear(h, sd[q + "projection.weight"], sd[q + "projection.bias"])

    def _attention(self, st, pre, a1, p, a):
        sd, c = self.sd, self.cfg
        B, n, d = a1.shape
        H = c["num_attention_heads"]
        hd = d // H
        xq = a1
        if self.ptype == "rotary":
            xq = R.apply_rotary(a1, self.rot[0][p:a], self.rot[1][p:a], H)
        lin = lambda nme, inp: F.linear(inp, sd[f"{pre}{nme}.weight"], sd[f"{pre}{nme}.bias"])
        st["k"] = torch.cat([st["k"], lin("linear_k", xq)], 1)
        st["v"] = torch.cat([st["v"], lin("linear_v", a1)], 1)
        qh = lin("linear_q", xq).view(B, n, H, hd).transpose(1, 2)
        kh = st["k"].view(B, a, H, hd).transpose(1, 2)
        vh = st["v"].view(B, a, H, hd).transpose(1, 2)
        i = torch.arange(p, a)[:, None]
        j = torch.arange(a)[None, :]
        if self.ptype == "relative":
            pp = F.linear(self.dist[:a], sd[pre + "linear_pos.weight"]).view(a, H, hd).transpose(0, 1)        # (H, dist, hd)
            ac = torch.matmul(qh + sd[pre + "pos_bias_u"][None, :, None, :], kh.transpose(-2, -1))
            bdd = torch.matmul(qh + sd[pre + "pos_bias_v"][None, :, None, :], pp.transpose(-2, -1)[None])     # (B, H, n, dist)
            bd = torch.gather(bdd, 3, (i - j).clamp(min=0)[None, None].expand(B, H, n, a))
            scores = (ac + bd) / math.sqrt(hd)
        else:
            scores = torch.matmul(qh, kh.transpose(-2, -1)) / math.sqrt(hd)
        scores = scores.masked_fill((j > i)[None, None], float("-inf"))
        ctx = torch.matmul(torch.softmax(scores, dim=-1), vh).transpose(1, 2).reshape(B, n, d)
        return lin("linear_out", ctx)

    def _cgmlp(self, st, pre, a2):
        sd, c = self.sd, self.cfg
        h = F.gelu(F.linear(a2, sd[pre + "channel_proj1.0.weight"], sd[pre + "channel_proj1.0.bias"]))
        r_, g = h.chunk(2, dim=-1)
        g = R.layer_norm(g, sd[pre + "csgu.norm.weight"], sd[pre + "csgu.norm.bias"])
        full = torch.cat([st["csgu"], g], 1)
        st["csgu"] = full[:, full.shape[1] - st["csgu"].shape[1]:]
        w = sd[pre + "csgu.conv.weight"]
        g = F.conv1d(full.transpose(1, 2), w, sd[pre + "csgu.conv.bias"], groups=w.shape[0], dilation=self.dil).transpose(1, 2)
        if c.get("csgu_use_linear_after_conv", False):
            g = F.linear(g, sd[pre + "csgu.linear.weight"], sd[pre + "csgu.linear.bias"])
        act = c.get("csgu_activation", "identity")
        if act != "identity":
            g = {"gelu": F.gelu, "relu": F.relu, "silu": F.silu, "swish": F.silu}[act](g)
        return F.linear(r_ * g, sd[pre + "channel_proj2.weight"], sd[pre + "channel_proj2.bias"])

    def _layer(self, l, x, rin, rout, ends):
        """x: rows [rin[0], rin[1]) of layer l's input -> rows [rout[0], rout[1]) of its output; ends (B) per-stream last frame + 1 in `finish`, else None"""
        sd, c, st, r = self.sd, self.cfg, self.layers[l], self.r
        pre = f"wav2vec2.encoder.layers.{l}."
        (p, a), (o0, o1) = rin, rout
        B, d = x.shape[0], c["hidden_size"]
        ln = lambda t, n: R.layer_norm(t, sd[pre + n + ".weight"], sd[pre + n + ".bias"], 1e-5)
        if a > p:
            if c.get("use_macaron_ff", True):
                x = x + 0.5 * R.ffn(sd, pre + "ff1.1.", ln(x, "ff1.0"))
            g = self._attention(st, pre + "self_attn.", ln(x, "self_attn_layer_norm"), p, a)
            lo = self._cgmlp(st, pre + "cgMLP.", ln(x, "cgMLP_layer_norm"))
            cat = torch.cat([g, lo], dim=-1)
        else:
            cat = torch.zeros(B, 0, 2 * d)
        full = torch.cat([st["cat"], cat], 1)                       # rows [p - 2r, a)
        pend = torch.cat([st["pend"], x], 1)                        # rows [o0, a)
        st["cat"] = full[:, full.shape[1] - 2 * r:]
        st["pend"] = pend[:, o1 - o0:]
        if o1 == o0:
            return torch.zeros(B, 0, d)
        base = p - 2 * r
        if ends is not None:                                        # flush: rows at or beyond a stream's end count as zero, r of them follow the last
            t = torch.arange(base, a)[None, :, None]
            full = torch.cat([full * (t < ends[:, None, None]), torch.zeros(B, r, 2 * d)], 1)
        win = full[:, o0 - r - base: o1 + r - base]
        w = sd[pre + "depthwise_conv_fusion.weight"]
        m2 = win[:, r: r + o1 - o0] + F.conv1d(win.transpose(1, 2), w, sd[pre + "depthwise_conv_fusion.bias"], groups=w.shape[0]).transpose(1, 2)
        y = pend[:, : o1 - o0] + F.linear(m2, sd[pre + "merge_proj.weight"], sd[pre + "merge_proj.bias"])
        if c.get("use_macaron_ff", True):
            y = y + 0.5 * R.ffn(sd, pre + "ff2.1.", ln(y, "ff2.0"))
        return ln(y, "final_layer_norm")

    def step(self, feats, finish=False, lengths=None):
        """feats (B, 4*C, F) (zero-padded in `finish`, `lengths` (B) valid frames) -> (logits (B, n_out, V+1), n_valid (B): rows of each stream that are final frames)"""
        assert not self.done
        B, C = self.B, self.C
        assert feats.shape[0] == B and feats.shape[1] == 4 * C
        n_prev = self.n_feat
        if finish:
            lengths = torch.full((B,), 4 * C, dtype=torch.long) if lengths is None else torch.as_tensor(lengths).long()
            totals = n_prev + lengths
            ends = (((totals + 1) // 2) + 1) // 2
            n_now = n_prev + int(lengths.max())
            self.done = True
        else:
            ends, n_now = None, n_prev + 4 * C
        rows = plan(n_now, C, self.L, self.r, finish, n_prev=n_prev)
        self.n_feat = n_now
        x = self._front(feats)[:, : rows[0][1] - rows[0][0]]
        for l in range(self.L):
            x = self._layer(l, x, rows[l], rows[l + 1], ends)
        x = R.layer_norm(x, self.sd["wav2vec2.encoder.layer_norm.weight"], self.sd["wav2vec2.encoder.layer_norm.bias"], self.cfg.get("layer_norm_eps", 1e-5))
        logits = R.ctc_head(self.sd, x)
        n_valid = torch.full((B,), x.shape[1], dtype=torch.long) if ends is None else ends - rows[self.L][0]
        return logits, n_valid


def stream_utterances(sd, cfg, feats, lengths, C, max_frames=None):
    """run utterances (B, T, F) with `lengths` (B) valid frames as one stream batch: whole chunks of 4*C frames while every stream still has one, then `finish`
    -> list of (out_frames(n_b), V+1) logits per stream, and the per-call (n_out, rows) record"""
    B, T = feats.shape[:2]
    lengths = [int(v) for v in lengths]
    st = RefStream(sd, cfg, B, C, max_frames or (T + 3) // 4 + 1)
    outs, rec = [[] for _ in range(B)], []
    pos = 0
    while min(lengths) - pos > 4 * C:
        lg, nv = st.step(feats[:, pos: pos + 4 * C])
        pos += 4 * C
        rec.append(lg.shape[1])
        for b in range(B):
            outs[b].append(lg[b, : int(nv[b])])
    tail = torch.zeros(B, 4 * C, feats.shape[2], dtype=feats.dtype)
    tl = [min(n - pos, 4 * C) for n in lengths]
    for b in range(B):
        tail[b, : tl[b]] = feats[b, pos: pos + tl[b]]
    lg, nv = st.step(tail, finish=True, lengths=tl)
    rec.append(lg.shape[1])
    for b in range(B):
        outs[b].append(lg[b, : int(nv[b])])
    return [torch.cat(o, 0) for o in outs], rec
