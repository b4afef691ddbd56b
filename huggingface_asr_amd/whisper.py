"""Whisper-style encoder and greedy decoding on the HIP kernels (BASELINE.json config 4).

The reference uses HuggingFace's Whisper classes as they are (`src/utilities/model_utils.py:183`,
`src/trainers/train_enc_dec_asr.py:82-83`, `configs/default_data_preprocessing_whisper.json`), so the drop-in unit here is an
engine that takes a `WhisperEncoder` state dict and reproduces `WhisperEncoder.forward` / `WhisperFeatureExtractor`:
Conv1d(80->d,k3)+GELU and Conv1d(d->d,k3,s2)+GELU as implicit GEMMs over a channels-last layout, + learned positions,
pre-LN layers (fused QKV GEMM with a zero bias block for k_proj, LDS-staged attention hd=64, out-proj / FFN GEMMs with the
residual fused), final LayerNorm.

Training: the encoder's forward / backward (`WhisperEncoderEngine.forward_train` / `backward`) and, opt-in through `install_whisper(decoder=True, fused_loss=True)`, the
decoder's teacher-forced forward / backward (`WhisperDecoderEngine.forward_train` / `backward`) and the loss out of the tied head's GEMM (`TiedHeadCE`)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .decoder import GPT2DecoderEngine
from .packing import _whisper_as_gpt2, _whisper_dec_map, mapped_fp32, packed, suppression_vectors, whisper_decoder_specs

BF16 = torch.bfloat16


class WhisperFrontend:
    """log-mel on device: (B, N) fp32 waveforms -> (B, 80, 3000) fp32 `input_features` (+ channels-last bf16 for conv1)."""

    def __init__(self, num_mel=80, n_samples=480000, sr=16000):
        self.num_mel, self.n_samples = num_mel, n_samples
        n = np.arange(400)
        self.window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / 400)                 # periodic hann
        self.twiddle = np.stack([np.cos(2 * np.pi * n / 400), np.sin(2 * np.pi * n / 400)], 1)
        self.filters = self._slaney(num_mel, sr)
        self._dev = {}

    @staticmethod
    def _slaney(num_mel, sr, fmin=0.0, fmax=8000.0):
        def hz2mel(f):
            f = np.asarray(f, dtype=np.float64)
            return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-30) / 1000.0) * (27.0 / np.log(6.4)), 3.0 * f / 200.0)

        def mel2hz(m):
            m = np.asarray(m, dtype=np.float64)
            return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), 200.0 * m / 3.0)
        ff = mel2hz(np.linspace(hz2mel(fmin), hz2mel(fmax), num_mel + 2))
        fft = np.linspace(0, sr // 2, 201)
        diff = np.diff(ff)
        sl = ff[None, :] - fft[:, None]
        fb = np.maximum(0.0, np.minimum(-sl[:, :-2] / diff[:-1], sl[:, 2:] / diff[1:]))
        return fb * (2.0 / (ff[2: num_mel + 2] - ff[:num_mel]))[None, :]

    def _tables(self, device):
        k = str(device)
        if k not in self._dev:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._dev[k] = (t(self.window), t(self.twiddle), t(self.filters.T.copy()))
        return self._dev[k]

    def __call__(self, wave: torch.Tensor, num_samples=None, want_features=True):
        if not wave.is_cuda:
            raise RuntimeError("WhisperFrontend needs device tensors (no CPU fallback)")
        B, N = wave.shape
        win, tw, mel = self._tables(wave.device)
        frames = self.n_samples // 160
        ns = num_samples.to(torch.int32) if num_samples is not None else torch.full((B,), min(N, self.n_samples), dtype=torch.int32, device=wave.device)
        scratch = torch.empty(B * frames * self.num_mel + B, dtype=torch.float32, device=wave.device)       # log-mel before the clamp + the per-clip maxima
        feats = torch.empty((B, self.num_mel, frames), dtype=torch.float32, device=wave.device) if want_features else None
        cl = torch.empty((B, frames, self.num_mel), dtype=BF16, device=wave.device)
        rc = _lib.lib().mi_whisper_logmel(wave.data_ptr(), wave.stride(0), ns.data_ptr(), self.n_samples, win.data_ptr(), tw.data_ptr(),
                                          mel.data_ptr(), self.num_mel, B, scratch.data_ptr(), 0 if feats is None else feats.data_ptr(),
                                          cl.data_ptr(), torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mi_whisper_logmel")
        return feats, cl


class WhisperEncoderEngine:
    def __init__(self, cfg: dict, device="cuda:0"):
        self.cfg = dict(cfg)
        self.device = torch.device(device)
        if cfg["d_model"] // cfg["encoder_attention_heads"] not in (64, 128):
            raise NotImplementedError("head size must be 64 or 128")
        self.w = None
        self.tail_split = True          # GEMM dispatch: give an under-filled last round of 256 x 256 tiles to the 128 x 128 kernel (gemm_glds.hip); set False when several batches are in flight on streams

    def load_state_dict(self, sd: dict, prefix: str = ""):
        dev, c = self.device, self.cfg
        d = c["d_model"]
        f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
        bf = lambda t: t.detach().to(dev, torch.float32).to(BF16).contiguous()
        g = lambda n: sd[prefix + n]
        w = dict(
            c1w=bf(g("conv1.weight").permute(0, 2, 1).reshape(d, -1)), c1b=f32(g("conv1.bias")),          # (d, k*mel): k-major, channel-minor
            c2w=bf(g("conv2.weight").permute(0, 2, 1).reshape(d, -1)), c2b=f32(g("conv2.bias")),
            pos=f32(g("embed_positions.weight")), lnf=(f32(g("layer_norm.weight")), f32(g("layer_norm.bias"))), layers=[])
        for l in range(c["encoder_layers"]):
            p = f"{prefix}layers.{l}."
            wqkv = bf(torch.cat([sd[p + f"self_attn.{n}_proj.weight"].detach().to(dev) for n in "qkv"], 0))
            bqkv = f32(torch.cat([sd[p + "self_attn.q_proj.bias"].detach().to(dev), torch.zeros(d, device=dev),
                                  sd[p + "self_attn.v_proj.bias"].detach().to(dev)], 0))                   # k_proj has no bias
            w["layers"].append(dict(
                ln1=(f32(sd[p + "self_attn_layer_norm.weight"]), f32(sd[p + "self_attn_layer_norm.bias"])), wqkv=wqkv, bqkv=bqkv,
                wo=bf(sd[p + "self_attn.out_proj.weight"]), bo=f32(sd[p + "self_attn.out_proj.bias"]),
                ln2=(f32(sd[p + "final_layer_norm.weight"]), f32(sd[p + "final_layer_norm.bias"])),
                w1=bf(sd[p + "fc1.weight"]), b1=f32(sd[p + "fc1.bias"]), w2=bf(sd[p + "fc2.weight"]), b2=f32(sd[p + "fc2.bias"])))
        self.w = w

    def forward(self, input_features: torch.Tensor | None = None, features_cl: torch.Tensor | None = None) -> torch.Tensor:
        """input_features (B, mel, T) fp32 (HF layout) or features_cl (B, T, mel) bf16 -> last_hidden_state (B, T/2, d) fp32."""
        c, w, dev = self.cfg, self.w, self.device
        L = _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        d, H = c["d_model"], c["encoder_attention_heads"]
        if features_cl is None:
            if not input_features.is_cuda:
                raise RuntimeError("WhisperEncoderEngine needs device tensors (no CPU fallback)")
            B, mel, T = input_features.shape
            x32 = input_features.to(torch.float32).contiguous()
            features_cl = torch.empty((B, T, mel), dtype=BF16, device=dev)
            _lib.check(L.mi_transpose_cast_bct_btc(x32.data_ptr(), features_cl.data_ptr(), B, mel, T, st), "mi_transpose_cast_bct_btc")
        B, T, mel = features_cl.shape
        P = w["pos"].shape[0]
        if T != 2 * P:
            raise ValueError(f"Whisper expects the mel input features to be of length {2 * P}, but found {T}")
        h1 = ops.conv2d_cl(features_cl.view(B, T, 1, mel), w["c1w"], w["c1b"], K=(3, 1), stride=1, pad=(1, 0))
        h2 = ops.conv2d_cl(h1, w["c2w"], w["c2b"], K=(3, 1), stride=2, pad=(1, 0))
        T2 = h2.shape[1]
        M = B * T2
        x = torch.empty((M, d), dtype=torch.float32, device=dev)
        _lib.check(L.mi_add_positions(h2.data_ptr(), w["pos"].data_ptr(), x.data_ptr(), M, T2, d, st), "mi_add_positions")
        a = torch.empty((M, d), dtype=BF16, device=dev)
        gv = 0 if self.tail_split else 48
        for lw in w["layers"]:
            ops.layernorm_chain(x, lna=lw["ln1"], outa=a)
            qkv = ops.gemm(a, lw["wqkv"], lw["bqkv"], variant=gv)
            ctx = ops.attention_qkv(qkv, B, T2, H)
            ops.gemm(ctx, lw["wo"], lw["bo"], out=x, resid=x, alpha=1.0, variant=gv)
            ops.layernorm_chain(x, lna=lw["ln2"], outa=a)
            m = ops.gemm(a, lw["w1"], lw["b1"], act="gelu", variant=gv)
            ops.gemm(m, lw["w2"], lw["b2"], out=x, resid=x, alpha=1.0, variant=gv)
        out = torch.empty((M, d), dtype=torch.float32, device=dev)
        ops.layernorm_chain(x, lna=w["lnf"], outa32=out)
        return out.view(B, T2, d)

    # ---------------------------------------------------------------------------------------------------------------------------------------------
    # Training: forward_train keeps what the backward reads; backward runs LayerNorm / GEMM dgrad + wgrad / GELU' / im2col + col2im and the attention
    # backward (ops_train.attn_bwd_fused: no (H, B, T, T) tensor) on the HIP kernels.  Dropout is not covered (the binding hands such calls to transformers).
    fused_attn_bwd = False      # True: ops_train.attn_bwd_fused (no (H, B, T, T) tensor); False: attn_bwd_probs + bgemm, which measured as fast at T' = 1500 (DESIGN "Whisper encoder training")

    def _wT(self, key, wm):
        """the transposed copy of a bf16 weight (N, K) -> (K, pad64(N)) for the dX GEMMs, made once per weight version (the engine is rebuilt when a parameter changes)"""
        from . import ops_train as OT
        cache = self.__dict__.setdefault("_wT_cache", {})
        if key not in cache:
            cache[key] = OT.transpose(wm)
        return cache[key]

    def forward_train(self, input_features: torch.Tensor, skip=None) -> tuple[torch.Tensor, dict]:
        """-> (last_hidden_state (B, T/2, d) fp32, saved).  skip: per layer, True = LayerDrop skipped it."""
        from . import ops_train as OT
        c, w, dev = self.cfg, self.w, self.device
        L = _lib.lib()
        st = torch.cuda.current_stream().cuda_stream
        d, H = c["d_model"], c["encoder_attention_heads"]
        B, mel, T = input_features.shape
        P = w["pos"].shape[0]
        if T != 2 * P:
            raise ValueError(f"Whisper expects the mel input features to be of length {2 * P}, but found {T}")
        x32 = input_features.detach().to(torch.float32).contiguous()
        fcl = torch.empty((B, T, mel), dtype=BF16, device=dev)
        _lib.check(L.mi_transpose_cast_bct_btc(x32.data_ptr(), fcl.data_ptr(), B, mel, T, st), "mi_transpose_cast_bct_btc")
        h1p = ops.conv2d_cl(fcl.view(B, T, 1, mel), w["c1w"], w["c1b"], K=(3, 1), stride=1, pad=(1, 0), act="none")
        h1 = OT.act_fwd(h1p.view(B * T, d)).view(B, T, 1, d)
        h2p = ops.conv2d_cl(h1, w["c2w"], w["c2b"], K=(3, 1), stride=2, pad=(1, 0), act="none")
        T2 = h2p.shape[1]
        M = B * T2
        h2 = OT.act_fwd(h2p.view(M, d))
        x = torch.empty((M, d), dtype=torch.float32, device=dev)
        _lib.check(L.mi_add_positions(h2.data_ptr(), w["pos"].data_ptr(), x.data_ptr(), M, T2, d, st), "mi_add_positions")
        skip = skip or [False] * len(w["layers"])
        layers = []
        for lw, sk in zip(w["layers"], skip):
            if sk:
                layers.append(None)
                continue
            S = dict(x_in=x)
            a = torch.empty((M, d), dtype=BF16, device=dev)
            ops.layernorm_chain(x, lna=lw["ln1"], outa=a)
            S["a1"] = a
            S["qkv"] = qkv = ops.gemm(a, lw["wqkv"], lw["bqkv"])
            S["lse"] = lse = torch.empty((B, H, T2), dtype=torch.float32, device=dev)
            S["ctx"] = ctx = ops.attention_qkv(qkv, B, T2, H, lse=lse)
            xm = ops.gemm(ctx, lw["wo"], lw["bo"], out=torch.empty((M, d), dtype=torch.float32, device=dev), resid=x, alpha=1.0)
            S["x_mid"] = xm
            a2 = torch.empty((M, d), dtype=BF16, device=dev)
            ops.layernorm_chain(xm, lna=lw["ln2"], outa=a2)
            S["a2"] = a2
            S["m_pre"], S["m"] = OT.gemm_act_fwd(a2, lw["w1"], lw["b1"], "gelu")
            x = ops.gemm(S["m"], lw["w2"], lw["b2"], out=torch.empty((M, d), dtype=torch.float32, device=dev), resid=xm, alpha=1.0)
            layers.append(S)
        out = torch.empty((M, d), dtype=torch.float32, device=dev)
        ops.layernorm_chain(x, lna=w["lnf"], outa32=out)
        saved = dict(B=B, T=T, T2=T2, mel=mel, fcl=fcl, h1p=h1p, h1=h1, h2p=h2p, x_last=x, layers=layers)
        return out.view(B, T2, d), saved

    def backward(self, saved: dict, d_last_hidden: torch.Tensor, want) -> dict:
        """Gradients keyed by the HF `WhisperEncoder` parameter names (`want(name)` -> bool; None for what is not wanted), fp32 in the parameters' shapes, plus
        "input_features" when want("input_features")."""
        from . import ops_train as OT
        c, w, dev = self.cfg, self.w, self.device
        d, H = c["d_model"], c["encoder_attention_heads"]
        B, T, T2, mel = saved["B"], saved["T"], saved["T2"], saved["mel"]
        M = B * T2
        f32 = torch.float32
        z = lambda *shape: torch.zeros(shape, dtype=f32, device=dev)
        G = {}

        def slot(name, *shape):
            if want(name):
                G[name] = z(*shape)
                return G[name]
            return None
        dy = d_last_hidden.detach().reshape(M, d).to(f32).contiguous()
        dx = torch.empty((M, d), dtype=f32, device=dev)
        OT.layernorm_bwd(saved["x_last"], w["lnf"][0], dy, dx, accumulate=False, dgamma=slot("layer_norm.weight", d), dbeta=slot("layer_norm.bias", d))
        for l in reversed(range(len(w["layers"]))):
            S, lw = saved["layers"][l], w["layers"][l]
            if S is None:                                   # LayerDrop skipped it: identity, no gradient
                continue
            p = f"layers.{l}."
            ffn = lw["w1"].shape[0]
            # FFN: x = x_mid + fc2(gelu(fc1(LN2(x_mid))))
            dyb = OT.add_cast(dx)
            dw2, db2 = slot(p + "fc2.weight", d, ffn), slot(p + "fc2.bias", d)
            if dw2 is not None or db2 is not None:
                OT.linear_bwd(dyb, S["m"], None, dw=dw2, db=db2, need_dx=False)
            dmp = OT.gemm_act_bwd(dyb, self._wT((l, "w2"), lw["w2"]), S["m_pre"], "gelu")
            dw1, db1 = slot(p + "fc1.weight", ffn, d), slot(p + "fc1.bias", ffn)
            da2 = OT.linear_bwd(dmp, S["a2"], self._wT((l, "w1"), lw["w1"]), dw=dw1, db=db1)
            OT.layernorm_bwd(S["x_mid"], lw["ln2"][0], da2, dx, accumulate=True, dgamma=slot(p + "final_layer_norm.weight", d), dbeta=slot(p + "final_layer_norm.bias", d))
            # attention: x_mid = x_in + out_proj(attn(LN1(x_in)))
            dyb = OT.add_cast(dx)
            dctx = OT.linear_bwd(dyb, S["ctx"], self._wT((l, "wo"), lw["wo"]), dw=slot(p + "self_attn.out_proj.weight", d, d), db=slot(p + "self_attn.out_proj.bias", d))
            dqkv = torch.empty((M, 3 * d), dtype=BF16, device=dev)
            (OT.attn_bwd_fused if self.fused_attn_bwd else OT.attn_bwd_materialized)(S["qkv"], B, T2, H, S["ctx"], dctx, S["lse"], dqkv)
            names = [p + f"self_attn.{n}_proj.weight" for n in "qkv"]
            dwqkv = z(3 * d, d) if any(want(n) for n in names) else None
            dbqkv = z(3 * d) if (want(p + "self_attn.q_proj.bias") or want(p + "self_attn.v_proj.bias")) else None
            da1 = OT.linear_bwd(dqkv, S["a1"], self._wT((l, "wqkv"), lw["wqkv"]), dw=dwqkv, db=dbqkv)
            for i, n in enumerate(names):
                if dwqkv is not None and want(n):
                    G[n] = dwqkv[i * d:(i + 1) * d]                 # row views of the packed [Wq; Wk; Wv] gradient
            for i, n in ((0, "q"), (2, "v")):                       # k_proj has no bias
                if dbqkv is not None and want(p + f"self_attn.{n}_proj.bias"):
                    G[p + f"self_attn.{n}_proj.bias"] = dbqkv[i * d:(i + 1) * d]
            OT.layernorm_bwd(S["x_in"], lw["ln1"][0], da1, dx, accumulate=True, dgamma=slot(p + "self_attn_layer_norm.weight", d),
                             dbeta=slot(p + "self_attn_layer_norm.bias", d))
        # positions add: x0 = gelu(conv2) + pos
        if want("embed_positions.weight"):
            G["embed_positions.weight"] = z(T2 * d)
            OT.colsum_(G["embed_positions.weight"], dx.view(B, T2 * d))             # sum over the batch, rows in order
            G["embed_positions.weight"] = G["embed_positions.weight"].view(T2, d)
        dxb = OT.add_cast(dx)
        need_conv1 = want("conv1.weight") or want("conv1.bias") or want("input_features")
        # conv2 (K 3, stride 2, pad 1) + GELU
        dh2p = OT.act_bwd(dxb, saved["h2p"].view(M, d))
        h1 = saved["h1"]
        dwc2, dbc2 = slot("conv2.weight", d, 3 * d), slot("conv2.bias", d)
        if dwc2 is not None or dbc2 is not None:
            OT.gemm_tn_(dwc2 if dwc2 is not None else z(d, 3 * d), dh2p, OT.im2col_geo(h1, (3, 1), (2, 1), (1, 0), T2, 1), db=dbc2)
        if need_conv1:
            dcol = ops.gemm(dh2p, self._wT("c2w", w["c2w"])[:, :d])
            dh1 = OT.col2im(dcol, (B, T, 1, d), (3, 1), (2, 1), (1, 0), T2, 1)
            dh1p = OT.act_bwd(dh1.view(B * T, d), saved["h1p"].view(B * T, d))
            dwc1, dbc1 = slot("conv1.weight", d, 3 * mel), slot("conv1.bias", d)
            if dwc1 is not None or dbc1 is not None:
                OT.gemm_tn_(dwc1 if dwc1 is not None else z(d, 3 * mel), dh1p, OT.im2col_geo(saved["fcl"].view(B, T, 1, mel), (3, 1), (1, 1), (1, 0), T, 1), db=dbc1)
            if want("input_features"):
                dcol1 = ops.gemm(dh1p, self._wT("c1w", w["c1w"])[:, :d])
                dfe = OT.col2im(dcol1, (B, T, 1, mel), (3, 1), (1, 1), (1, 0), T, 1)
                G["input_features"] = dfe.view(B, T, mel).permute(0, 2, 1).to(f32)
        for n in ("conv1.weight", "conv2.weight"):                  # (d, k*Cin) k-major -> HF (d, Cin, k)
            if G.get(n) is not None:
                G[n] = G[n].view(d, 3, -1).permute(0, 2, 1)
        return G


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Decoding.  A Whisper decoder block is the GPT-2 cross-attention block of decoder.py (pre-LN: self-attention over the KV cache, cross-attention over cached encoder
# K/V, MLP) with separate q / k / v matrices (k_proj without a bias), erf-GELU, learned positions and the token embedding as the head — so it runs on the same C step
# (`mi_decoder_step`, csrc/decoder_step.hip) from a table packed by `packing.whisper_decoder_specs`.
class WhisperDecoderEngine(GPT2DecoderEngine):
    """transformers' `WhisperDecoder.forward` with a KV cache + the tied `proj_out`, one C call per step.  cfg: the decoder fields of a `WhisperConfig`
    (d_model, decoder_layers, decoder_attention_heads, decoder_ffn_dim, vocab_size, max_target_positions, activation_function, scale_embedding)."""

    # (rows, d_model) at which the streaming form of the step (`mi_gpt2_config.step_form = 2`, csrc/linear_rows.hip) measured faster than the launch-per-op form by more
    # than the run-to-run spread of the same call (tools/whisper_decode_bench.py, DESIGN "Whisper decoding"); every other shape runs form 1
    STREAMING_AT = ((1, 768), (16, 768), (16, 1024))          # measured and lost: (64, 768); every other shape: not measured

    def __init__(self, cfg: dict, device="cuda:0"):
        d, H = cfg["d_model"], cfg["decoder_attention_heads"]
        if d % H or d // H != 64:
            raise NotImplementedError("the HIP Whisper decoder supports head size 64 (every released checkpoint)")
        if cfg.get("decoder_ffn_dim", 4 * d) != 4 * d:
            raise NotImplementedError("the HIP Whisper decoder needs decoder_ffn_dim == 4 * d_model")
        if cfg.get("activation_function", "gelu") != "gelu":
            raise NotImplementedError("Whisper decoder activation other than gelu")
        self.cfg = dict(cfg, **_whisper_as_gpt2(cfg))        # + the GPT-2 names of the same numbers, which the inherited cache / position code reads
        self.device = torch.device(device)
        self.step_form = None           # None: by STREAMING_AT; 1 / 2 force a form (tests, the bench tool)
        self.w = None

    def load_state_dict(self, sd: dict, prefix: str = ""):
        """transformers' `WhisperDecoder` names (embed_tokens, embed_positions, layers.N.{self_attn,encoder_attn}.*, layers.N.fc1 / fc2, layer_norm) -> the step's table"""
        c, dev = self.cfg, self.device
        d, L = c["d_model"], c["decoder_layers"]
        m = _whisper_dec_map(c, prefix)
        P = {s.name: (t.to(BF16) if s.mat and s.name != "wte" else t).contiguous()          # wte stays fp32: the embedding gather reads it
             for s, t in packed(whisper_decoder_specs(c), m, mapped_fp32(m, sd, dev))}
        w = dict(wte=P["wte"], scale=float(d) ** 0.5 if c.get("scale_embedding", False) else 1.0, pos=P["wpe"], lnf=(P["lnf_g"], P["lnf_b"]), heads=[],
                 lm_head=P["wte"].to(BF16))                                                   # tied: the token embedding's bf16 image is the head
        w["layers"] = [dict({n: P[f"h{l}.{n}"] for n in ("wqkv", "bqkv", "wo", "bo", "wq", "bq", "wkv", "bkv", "wco", "bco", "wfc", "bfc", "wpr", "bpr")},
                            **{n: (P[f"h{l}.{n}_g"], P[f"h{l}.{n}_b"]) for n in ("ln1", "lnc", "ln2")}) for l in range(L)]
        self.w = w
        ptrs = [w["wte"], w["pos"], w["lnf"][0], w["lnf"][1], w["lm_head"]]
        for lw in w["layers"]:
            ptrs += [lw["ln1"][0], lw["ln1"][1], lw["wqkv"], lw["bqkv"], lw["wo"], lw["bo"], lw["lnc"][0], lw["lnc"][1], lw["wq"], lw["bq"],
                     lw["wco"], lw["bco"], lw["ln2"][0], lw["ln2"][1], lw["wfc"], lw["bfc"], lw["wpr"], lw["bpr"]]
        self.__dict__.pop("_wT_cache", None)                  # the transposed copies of the training backward belong to the previous weights
        self._wtable = (C.c_void_p * len(ptrs))(*[t.data_ptr() for t in ptrs])
        self._gcfg = _lib.Gpt2Config(d=d, H=c["decoder_attention_heads"], L=L, V=c["vocab_size"], eps=1e-5, step_form=1, act=1)
        self._step_ws = None

    def ensure_positions(self, n: int):
        have = self.cfg["max_target_positions"]
        if n > have:
            raise ValueError(f"decoding needs {n} positions but the learned position table (embed_positions) has max_target_positions = {have} rows")

    def form_for(self, rows: int) -> int:
        if self.step_form is not None:
            return self.step_form
        return 2 if (rows, self.cfg["d_model"]) in self.STREAMING_AT else 1

    def step(self, ids_new: torch.Tensor, cache, kvs, T_enc: int, head_bias=None):
        """ids_new (B, U) -> fp32 logits (B, V) of the last new position (+ head_bias (V) fp32, 0 / -inf); appends to the KV cache.  One C call (mi_decoder_step)."""
        ids_new = ids_new.contiguous()
        B, U = ids_new.shape
        past, Lmax = cache["past"], cache["Lmax"]
        self.ensure_positions(past + U)
        if past + U > Lmax:
            raise ValueError(f"the KV cache holds {Lmax} positions, the step needs {past + U}")
        L_ = _lib.lib()
        self._gcfg.step_form = self.form_for(B)
        nbytes = L_.mi_gpt2_step_workspace_bytes(C.byref(self._gcfg), B, U)
        if self._step_ws is None or self._step_ws.numel() < nbytes:
            self._step_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if cache.get("kv_id") != id(kvs):
            cache["tkv"] = (C.c_void_p * len(kvs))(*[t.data_ptr() for t in kvs])
            cache["kv_id"] = id(kvs)
        V = self._gcfg.V
        Vp = (V + 7) // 8 * 8
        buf = torch.empty((B, Vp), device=self.device, dtype=torch.float32)
        _lib.check(L_.mi_decoder_step(C.byref(self._gcfg), self._wtable, ids_new.data_ptr(), B, U, past, Lmax, cache["tk"], cache["tv"], cache["tkv"], T_enc, None,
                                      float(self.w["scale"]), head_bias.data_ptr() if head_bias is not None else None, self._step_ws.data_ptr(), self._step_ws.numel(),
                                      buf.data_ptr(), Vp, torch.cuda.current_stream().cuda_stream), "mi_decoder_step")
        cache["past"] = past + U
        return buf[:, :V]

    def forward(self, *a, **k):
        raise NotImplementedError("WhisperDecoderEngine decodes step by step (step / greedy_decode); the teacher-forced training forward stays transformers'")

    step_py = forward

    # ---------------------------------------------------------------------------------------------------------------------------------------------
    # Training: the teacher-forced pass over all U positions at once and its analytic backward — the block of `train_aed.JointAEDTrainer._layer_fwd` / `_layer_bwd`
    # (causal self-attention, cross-attention over the encoder frames, MLP) with erf-GELU in the FFN-in GEMM's epilogue and transformers' parameter names, shaped like
    # `WhisperEncoderEngine.forward_train` / `backward`.  Dropout is not covered (the binding hands such calls to transformers).
    _wT = WhisperEncoderEngine._wT

    def forward_train(self, input_ids: torch.Tensor, encoder_hidden: torch.Tensor, skip=None) -> tuple[torch.Tensor, dict]:
        """input_ids (B, U) int64, encoder_hidden (B, T2, d) -> (last_hidden_state (B, U, d) fp32, saved).  skip: per layer, True = LayerDrop skipped it."""
        from . import ops_train as OT
        c, w, dev = self.cfg, self.w, self.device
        d, H = c["d_model"], c["decoder_attention_heads"]
        if not input_ids.is_cuda or not encoder_hidden.is_cuda:
            raise RuntimeError("WhisperDecoderEngine needs device tensors (no CPU fallback)")
        ids = input_ids.detach().to(torch.long).contiguous()
        B, U = ids.shape
        T2 = encoder_hidden.shape[1]
        self.ensure_positions(U)
        M, Me = B * U, B * T2
        f32 = torch.float32
        e16 = lambda *sh: torch.empty(sh, dtype=BF16, device=dev)
        e32 = lambda *sh: torch.empty(sh, dtype=f32, device=dev)
        enc_bf = ops.cast_bf16(encoder_hidden.detach().reshape(Me, d).to(f32).contiguous())
        x = ops.embed_tokens(ids, w["wte"], w["pos"], scale=w["scale"])
        skip = skip or [False] * len(w["layers"])
        layers = []
        for lw, sk in zip(w["layers"], skip):
            if sk:
                layers.append(None)
                continue
            S = dict(x=x)
            S["a1"] = a1 = e16(M, d)
            ops.layernorm_chain(x, lna=lw["ln1"], outa=a1)
            S["qkv"] = qkv = ops.gemm(a1, lw["wqkv"], lw["bqkv"])
            S["ctx1"], S["lse1"] = OT.attention_x_lse(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], B, U, U, H, causal=True)
            S["x1"] = x1 = ops.gemm(S["ctx1"], lw["wo"], lw["bo"], out=e32(M, d), resid=x, alpha=1.0)
            S["a2"] = a2 = e16(M, d)
            ops.layernorm_chain(x1, lna=lw["lnc"], outa=a2)
            S["qq"] = qq = ops.gemm(a2, lw["wq"], lw["bq"])
            S["kv"] = kv = ops.gemm(enc_bf, lw["wkv"], lw["bkv"])
            S["ctx2"], S["lse2"] = OT.attention_x_lse(qq, kv[:, :d], kv[:, d:], B, U, T2, H)
            S["x2"] = x2 = ops.gemm(S["ctx2"], lw["wco"], lw["bco"], out=e32(M, d), resid=x1, alpha=1.0)
            S["a3"] = a3 = e16(M, d)
            ops.layernorm_chain(x2, lna=lw["ln2"], outa=a3)
            S["mp"], S["mm"] = OT.gemm_act_fwd(a3, lw["wfc"], lw["bfc"], "gelu")
            x = ops.gemm(S["mm"], lw["wpr"], lw["bpr"], out=e32(M, d), resid=x2, alpha=1.0)
            layers.append(S)
        out = e32(M, d)
        ops.layernorm_chain(x, lna=w["lnf"], outa32=out)
        saved = dict(B=B, U=U, T2=T2, ids=ids, enc_bf=enc_bf, x_last=x, layers=layers)
        return out.view(B, U, d), saved

    def backward(self, saved: dict, d_last_hidden: torch.Tensor, want) -> dict:
        """Gradients keyed by the HF `WhisperDecoder` parameter names (`want(name)` -> bool; absent for what is not wanted), fp32 in the parameters' shapes, plus
        "encoder_hidden_states" (B, T2, d) when want("encoder_hidden_states")."""
        from . import ops_train as OT
        from .train_aed import attention_bwd_fused
        c, w, dev = self.cfg, self.w, self.device
        d, H = c["d_model"], c["decoder_attention_heads"]
        B, U, T2 = saved["B"], saved["U"], saved["T2"]
        M, Me = B * U, B * T2
        f32 = torch.float32
        z = lambda *shape: torch.zeros(shape, dtype=f32, device=dev)
        e16 = lambda *sh: torch.empty(sh, dtype=BF16, device=dev)
        G = {}

        def slot(name, *shape):
            if want(name):
                G[name] = z(*shape)
                return G[name]
            return None

        def packed_rows(names, rows, cols=None):
            """one zeroed buffer for parameters the engine keeps stacked ([Wq; Wk; Wv], [Wk; Wv] and their biases; names[i] None: a block without a parameter) when any
            of them is wanted, and the wanted ones as row views of it"""
            if not any(n is not None and want(n) for n in names):
                return None
            buf = z(rows * len(names), cols) if cols else z(rows * len(names))
            for i, n in enumerate(names):
                if n is not None and want(n):
                    G[n] = buf[i * rows:(i + 1) * rows]
            return buf
        enc_bf = saved["enc_bf"]
        want_enc = want("encoder_hidden_states")
        denc = z(Me, d) if want_enc else None               # every layer's cross-attention adds its share, from the last layer down
        dy = d_last_hidden.detach().reshape(M, d).to(f32).contiguous()
        dx = torch.empty((M, d), dtype=f32, device=dev)
        OT.layernorm_bwd(saved["x_last"], w["lnf"][0], dy, dx, accumulate=False, dgamma=slot("layer_norm.weight", d), dbeta=slot("layer_norm.bias", d))
        for l in reversed(range(len(w["layers"]))):
            S, lw = saved["layers"][l], w["layers"][l]
            if S is None:                                   # LayerDrop skipped it: identity, no gradient
                continue
            p = f"layers.{l}."
            sa, ca = p + "self_attn.", p + "encoder_attn."
            ffn = lw["wfc"].shape[0]
            # FFN: x3 = x2 + fc2(gelu(fc1(LN(x2))))
            dyb = OT.add_cast(dx)
            dw2, db2 = slot(p + "fc2.weight", d, ffn), slot(p + "fc2.bias", d)
            if dw2 is not None or db2 is not None:
                OT.linear_bwd(dyb, S["mm"], None, dw=dw2, db=db2, need_dx=False)
            dmp = OT.gemm_act_bwd(dyb, self._wT((l, "wpr"), lw["wpr"]), S["mp"], "gelu")
            da3 = OT.linear_bwd(dmp, S["a3"], self._wT((l, "wfc"), lw["wfc"]), dw=slot(p + "fc1.weight", ffn, d), db=slot(p + "fc1.bias", ffn))
            OT.layernorm_bwd(S["x2"], lw["ln2"][0], da3, dx, accumulate=True, dgamma=slot(p + "final_layer_norm.weight", d), dbeta=slot(p + "final_layer_norm.bias", d))
            # cross-attention: x2 = x1 + out_proj(attn(q(LN(x1)), k(enc), v(enc)))
            dyb = OT.add_cast(dx)
            dctx2 = OT.linear_bwd(dyb, S["ctx2"], self._wT((l, "wco"), lw["wco"]), dw=slot(ca + "out_proj.weight", d, d), db=slot(ca + "out_proj.bias", d))
            dqq, dkv = e16(M, d), e16(Me, 2 * d)
            kv = S["kv"]
            attention_bwd_fused(S["qq"], kv[:, :d], kv[:, d:], S["ctx2"], dctx2, S["lse2"], dqq, dkv[:, :d], dkv[:, d:], B, U, T2, H)
            da2 = OT.linear_bwd(dqq, S["a2"], self._wT((l, "wq"), lw["wq"]), dw=slot(ca + "q_proj.weight", d, d), db=slot(ca + "q_proj.bias", d))
            dwkv = packed_rows([ca + "k_proj.weight", ca + "v_proj.weight"], d, d)
            dbkv = packed_rows([None, ca + "v_proj.bias"], d)                      # k_proj has no bias
            if dwkv is not None or dbkv is not None:
                OT.linear_bwd(dkv, enc_bf, None, dw=dwkv, db=dbkv, need_dx=False)
            if want_enc:
                ops.gemm(dkv, self._wT((l, "wkv"), lw["wkv"])[:, :2 * d], out=denc, resid=denc, alpha=1.0)
            OT.layernorm_bwd(S["x1"], lw["lnc"][0], da2, dx, accumulate=True, dgamma=slot(p + "encoder_attn_layer_norm.weight", d),
                             dbeta=slot(p + "encoder_attn_layer_norm.bias", d))
            # causal self-attention: x1 = x + out_proj(attn(LN(x)))
            dyb = OT.add_cast(dx)
            dctx1 = OT.linear_bwd(dyb, S["ctx1"], self._wT((l, "wo"), lw["wo"]), dw=slot(sa + "out_proj.weight", d, d), db=slot(sa + "out_proj.bias", d))
            qkv = S["qkv"]
            dqkv = e16(M, 3 * d)
            attention_bwd_fused(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], S["ctx1"], dctx1, S["lse1"], dqkv[:, :d], dqkv[:, d:2 * d], dqkv[:, 2 * d:], B, U, U, H, causal=True)
            dwqkv = packed_rows([sa + f"{n}_proj.weight" for n in "qkv"], d, d)
            dbqkv = packed_rows([sa + "q_proj.bias", None, sa + "v_proj.bias"], d)
            da1 = OT.linear_bwd(dqkv, S["a1"], self._wT((l, "wqkv"), lw["wqkv"]), dw=dwqkv, db=dbqkv)
            OT.layernorm_bwd(S["x"], lw["ln1"][0], da1, dx, accumulate=True, dgamma=slot(p + "self_attn_layer_norm.weight", d), dbeta=slot(p + "self_attn_layer_norm.bias", d))
        # x0 = embed_tokens[ids] + embed_positions[0 .. U)
        V, P = w["wte"].shape[0], w["pos"].shape[0]
        dwte, dwpe = slot("embed_tokens.weight", V, d), slot("embed_positions.weight", P, d)
        if dwte is not None or dwpe is not None:
            OT.embed_tokens_bwd(saved["ids"], dx, dwte if dwte is not None else z(V, d), dwpe, scale=w["scale"])
        if want_enc:
            G["encoder_hidden_states"] = denc.view(B, T2, d)
        return G


def greedy_decode(enc_engine, dec_engine, input_features, prompt_ids, *, max_new_tokens, eos_token_id, pad_token_id, suppress_tokens=None, begin_suppress_tokens=None,
                  run_ahead=2, stats=None):
    """Greedy transcription with the loop on the device -> (B, P + n) LongTensor: per row the prompt, the generated tokens, the first EOS (kept), then pad_token_id —
    `GenerationMixin`'s greedy layout, trimmed to the longest row.  Per token: the decoder step with the suppression vector as the head's bias (the begin-suppress ids in
    the first generated token's only), `mi_row_argmax`, and one kernel that appends the token (pad for a finished row), hands it to the next step and sets the row's done
    flag at EOS, writing the flags into pinned memory.  The host only enqueues, at most `run_ahead` steps in front of the flags it has seen, and stops once every row is
    done; nothing is copied per token.  The prompt (B, P) is consumed by one step of P positions.  `stats` receives the number of steps enqueued."""
    if not input_features.is_cuda or not prompt_ids.is_cuda:
        raise RuntimeError("greedy_decode needs device tensors (no CPU fallback)")
    dev = dec_engine.device
    B, P = prompt_ids.shape
    V = dec_engine.cfg["vocab_size"]
    if max_new_tokens < 1:
        raise ValueError("max_new_tokens >= 1 required")
    dec_engine.ensure_positions(P + max_new_tokens)
    for name, t in (("eos_token_id", eos_token_id), ("pad_token_id", pad_token_id)):
        if not 0 <= int(t) < V:
            raise ValueError(f"{name} {t} outside the vocabulary [0, {V})")
    every, first = suppression_vectors(V, suppress_tokens, begin_suppress_tokens, dev)
    enc = enc_engine.forward(input_features=input_features)
    T2, d = enc.shape[1], enc.shape[2]
    kvs = dec_engine.cross_kv(ops.cast_bf16(enc.reshape(B * T2, d)))
    Lmax = P + max_new_tokens
    cache = dec_engine.init_cache(B, Lmax)
    ids = torch.full((B, Lmax), int(pad_token_id), dtype=torch.long, device=dev)
    ids[:, :P] = prompt_ids
    done = torch.zeros((B,), dtype=torch.int32, device=dev)
    done_host = torch.zeros((max_new_tokens, B), dtype=torch.int32).pin_memory()
    new_tok = prompt_ids.to(torch.long).contiguous()
    L_ = _lib.lib()
    main = torch.cuda.current_stream()
    flags, steps = [], 0
    while steps < max_new_tokens:
        if len(flags) >= run_ahead:                # bounded run-ahead: the flags of step (now - run_ahead) are in pinned memory once its event has fired
            flags[len(flags) - run_ahead].synchronize()
            if bool(done_host[steps - run_ahead].all()):
                break
        logits = dec_engine.step(new_tok, cache, kvs, T2, first if steps == 0 else every)
        best = ops.row_argmax(logits)
        new_tok = torch.empty((B, 1), dtype=torch.long, device=dev)
        _lib.check(L_.mi_greedy_advance(best.data_ptr(), ids.data_ptr(), Lmax, P + steps, int(eos_token_id), int(pad_token_id), done.data_ptr(), new_tok.data_ptr(),
                                        done_host[steps].data_ptr(), B, main.cuda_stream), "mi_greedy_advance")
        ev = torch.cuda.Event()
        ev.record(main)
        flags.append(ev)
        steps += 1
    main.synchronize()
    n = steps
    for t in range(steps):                         # steps enqueued past the one that finished the last row only wrote pads
        if bool(done_host[t].all()):
            n = t + 1
            break
    if stats is not None:
        stats["steps"] = steps
        stats["tokens"] = n
    return ids[:, :P + n]


_GENERATE_REFUSED = ("logits_processor", "stopping_criteria", "prefix_allowed_tokens_fn", "assistant_model", "streamer", "prompt_ids", "language", "task", "is_multilingual",
                     "negative_prompt_ids", "forced_decoder_ids")


def _decoder_engine_for(dec) -> WhisperDecoderEngine:
    """the HIP engine of a `WhisperDecoder` module, keyed like `_engine_for`: rebuilt when a parameter was replaced, moved or written in place"""
    params = list(dec.parameters())
    key = (str(params[0].device), tuple((p.data_ptr(), p._version) for p in params))
    cached = dec.__dict__.get("_hfasr_engine")
    if cached is not None and cached[0] == key:
        return cached[1]
    c = dec.config
    eng = WhisperDecoderEngine(dict(d_model=c.d_model, decoder_layers=c.decoder_layers, decoder_attention_heads=c.decoder_attention_heads, decoder_ffn_dim=c.decoder_ffn_dim,
                                    vocab_size=c.vocab_size, max_target_positions=c.max_target_positions, activation_function=c.activation_function,
                                    scale_embedding=False), params[0].device)       # transformers' WhisperDecoder.forward never applies embed_scale
    eng.load_state_dict(dec.state_dict())
    dec.__dict__["_hfasr_engine"] = (key, eng)
    return eng


def hip_generate(model, input_features, decoder_input_ids=None, max_new_tokens=None, max_length=None, **kw):
    """Greedy transcription of a transformers `WhisperForConditionalGeneration` on the HIP path: the bound encoder, `WhisperDecoderEngine` and `greedy_decode`
    (the recipes' case: `--num_beams=1 --predict_with_generate`).  eos / pad / suppress_tokens / begin_suppress_tokens come from `model.generation_config`; the prompt is
    `decoder_input_ids`, or `[[decoder_start_token_id]]`.  Returns (B, P + n) ids in `GenerationMixin`'s greedy layout.  What it does not do is refused with
    NotImplementedError before the device is touched — beams, sampling, timestamps, language / task prompts, custom processors or stopping criteria —: those stay
    `model.generate`, which is transformers' own and not rerouted.  CPU tensors raise RuntimeError (no fallback)."""
    gc, cfg = model.generation_config, model.config
    if kw.pop("num_beams", None) not in (None, 1) or (getattr(gc, "num_beams", 1) or 1) > 1:
        raise NotImplementedError("hip_generate is greedy: num_beams > 1 stays model.generate")
    if kw.pop("do_sample", None) or getattr(gc, "do_sample", False):
        raise NotImplementedError("hip_generate is greedy: do_sample stays model.generate")
    if kw.pop("return_timestamps", None) or getattr(gc, "return_timestamps", False):
        raise NotImplementedError("hip_generate does not apply the timestamp rules: return_timestamps stays model.generate")
    for k in _GENERATE_REFUSED:
        if kw.get(k) is not None:
            raise NotImplementedError(f"hip_generate does not take {k}=: it stays model.generate")
    if kw:
        raise NotImplementedError(f"hip_generate does not take {sorted(kw)}: it stays model.generate")
    if getattr(cfg, "scale_embedding", False):
        raise NotImplementedError("scale_embedding: transformers' WhisperDecoder computes embed_scale and never applies it; no checkpoint sets it")
    if input_features.dim() == 2:
        input_features = input_features[None]
    frames = 2 * cfg.max_source_positions
    if input_features.dim() != 3 or input_features.shape[-1] != frames:
        raise NotImplementedError(f"hip_generate takes (B, mel, {frames}) input features (long-form and shorter inputs stay model.generate), got {tuple(input_features.shape)}")
    B = input_features.shape[0]
    if decoder_input_ids is None:
        start = gc.decoder_start_token_id if getattr(gc, "decoder_start_token_id", None) is not None else cfg.decoder_start_token_id
        decoder_input_ids = torch.full((B, 1), int(start), dtype=torch.long, device=input_features.device)
    P = decoder_input_ids.shape[1]
    if max_new_tokens is None:
        max_new_tokens = (max_length if max_length is not None else (getattr(gc, "max_length", None) or cfg.max_target_positions)) - P
    if max_new_tokens < 1:
        raise ValueError(f"nothing to generate: max_new_tokens = {max_new_tokens}")
    if P + max_new_tokens > cfg.max_target_positions:
        raise ValueError(f"prompt ({P}) + max_new_tokens ({max_new_tokens}) exceeds max_target_positions = {cfg.max_target_positions}")
    eos = gc.eos_token_id if gc.eos_token_id is not None else cfg.eos_token_id
    if isinstance(eos, (list, tuple)):
        if len(eos) != 1:
            raise NotImplementedError("hip_generate takes one eos_token_id")
        eos = eos[0]
    pad = gc.pad_token_id if gc.pad_token_id is not None else cfg.pad_token_id
    if eos is None or pad is None:
        raise ValueError("generation_config needs eos_token_id and pad_token_id")
    if not input_features.is_cuda or not decoder_input_ids.is_cuda or not next(model.parameters()).is_cuda:
        raise RuntimeError("hip_generate needs the model and its inputs on the GPU (no CPU fallback)")
    enc_eng = _engine_for(model.model.encoder)
    dec_eng = _decoder_engine_for(model.model.decoder)
    with torch.no_grad():
        return greedy_decode(enc_eng, dec_eng, input_features, decoder_input_ids, max_new_tokens=max_new_tokens, eos_token_id=int(eos), pad_token_id=int(pad),
                             suppress_tokens=getattr(gc, "suppress_tokens", None), begin_suppress_tokens=getattr(gc, "begin_suppress_tokens", None))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The Whisper branch of the reference (`src/utilities/model_utils.py:183`: `AutoModelForSpeechSeq2Seq.from_pretrained(...)` on a Whisper checkpoint, e.g.
# `recipes_v0.0.1/decred/out_of_domain/decode_whisper_lumi.sh:60-66` `--from_pretrained=openai/whisper-medium --predict_with_generate`) runs HuggingFace's
# `WhisperForConditionalGeneration` as it is, and `src/trainers/train_enc_dec_asr.py:82-83` tests `isinstance(model, WhisperForConditionalGeneration)` — so the class has
# to stay HuggingFace's.  The drop-in is therefore a replacement of `WhisperEncoder.forward`: the encoder (the whole cost of config 4) runs on the HIP engine above;
# `generate`, the loss and the checkpoint format stay transformers' own.  Greedy transcription on the HIP path is the separate entry `hip_generate` above.
def _encoder_cfg(enc) -> dict:
    c = enc.config
    return dict(d_model=c.d_model, encoder_layers=c.encoder_layers, encoder_attention_heads=c.encoder_attention_heads, encoder_ffn_dim=c.encoder_ffn_dim)


def _engine_for(enc) -> WhisperEncoderEngine:
    """the HIP engine of a `WhisperEncoder` module: built at the first forward, rebuilt when a parameter was replaced, moved or written in place"""
    params = list(enc.parameters())
    key = (str(params[0].device), tuple((p.data_ptr(), p._version) for p in params))
    cached = enc.__dict__.get("_hfasr_engine")
    if cached is not None and cached[0] == key:
        return cached[1]
    eng = WhisperEncoderEngine(_encoder_cfg(enc), params[0].device)
    eng.load_state_dict(enc.state_dict())
    enc.__dict__["_hfasr_engine"] = (key, eng)
    return eng


def _stock_forward(self, why, input_features, attention_mask, kwargs):
    """What the HIP engine does not cover runs transformers' OWN `WhisperEncoder.forward` — the code the reference runs for its Whisper branch anyway (the class is
    transformers', not ours: replacing its forward process-wide must not take away what worked before).  Said once per reason; `HFASR_WHISPER_STRICT=1` raises
    instead (what the GPU parity tests run under, so that a silent PyTorch pass cannot stand in for the HIP encoder)."""
    import os
    import warnings
    if os.environ.get("HFASR_WHISPER_STRICT") == "1":
        raise NotImplementedError(f"huggingface_asr_amd: the HIP Whisper encoder does not cover this call ({why}) and HFASR_WHISPER_STRICT=1 forbids transformers' own forward")
    if why not in _stock_forward.said:
        _stock_forward.said.add(why)
        warnings.warn(f"huggingface_asr_amd: WhisperEncoder.forward runs transformers' own PyTorch implementation for this call ({why}); the HIP engine covers "
                      "inference and training (dropout 0) on GPU tensors returning last_hidden_state", stacklevel=3)
    from transformers.models.whisper import modeling_whisper as MW
    return MW.WhisperEncoder._hfasr_reference_forward(self, input_features, attention_mask=attention_mask, **kwargs)


_stock_forward.said = set()


class _WhisperEncoderFn(torch.autograd.Function):
    """Training / gradient-wanted calls: forward = `WhisperEncoderEngine.forward_train`, backward = `WhisperEncoderEngine.backward` (every pass on the HIP kernels).
    Inputs: (enc, skip, input_features, *parameters in `enc.named_parameters()` order)."""

    @staticmethod
    def forward(ctx, enc, skip, input_features, *params):
        eng = _engine_for(enc)
        out, saved = eng.forward_train(input_features, skip)
        ctx.eng, ctx.saved_fw = eng, saved
        ctx.names = [n for n, _ in enc.named_parameters()]
        ctx.in_dtype = input_features.dtype
        ctx.dtypes = [p.dtype for p in params]
        return out.to(enc.layer_norm.weight.dtype)

    @staticmethod
    def backward(ctx, dout):
        wanted = {n for n, need in zip(ctx.names, ctx.needs_input_grad[3:]) if need}
        if ctx.needs_input_grad[2]:
            wanted.add("input_features")
        G = ctx.eng.backward(ctx.saved_fw, dout, lambda n: n in wanted)
        ctx.saved_fw = None
        gin = G.get("input_features")
        out = [None, None, gin.to(ctx.in_dtype) if gin is not None else None]
        for n, dt in zip(ctx.names, ctx.dtypes):
            g = G.get(n)
            out.append(g.to(dt).contiguous() if g is not None else None)
        return tuple(out)


def _encoder_train_forward(self, input_features):
    """LayerDrop drawn here exactly as `WhisperEncoder.forward` draws it (one `torch.rand([])` per layer in training), then the HIP training forward"""
    skip = [bool(self.training and torch.rand([]) < self.layerdrop) for _ in range(len(self.layers))]
    return _WhisperEncoderFn.apply(self, skip, input_features, *[p for _, p in self.named_parameters()])


def hip_whisper_encoder_forward(self, input_features, attention_mask=None, **kwargs):
    """`transformers.models.whisper.modeling_whisper.WhisperEncoder.forward` on the HIP engine, on GPU tensors returning `last_hidden_state`: inference, and training /
    autograd through the encoder (`train_enc_dec_asr.py --do_train` on a Whisper checkpoint, `recipes_v0.0.1/librispeech_whisper_ctc`) through `_WhisperEncoderFn`,
    LayerDrop included.  Handed to transformers' own forward (`_stock_forward`): dropout > 0 in training, attention or hidden-state outputs, head masks, CPU tensors."""
    from transformers.modeling_outputs import BaseModelOutput
    cfg = self.config
    want = {k: kwargs.get(k) for k in ("output_attentions", "output_hidden_states", "head_mask")}
    if want["output_attentions"] or want["output_hidden_states"] or getattr(cfg, "output_attentions", False) or getattr(cfg, "output_hidden_states", False) \
            or want["head_mask"] is not None:
        return _stock_forward(self, "attentions / hidden states / head mask requested", input_features, attention_mask, kwargs)
    if not input_features.is_cuda:
        return _stock_forward(self, "CPU tensors", input_features, attention_mask, kwargs)
    if self.training and any(float(getattr(cfg, n, 0.0) or 0.0) > 0.0 for n in ("dropout", "attention_dropout", "activation_dropout")):
        return _stock_forward(self, "dropout > 0 in training: the library's dropout masks cannot match torch's", input_features, attention_mask, kwargs)
    if self.training or (torch.is_grad_enabled() and (input_features.requires_grad or any(p.requires_grad for p in self.parameters()))):
        return BaseModelOutput(last_hidden_state=_encoder_train_forward(self, input_features))
    out = _engine_for(self).forward(input_features=input_features)                       # (B, T/2, d) fp32; same length check / message as transformers
    return BaseModelOutput(last_hidden_state=out.to(self.layer_norm.weight.dtype))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Decoder training (opt-in: `install_whisper(decoder=True)`).  `WhisperDecoder.forward` is replaced like the encoder's; the replacement sees the RAW keyword arguments
# (transformers' `merge_with_config_defaults` decorator, which would turn use_cache=None into config.use_cache, wraps the original only), so a teacher-forced training call
# (use_cache None / False, no cache) can be told from `generate`'s cached steps.
_DECODER_KNOWN = ("input_ids", "attention_mask", "encoder_hidden_states", "past_key_values", "inputs_embeds", "position_ids", "use_cache", "output_attentions",
                  "output_hidden_states")


def decoder_route(kw: dict, *, training: bool, cfg) -> tuple[str, str | None]:
    """Where a `WhisperDecoder.forward` call with the raw keyword arguments `kw` runs: ("hip", None) — the teacher-forced pass on the HIP engine —, ("stock", None) —
    transformers' own forward, silently: cached calls, i.e. everything `generate` does —, or ("stock", reason) — transformers' own forward for a cache-less call the HIP
    path does not cover (said once per reason; HFASR_WHISPER_STRICT=1 raises).  Pure: tensors are only asked for `.is_cuda`, `cfg` for its dropout / output attributes."""
    g = kw.get
    if g("past_key_values") is not None or g("use_cache") is True:
        return "stock", None
    if g("input_ids") is None or g("inputs_embeds") is not None:
        return "stock", "inputs_embeds instead of input_ids"
    if g("encoder_hidden_states") is None:
        return "stock", "no encoder_hidden_states"
    if g("attention_mask") is not None:
        return "stock", "decoder attention_mask given"
    if g("position_ids") is not None:
        return "stock", "position_ids given"
    if g("output_attentions") or g("output_hidden_states") or getattr(cfg, "output_attentions", False) or getattr(cfg, "output_hidden_states", False):
        return "stock", "attentions / hidden states requested"
    # (num_items_in_batch: what `Trainer` hands to a forward with **kwargs; transformers' Whisper classes pass it down and nothing reads it)
    extra = sorted(k for k, v in kw.items() if k not in _DECODER_KNOWN and v is not None and k != "num_items_in_batch" and not (k == "return_dict" and v is True))
    if extra:
        return "stock", f"keyword arguments {extra}"
    if not (getattr(g("input_ids"), "is_cuda", False) and getattr(g("encoder_hidden_states"), "is_cuda", False)):
        return "stock", "CPU tensors"
    if training and any(float(getattr(cfg, n, 0.0) or 0.0) > 0.0 for n in ("dropout", "attention_dropout", "activation_dropout")):
        return "stock", "dropout > 0 in training: the library's dropout masks cannot match torch's"
    return "hip", None


def _stock_decoder_forward(self, why, kw):
    """`_stock_forward` for the decoder: transformers' own `WhisperDecoder.forward`; `why` None = a cached call (silent, also under HFASR_WHISPER_STRICT=1)"""
    import os
    import warnings
    from transformers.models.whisper import modeling_whisper as MW
    if why is not None:
        if os.environ.get("HFASR_WHISPER_STRICT") == "1":
            raise NotImplementedError(f"huggingface_asr_amd: the HIP Whisper decoder does not cover this call ({why}) and HFASR_WHISPER_STRICT=1 forbids transformers' own forward")
        if why not in _stock_decoder_forward.said:
            _stock_decoder_forward.said.add(why)
            warnings.warn(f"huggingface_asr_amd: WhisperDecoder.forward runs transformers' own PyTorch implementation for this call ({why}); the HIP engine covers the "
                          "teacher-forced pass (input_ids + encoder_hidden_states, no cache, no masks, dropout 0) on GPU tensors", stacklevel=3)
    return MW.WhisperDecoder._hfasr_reference_forward(self, **kw)


_stock_decoder_forward.said = set()


class _WhisperDecoderFn(torch.autograd.Function):
    """forward = `WhisperDecoderEngine.forward_train`, backward = `WhisperDecoderEngine.backward` (every pass on the HIP kernels).
    Inputs: (dec, skip, input_ids, encoder_hidden_states, *parameters in `dec.named_parameters()` order)."""

    @staticmethod
    def forward(ctx, dec, skip, input_ids, encoder_hidden, *params):
        eng = _decoder_engine_for(dec)
        out, saved = eng.forward_train(input_ids, encoder_hidden, skip)
        ctx.eng, ctx.saved_fw = eng, saved
        ctx.names = [n for n, _ in dec.named_parameters()]
        ctx.enc_dtype = encoder_hidden.dtype
        ctx.dtypes = [p.dtype for p in params]
        return out.to(dec.layer_norm.weight.dtype)

    @staticmethod
    def backward(ctx, dout):
        wanted = {n for n, need in zip(ctx.names, ctx.needs_input_grad[4:]) if need}
        if ctx.needs_input_grad[3]:
            wanted.add("encoder_hidden_states")
        G = ctx.eng.backward(ctx.saved_fw, dout, lambda n: n in wanted)
        ctx.saved_fw = None
        genc = G.get("encoder_hidden_states")
        out = [None, None, None, genc.to(ctx.enc_dtype) if genc is not None else None]
        for n, dt in zip(ctx.names, ctx.dtypes):
            g = G.get(n)
            out.append(g.to(dt).contiguous() if g is not None else None)
        return tuple(out)


def hip_whisper_decoder_forward(self, input_ids=None, attention_mask=None, encoder_hidden_states=None, past_key_values=None, inputs_embeds=None, position_ids=None,
                                use_cache=None, **kwargs):
    """`transformers.models.whisper.modeling_whisper.WhisperDecoder.forward`: the teacher-forced pass (what `WhisperForConditionalGeneration.forward` with labels runs
    under `train_enc_dec_asr.py --do_train`) on the HIP engine through `_WhisperDecoderFn`, LayerDrop drawn as transformers draws it; everything else — `decoder_route` —
    is transformers' own forward."""
    from transformers.modeling_outputs import BaseModelOutputWithPastAndCrossAttentions
    kw = dict(input_ids=input_ids, attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states, past_key_values=past_key_values, inputs_embeds=inputs_embeds,
              position_ids=position_ids, use_cache=use_cache, **kwargs)
    route, why = decoder_route(kw, training=self.training, cfg=self.config)
    if route != "hip":
        return _stock_decoder_forward(self, why, kw)
    skip = [bool(self.training and torch.rand([]) < self.layerdrop) for _ in range(len(self.layers))]
    out = _WhisperDecoderFn.apply(self, skip, input_ids, encoder_hidden_states, *[p for _, p in self.named_parameters()])
    return BaseModelOutputWithPastAndCrossAttentions(last_hidden_state=out, past_key_values=None)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The loss of the training step (opt-in: `install_whisper(fused_loss=True)`): proj_out — the tied (V, d) embedding — and CrossEntropyLoss as `ops.gemm_ce` /
# `ops_train.gemm_ce_bwd`: the (B U, V) fp32 logits are never written.
class TiedHeadCE(torch.autograd.Function):
    """loss = CrossEntropyLoss()(last_hidden @ weight^T, labels): the mean over the rows with label >= 0 (NaN when there is none, every gradient then exactly zero, as
    torch's).  backward -> (d last_hidden, d weight (V, d)); with the weight tied to embed_tokens autograd adds the embedding's share."""

    @staticmethod
    def forward(ctx, last_hidden, weight, labels):
        V, d = weight.shape
        hid = ops.cast_bf16(last_hidden.detach().reshape(-1, d).to(torch.float32).contiguous())
        w16 = ops.cast_bf16(weight.detach().to(torch.float32).contiguous())
        lab = labels.detach().reshape(-1).to(torch.long).contiguous()
        acc, lse, _ = ops.gemm_ce(hid, w16, lab)
        ctx.saved_fw = (hid, w16, lab, lse, acc)
        ctx.shape, ctx.dtypes = last_hidden.shape, (last_hidden.dtype, weight.dtype)
        return (acc[0] / acc[1]).to(last_hidden.dtype)

    @staticmethod
    def backward(ctx, dloss):
        from . import ops_train as OT
        hid, w16, lab, lse, acc = ctx.saved_fw
        ctx.saved_fw = None
        V, d = w16.shape
        g = torch.where(lab >= 0, dloss.to(torch.float32) / acc[1], torch.zeros((), dtype=torch.float32, device=lab.device)).contiguous()
        dl = OT.gemm_ce_bwd(hid, w16, lab, lse, g, OT.pad64(V))                    # (M, pad64(V)): the K extent of the transposed weight copy below
        dh = dw = None
        if ctx.needs_input_grad[0]:
            dh = ops.gemm(dl, OT.transpose(w16), out_dtype=torch.float32).view(ctx.shape).to(ctx.dtypes[0])
        if ctx.needs_input_grad[1]:
            dw = OT.gemm_tn_(torch.zeros((V, d), dtype=torch.float32, device=lab.device), dl, hid, n_store=V).to(ctx.dtypes[1])
        return dh, dw, None


def fused_loss_route(model, kw: dict) -> bool:
    """True when `WhisperForConditionalGeneration.forward(**kw)` (raw keyword arguments) takes the fused loss: training mode with labels, the decoder ids derived from
    them, and a decoder call that `decoder_route` sends to the HIP path"""
    g = kw.get
    labels = g("labels")
    if labels is None or not model.training or g("decoder_input_ids") is not None or g("decoder_inputs_embeds") is not None or g("return_dict") is False:
        return False
    if labels.shape[1] > model.max_target_positions or not getattr(labels, "is_cuda", False):
        return False
    src = g("input_features") if g("encoder_outputs") is None else g("encoder_outputs")[0]
    known = ("input_features", "attention_mask", "decoder_input_ids", "decoder_attention_mask", "encoder_outputs", "past_key_values", "decoder_inputs_embeds",
             "decoder_position_ids", "labels", "use_cache", "return_dict")
    dkw = dict({k: v for k, v in kw.items() if k not in known}, input_ids=labels, attention_mask=g("decoder_attention_mask"), encoder_hidden_states=src,
               past_key_values=g("past_key_values"), position_ids=g("decoder_position_ids"), use_cache=g("use_cache"))
    return src is not None and decoder_route(dkw, training=True, cfg=model.config)[0] == "hip"


def hip_whisper_lm_forward(self, input_features=None, attention_mask=None, decoder_input_ids=None, decoder_attention_mask=None, encoder_outputs=None, past_key_values=None,
                           decoder_inputs_embeds=None, decoder_position_ids=None, labels=None, use_cache=None, **kwargs):
    """`WhisperForConditionalGeneration.forward`: a training call with labels gets its loss from `TiedHeadCE` and returns `logits=None` (`Trainer.training_step` never reads
    them); eval mode, calls without labels and everything else `fused_loss_route` declines run the original forward and return logits as before."""
    from transformers.modeling_outputs import Seq2SeqLMOutput
    from transformers.models.whisper import modeling_whisper as MW
    kw = dict(input_features=input_features, attention_mask=attention_mask, decoder_input_ids=decoder_input_ids, decoder_attention_mask=decoder_attention_mask,
              encoder_outputs=encoder_outputs, past_key_values=past_key_values, decoder_inputs_embeds=decoder_inputs_embeds, decoder_position_ids=decoder_position_ids,
              labels=labels, use_cache=use_cache, **kwargs)
    if not fused_loss_route(self, kw):
        return MW.WhisperForConditionalGeneration._hfasr_reference_forward(self, **kw)
    kwargs.pop("return_dict", None)
    kwargs.pop("num_items_in_batch", None)                  # CrossEntropyLoss() takes its own mean, as the original forward's does
    ids = MW.shift_tokens_right(labels, self.config.pad_token_id, self.config.decoder_start_token_id)
    o = self.model(input_features, attention_mask=attention_mask, decoder_input_ids=ids, encoder_outputs=encoder_outputs, use_cache=use_cache, **kwargs)
    loss = TiedHeadCE.apply(o.last_hidden_state, self.proj_out.weight, labels)
    return Seq2SeqLMOutput(loss=loss, logits=None, past_key_values=o.past_key_values, decoder_hidden_states=o.decoder_hidden_states, decoder_attentions=o.decoder_attentions,
                           cross_attentions=o.cross_attentions, encoder_last_hidden_state=o.encoder_last_hidden_state, encoder_hidden_states=o.encoder_hidden_states,
                           encoder_attentions=o.encoder_attentions)


def _replace_forward(cls, ours):
    if getattr(cls.forward, "_hfasr_hip", False):
        return
    cls._hfasr_reference_forward = cls.forward
    ours._hfasr_hip = True
    cls.forward = ours


def install_whisper(decoder: bool = False, fused_loss: bool = False):
    """Give transformers' `WhisperEncoder` the HIP forward (idempotent).  The original stays reachable as `WhisperEncoder._hfasr_reference_forward` (tests compare against it).
    Opt-in: decoder=True also replaces `WhisperDecoder.forward` (`hip_whisper_decoder_forward`: the teacher-forced training pass on the HIP engine), fused_loss=True
    (implies decoder=True) wraps `WhisperForConditionalGeneration.forward` (`hip_whisper_lm_forward`: the training loss out of the tied head's GEMM, no logits); their
    originals stay reachable under the same name.  With neither, both classes are left untouched."""
    from transformers.models.whisper import modeling_whisper as MW
    _replace_forward(MW.WhisperEncoder, hip_whisper_encoder_forward)
    if decoder or fused_loss:
        _replace_forward(MW.WhisperDecoder, hip_whisper_decoder_forward)
    if fused_loss:
        _replace_forward(MW.WhisperForConditionalGeneration, hip_whisper_lm_forward)
