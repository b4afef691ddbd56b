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

    def __init__(self, cfg: dict, device="cuda:0", precision="bf16"):
        from .decoder import _check_precision
        if _check_precision("WhisperDecoderEngine", precision) == "fp32":
            raise NotImplementedError("precision='fp32' does not cover the Whisper decoder engine: use the default precision='bf16'")
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

    def step(self, ids_new: torch.Tensor, cache, kvs, T_enc: int, head_bias=None, beams: int = 1):
        """ids_new (B, U) -> fp32 logits (B, V) of the last new position (+ head_bias (V) fp32, 0 / -inf); appends to the KV cache.  One C call (mi_decoder_step).
        `beams` > 1 (beam search): the B rows are B / beams utterances x `beams` hypotheses, utterance-major, that share their utterance's cross K/V — `kvs` are the
        (B / beams * T_enc, 2d) tables of the un-replicated encoder output; one new token per row, no head bias (the beam loop masks log-probabilities, not logits):
        mi_decoder_step_beams."""
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
        if beams != 1:
            if beams < 1 or B % beams or U != 1 or head_bias is not None or kvs[0].shape[0] != B // beams * T_enc:
                raise ValueError(f"step(beams={beams}): {B} rows of {U} new tokens over cross tables of {kvs[0].shape[0]} rows (T_enc = {T_enc}), head bias "
                                 f"{'given' if head_bias is not None else 'none'}")
            _lib.check(L_.mi_decoder_step_beams(C.byref(self._gcfg), self._wtable, ids_new.data_ptr(), B, beams, U, past, Lmax, cache["tk"], cache["tv"], cache["tkv"], T_enc,
                                                None, float(self.w["scale"]), None, self._step_ws.data_ptr(), self._step_ws.numel(), buf.data_ptr(), Vp,
                                                torch.cuda.current_stream().cuda_stream), "mi_decoder_step_beams")
            cache["past"] = past + U
            return buf[:, :V]
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


def encode_for_decoding(enc_engine, dec_engine, input_features, Lmax):
    """The state a token loop starts from: the encoder run ONCE, its frames as every layer's cross K/V, and an empty KV cache of Lmax positions ->
    dict(kvs, T2, cache).  `detect_language` advances the cache by the start token; `greedy_decode(state=...)` goes on from there."""
    if not input_features.is_cuda:
        raise RuntimeError("encode_for_decoding needs device tensors (no CPU fallback)")
    enc = enc_engine.forward(input_features=input_features)
    B, T2, d = enc.shape
    return dict(kvs=dec_engine.cross_kv(ops.cast_bf16(enc.reshape(B * T2, d))), T2=T2, cache=dec_engine.init_cache(B, Lmax))


def detect_language(dec_engine, state, start_token_id, lang_ids):
    """transformers' `WhisperGenerationMixin.detect_language` on the HIP path -> (B) int64 language token ids: one decoder step over [start_token_id] whose head bias is 0
    on `lang_ids` and -inf elsewhere, then `mi_row_argmax`.  The step stays in `state`'s KV cache (past = 1), so the prompt's remaining positions follow it."""
    cache = state["cache"]
    if cache["past"] != 0:
        raise ValueError("detect_language is the first step on a fresh cache")
    V = dec_engine.cfg["vocab_size"]
    lang_ids = sorted({int(i) for i in lang_ids})
    if not lang_ids or lang_ids[0] < 0 or lang_ids[-1] >= V:
        raise ValueError(f"language token ids outside the vocabulary [0, {V})")
    B = cache["k"][0].shape[0]
    bias = torch.full((V,), float("-inf"), dtype=torch.float32, device=dec_engine.device)
    bias[torch.tensor(lang_ids, device=dec_engine.device)] = 0.0
    start = torch.full((B, 1), int(start_token_id), dtype=torch.long, device=dec_engine.device)
    return ops.row_argmax(dec_engine.step(start, cache, state["kvs"], state["T2"], bias)).to(torch.long)


def greedy_decode(enc_engine, dec_engine, input_features, prompt_ids, *, max_new_tokens, eos_token_id, pad_token_id, suppress_tokens=None, begin_suppress_tokens=None,
                  run_ahead=2, stats=None, timestamps=None, state=None):
    """Greedy transcription with the loop on the device -> (B, P + n) LongTensor: per row the prompt, the generated tokens, the first EOS (kept), then pad_token_id —
    `GenerationMixin`'s greedy layout, trimmed to the longest row.  Per token: the decoder step with the suppression vector as the head's bias (the begin-suppress ids in
    the first generated token's only), `mi_row_argmax`, and one kernel that appends the token (pad for a finished row), hands it to the next step and sets the row's done
    flag at EOS, writing the flags into pinned memory.  The host only enqueues, at most `run_ahead` steps in front of the flags it has seen, and stops once every row is
    done; nothing is copied per token.  The prompt (B, P) is consumed by one step of P positions.  `stats` receives the number of steps enqueued.
    `timestamps` = dict(no_timestamps_token_id, max_initial_timestamp_index (None = no limit), detect_from_logprob): every token is chosen under transformers'
    `WhisperTimeStampLogitsProcessor` with begin_index = P — `mi_whisper_timestamp_argmax` over the step's logits and the device-resident ids in place of `mi_row_argmax`.
    `state` (from `encode_for_decoding`; input_features is then not read): the encoder output / cross K/V to decode on and a KV cache that already holds the first
    `cache["past"]` prompt positions (the start token after `detect_language`); the first step consumes the rest of the prompt."""
    if (state is None and not input_features.is_cuda) or not prompt_ids.is_cuda:
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
    Lmax = P + max_new_tokens
    if timestamps is not None:
        ts = dict(no_timestamps_token_id=int(timestamps["no_timestamps_token_id"]), eos_token_id=int(eos_token_id),
                  max_initial_timestamp_index=timestamps.get("max_initial_timestamp_index"), detect_from_logprob=bool(timestamps.get("detect_from_logprob", True)))
        if not 0 <= ts["no_timestamps_token_id"] < V:
            raise ValueError(f"no_timestamps_token_id {ts['no_timestamps_token_id']} outside the vocabulary [0, {V})")
    if state is None:
        enc = enc_engine.forward(input_features=input_features)
        T2, d = enc.shape[1], enc.shape[2]
        kvs = dec_engine.cross_kv(ops.cast_bf16(enc.reshape(B * T2, d)))
        cache = dec_engine.init_cache(B, Lmax)
    else:
        kvs, T2, cache = state["kvs"], state["T2"], state["cache"]
        if cache["k"][0].shape[0] != B or cache["Lmax"] < Lmax or not 0 <= cache["past"] < P:
            raise ValueError(f"state does not fit: its cache holds {cache['k'][0].shape[0]} rows x {cache['Lmax']} positions with {cache['past']} consumed; "
                             f"decoding needs {B} rows x {Lmax} positions and a prompt of {P} > consumed")
    ids = torch.full((B, Lmax), int(pad_token_id), dtype=torch.long, device=dev)
    ids[:, :P] = prompt_ids
    done = torch.zeros((B,), dtype=torch.int32, device=dev)
    done_host = torch.zeros((max_new_tokens, B), dtype=torch.int32).pin_memory()
    new_tok = prompt_ids[:, cache["past"]:].to(torch.long).contiguous()
    L_ = _lib.lib()
    main = torch.cuda.current_stream()
    flags, steps = [], 0
    while steps < max_new_tokens:
        if len(flags) >= run_ahead:                # bounded run-ahead: the flags of step (now - run_ahead) are in pinned memory once its event has fired
            flags[len(flags) - run_ahead].synchronize()
            if bool(done_host[steps - run_ahead].all()):
                break
        logits = dec_engine.step(new_tok, cache, kvs, T2, first if steps == 0 else every)
        best = ops.row_argmax(logits) if timestamps is None else ops.whisper_timestamp_argmax(logits, ids, begin_index=P, cur_len=P + steps, **ts)
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


def fan_out_cache(dec_engine, src_cache, W, dst=None):
    """The self-attention cache of B prompts -> a cache of B * W rows (double-buffered, as `reorder_cache` needs it) whose rows b * W + k hold row b's consumed positions:
    `mi_kv_cache_reorder`, which gathers rows by index, with a B-row source and the index b * W + k -> b.  Positions past the consumed ones are not written: they stay
    as `init_cache` leaves them (or as the given `dst`, a cache of B * W rows and the source's positions, holds them)."""
    B, Lmax, d = src_cache["k"][0].shape
    if dst is None:
        dst = dec_engine.init_cache(B * W, Lmax)
    elif tuple(dst["k"][0].shape) != (B * W, Lmax, d):
        raise ValueError(f"fan_out_cache: dst holds {tuple(dst['k'][0].shape)}, needed {(B * W, Lmax, d)}")
    idx = torch.arange(B * W, dtype=torch.long, device=dec_engine.device) // W
    _lib.check(_lib.lib().mi_kv_cache_reorder(src_cache["tk"], src_cache["tv"], dst["tk"], dst["tv"], idx.data_ptr(), len(dst["k"]), B * W, src_cache["past"], Lmax, d,
                                              torch.cuda.current_stream().cuda_stream), "mi_kv_cache_reorder")
    dst["past"] = src_cache["past"]
    return dst


def beam_decode(enc_engine, dec_engine, input_features, prompt_ids, *, max_new_tokens, eos_token_id, pad_token_id, num_beams, length_penalty=1.0, early_stopping=False,
                suppress_tokens=None, begin_suppress_tokens=None, run_ahead=2, stats=None, timestamps=None, state=None, route=None):
    """Beam search with the loop on the device -> (B, P + n) LongTensor in the layout transformers' `_beam_search` returns for num_return_sequences = 1: per row the
    prompt, the best kept hypothesis, its EOS (kept), then pad_token_id, trimmed to the longest row.  `greedy_decode`'s arguments plus `num_beams` (2 .. 64),
    `length_penalty` and `early_stopping` (False, True, "never").
    The prompt — what `state` has not consumed of it — runs ONCE per utterance, on B rows; `fan_out_cache` then copies each row's self-attention cache to its W hypotheses,
    and the first step's logits are the B rows repeated W times under beam scores [0, -1e9, ...].  Per token after that: `WhisperDecoderEngine.step(beams=W)` (the W
    hypotheses share their utterance's cross K/V: it exists B times, not B * W times), `ops.whisper_beam_scores` (transformers applies suppression and the timestamp
    rules to log-probabilities here, so the raw row's log-sum-exp comes with the mask; the begin-suppress ids join it at the first generated position), the beam-step
    kernel `decoder.beam_loop_route` picks (ctc NULL, mask_pad 0, the length-penalty denominators of `decoder._step_denoms` with the prompt length in place of 1) and the
    cache re-ordering.  The host only enqueues, at most `run_ahead` steps in front of the pinned done flags it has seen; nothing is copied per token.
    A request `beam_loop_route` would give to a host loop (more than 64 beams, W * V >= 2^24) raises NotImplementedError before anything is enqueued.  `route` forces
    "device" / "device_wide" (tests, the bench tool).  `stats` receives steps, route and the kept hypotheses per utterance: [(score, tokens incl. the prompt)], best first."""
    from .decoder import _ES_MODE, _step_denoms, beam_loop_route
    if (state is None and not input_features.is_cuda) or not prompt_ids.is_cuda:
        raise RuntimeError("beam_decode needs device tensors (no CPU fallback)")
    dev = dec_engine.device
    B, P = prompt_ids.shape
    V, W = dec_engine.cfg["vocab_size"], int(num_beams)
    if max_new_tokens < 1:
        raise ValueError("max_new_tokens >= 1 required")
    if W < 2:
        raise ValueError("beam_decode needs num_beams >= 2 (one beam is greedy_decode)")
    if early_stopping not in _ES_MODE:
        raise ValueError(f"early_stopping must be False, True or 'never', got {early_stopping!r}")
    max_length = P + max_new_tokens
    picked = beam_loop_route(W, V, max_length)
    if picked == "host":
        raise NotImplementedError(f"beam_decode: {W} beams over {V} tokens are outside the device loop (at most 64 beams, num_beams * vocab_size < 2^24)")
    if route is not None:
        if route not in ("device", "device_wide") or (route == "device" and picked != "device"):
            raise ValueError(f"route {route!r} does not serve this request (beam_loop_route: {picked!r})")
        picked = route
    dec_engine.ensure_positions(max_length)
    for name, t in (("eos_token_id", eos_token_id), ("pad_token_id", pad_token_id)):
        if not 0 <= int(t) < V:
            raise ValueError(f"{name} {t} outside the vocabulary [0, {V})")
    eos, pad = int(eos_token_id), int(pad_token_id)
    every, first = suppression_vectors(V, suppress_tokens, begin_suppress_tokens, dev)
    ts = dict(no_timestamps_token_id=None, eos_token_id=eos)
    if timestamps is not None:
        ts = dict(no_timestamps_token_id=int(timestamps["no_timestamps_token_id"]), eos_token_id=eos,
                  max_initial_timestamp_index=timestamps.get("max_initial_timestamp_index"), detect_from_logprob=bool(timestamps.get("detect_from_logprob", True)))
        if not 0 <= ts["no_timestamps_token_id"] < V:
            raise ValueError(f"no_timestamps_token_id {ts['no_timestamps_token_id']} outside the vocabulary [0, {V})")
    if state is None:
        enc = enc_engine.forward(input_features=input_features)
        T2, d = enc.shape[1], enc.shape[2]
        kvs = dec_engine.cross_kv(ops.cast_bf16(enc.reshape(B * T2, d)))
        cache1 = dec_engine.init_cache(B, max_length)
    else:
        kvs, T2, cache1 = state["kvs"], state["T2"], state["cache"]
        if cache1["k"][0].shape[0] != B or cache1["Lmax"] < max_length or not 0 <= cache1["past"] < P:
            raise ValueError(f"state does not fit: its cache holds {cache1['k'][0].shape[0]} rows x {cache1['Lmax']} positions with {cache1['past']} consumed; "
                             f"decoding needs {B} rows x {max_length} positions and a prompt of {P} > consumed")
    # the prompt, once per utterance; its cache and its logits then fan out to the W hypotheses
    base = dec_engine.step(prompt_ids[:, cache1["past"]:].to(torch.long).contiguous(), cache1, kvs, T2)
    cache = fan_out_cache(dec_engine, cache1, W)
    n_bh, Lmax = B * W, max_length + 1
    Vp = (V + 7) // 8 * 8
    logits = torch.empty((n_bh, Vp), dtype=torch.float32, device=dev)
    logits.view(B, W, Vp)[:, :, :V] = base[:, None, :]
    logits = logits[:, :V]
    ids = torch.full((n_bh, Lmax), pad, dtype=torch.long, device=dev)
    ids[:, :P] = prompt_ids.to(torch.long).repeat_interleave(W, 0)
    beam_scores = torch.zeros((B, W), device=dev)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1).contiguous()
    done = torch.zeros((B,), dtype=torch.int32, device=dev)
    nfin = torch.zeros((B,), dtype=torch.int32, device=dev)
    fin_score = torch.zeros((B, W), dtype=torch.float32, device=dev)
    fin_len = torch.zeros((B, W), dtype=torch.int32, device=dev)
    fin_tok = torch.full((B, W, Lmax), pad, dtype=torch.long, device=dev)
    done_host = torch.zeros((max_new_tokens, B), dtype=torch.int32).pin_memory()
    L_ = _lib.lib()
    main = torch.cuda.current_stream()
    step_fn, step_name = (L_.mi_beam_step_wide, "mi_beam_step_wide") if picked == "device_wide" else (L_.mi_beam_step, "mi_beam_step")
    flags, steps, cur_len = [], 0, P
    new_tok = None
    while cur_len < max_length:
        if len(flags) >= run_ahead:                # bounded run-ahead on the pinned done flags, as in `decoder.generate`
            flags[len(flags) - run_ahead].synchronize()
            if bool(done_host[steps - run_ahead].all()):
                break
        if steps > 0:
            logits = dec_engine.step(new_tok, cache, kvs, T2, beams=W)
        lse = ops.whisper_beam_scores(logits, ids, begin_index=P, cur_len=cur_len, suppress=first if steps == 0 else every, **ts)
        new_tok = torch.empty((n_bh, 1), dtype=torch.long, device=dev)
        beam_idx = torch.empty((n_bh,), dtype=torch.long, device=dev)
        denom, heur = _step_denoms(cur_len, max_length, length_penalty, early_stopping, prompt_len=P)
        args = (logits.data_ptr(), logits.stride(0), lse.data_ptr(), None, 1.0, 0.0, 0, pad, eos, B, W, V, cur_len, max_length, Lmax, denom, heur, _ES_MODE[early_stopping],
                ids.data_ptr(), beam_scores.data_ptr(), new_tok.data_ptr(), beam_idx.data_ptr(), done.data_ptr(), nfin.data_ptr(), fin_score.data_ptr(), fin_len.data_ptr(),
                fin_tok.data_ptr(), None, None, done_host[steps].data_ptr())
        if picked == "device_wide":
            args += (None, 0, None, 0.0)
        _lib.check(step_fn(*args, main.cuda_stream), step_name)
        dec_engine.reorder_cache(cache, beam_idx)
        ev = torch.cuda.Event()
        ev.record(main)
        flags.append(ev)
        cur_len += 1
        steps += 1
    nfin_c, fs_c, fl_c, ft_c = nfin.cpu(), fin_score.cpu(), fin_len.cpu(), fin_tok.cpu()             # the first copy synchronises with everything enqueued
    if stats is not None:
        stats["steps"], stats["route"] = steps, picked
        stats["hypotheses"] = [[(float(fs_c[b, k]), ft_c[b, k, :int(fl_c[b, k])].tolist()) for k in range(int(nfin_c[b]))] for b in range(B)]
    n = int(fl_c[:, 0].max())                      # every utterance ends with kept hypotheses: at max_length the step's first W candidates all stop
    return fin_tok[:, 0, :n].contiguous()


_GENERATE_REFUSED = ("logits_processor", "stopping_criteria", "prefix_allowed_tokens_fn", "assistant_model", "streamer", "prompt_ids", "negative_prompt_ids")


LANGUAGE_TO_DETECT = -1          # stands in the language slot of `prompt_template`'s rows where the language has to be detected


def build_prompt(generation_config, config, batch_size, *, language=None, task=None, is_multilingual=None, return_timestamps=False, detect_language=None):
    """The decoder prompt of one segment -> `batch_size` equal-length lists of token ids: transformers' `WhisperGenerationMixin._set_language_and_task` followed by
    `_retrieve_init_tokens` (models/whisper/generation_whisper.py), restated without a model and without touching `generation_config`: decoder_start_token_id (the model
    config's when the generation config has none); `forced_decoder_ids` of the (generation) config only when neither task nor language is set; the language — a name, a code
    or a `<|xx|>` token, one string or one per row, mapped through `lang_to_id` — or, when none is given, the config has `lang_to_id` and the language slot is still open,
    what `detect_language()` (-> batch_size ids) finds; the task (`transcribe` when only a language is given); `no_timestamps_token_id` appended unless `return_timestamps`,
    and dropped where it is last and `return_timestamps` is set.  `language` / `task` None fall back to the attributes of `generation_config`.  Raises the ValueError /
    TypeError transformers raises at the same inputs.  Pure host code: the only device work is inside the injected `detect_language`."""
    rows, detect = prompt_template(generation_config, config, batch_size, language=language, task=task, is_multilingual=is_multilingual, return_timestamps=return_timestamps)
    if detect:
        if detect_language is None:
            raise ValueError("the language has to be detected and no `detect_language` was given")
        for r, lid in zip(rows, detect_language()):
            r[1] = int(lid)
    return rows


def prompt_template(generation_config, config, batch_size, *, language=None, task=None, is_multilingual=None, return_timestamps=False):
    """`build_prompt` up to the detection -> (rows, detect): with `detect` the language slot (index 1) of every row holds LANGUAGE_TO_DETECT for the caller to fill — the
    prompt's length and every other token do not depend on WHICH language is found, so one call sizes the KV cache before the detection step runs."""
    from transformers.models.whisper.tokenization_whisper import TASK_IDS, TO_LANGUAGE_CODE
    gc = generation_config
    issue = "https://github.com/huggingface/transformers/issues/25084#issuecomment-1664398224"
    outdated = "The generation config is outdated and is thus not compatible with the `{}` argument to `generate`. Please update the generation config as per the instructions " + issue
    multilingual = getattr(gc, "is_multilingual", None)
    if is_multilingual is not None:
        if not hasattr(gc, "is_multilingual"):
            raise ValueError(outdated.format("is_multilingual"))
        multilingual = is_multilingual
    if (hasattr(gc, "is_multilingual") or is_multilingual is not None) and not multilingual and (task is not None or language is not None):
        raise ValueError("Cannot specify `task` or `language` for an English-only model. If the model is intended to be multilingual, pass `is_multilingual=True` to generate, "
                         "or update the generation config.")
    if language is not None and not hasattr(gc, "lang_to_id"):
        raise ValueError(outdated.format("language"))
    if task is not None and not hasattr(gc, "task_to_id"):
        raise ValueError(outdated.format("task"))
    language = language if language is not None else getattr(gc, "language", None)
    task = task if task is not None else getattr(gc, "task", None)

    def language_to_id(lang):
        lang = lang.lower()
        if lang in gc.lang_to_id:
            token = lang
        elif lang in TO_LANGUAGE_CODE:
            token = f"<|{TO_LANGUAGE_CODE[lang]}|>"
        elif lang in TO_LANGUAGE_CODE.values():
            token = f"<|{lang}|>"
        else:
            raise ValueError(f"Unsupported language: {lang}. Language should be one of: {list(TO_LANGUAGE_CODE.values()) if len(lang) == 2 else list(TO_LANGUAGE_CODE.keys())}.")
        if token not in gc.lang_to_id:
            raise ValueError(f"{token} is not supported by this specific model as it is not in the `generation_config.lang_to_id`. (You should just add it to the generation config)")
        return gc.lang_to_id[token]

    start = gc.decoder_start_token_id if getattr(gc, "decoder_start_token_id", None) is not None else getattr(config, "decoder_start_token_id", None)
    if start is None:
        raise ValueError("neither the generation config nor the model config has a decoder_start_token_id")
    init = [start]
    if task is None and language is None:
        forced = getattr(gc, "forced_decoder_ids", None)
        if forced is None and getattr(config, "forced_decoder_ids", None) is not None:
            forced = config.forced_decoder_ids
        if forced is not None and forced[0][0] == 1:
            i = 1
            while len(forced) > 0 and forced[0][0] == i:
                init.append(forced[0][1])
                forced = forced[1:]
                i += 1
            if len(forced) > 0:
                raise ValueError(f"You are using token ids in `forced_decoder_ids` that do not seem to correctly follow the prompt pattern of Whisper. Make sure that {forced} "
                                 f"has an entry for all indices >= 1 and < {forced[0][0]}.")
    lang_slot_open = len(init) <= 1 or init[1] is None
    if isinstance(language, (list, tuple)):
        if any(l is None for l in language):
            raise TypeError("Expected `language` to be `None`, a single string (e.g. `'en'`), or a list of strings with length equal to the batch size (e.g. `('en', 'fr')` for "
                            "a batch size of 2). Got a list containing `None`.")
        if len(language) != batch_size:
            raise ValueError(f"When passing a list of languages, the length of the list must match the batch size. Expected length of {batch_size}, but got {len(language)} languages.")
        languages = list(language)
    elif language is None:
        languages = [None] * batch_size
    else:
        languages = [language]                           # one row now, every row below
    rows = [list(init) for _ in languages]
    lang_ids, detect = None, False
    if language is not None:
        lang_ids = [language_to_id(l) for l in languages]
    elif hasattr(gc, "lang_to_id") and lang_slot_open:
        lang_ids, detect = [LANGUAGE_TO_DETECT] * len(rows), True
    if lang_ids is not None:
        for r, lid in zip(rows, lang_ids):
            if len(r) > 1:
                r[1] = lid
            else:
                r.append(lid)
    out = []
    for r in rows:
        if task is not None:
            if task not in TASK_IDS:
                raise ValueError(f"The `{task}` task is not supported. The task should be one of `{TASK_IDS}`")
            r.append(gc.task_to_id[task])                # (transformers appends; its replace_or_add after that changes nothing)
        elif language is not None and hasattr(gc, "task_to_id"):
            if not any(t in r for t in gc.task_to_id.values()):
                r.append(gc.task_to_id["transcribe"])
        if not return_timestamps and hasattr(gc, "no_timestamps_token_id") and r[-1] != gc.no_timestamps_token_id:
            r.append(gc.no_timestamps_token_id)
        elif return_timestamps and r[-1] == gc.no_timestamps_token_id:
            r = r[:-1]
        out.append([t for t in r if t is not None])
    if len(out) == 1 and batch_size != 1:
        out = [list(out[0]) for _ in range(batch_size)]
    if any(len(r) != len(out[0]) for r in out) or len(out) != batch_size:
        raise ValueError("the prompts of a batch must have one length")           # (torch.as_tensor over ragged rows, in transformers)
    return out, detect


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


def _token_rules(gc, cfg) -> dict:
    """eos / pad / suppression ids of a generation config, as `greedy_decode` takes them"""
    eos = gc.eos_token_id if gc.eos_token_id is not None else cfg.eos_token_id
    if isinstance(eos, (list, tuple)):
        if len(eos) != 1:
            raise NotImplementedError("hip_generate takes one eos_token_id")
        eos = eos[0]
    pad = gc.pad_token_id if gc.pad_token_id is not None else cfg.pad_token_id
    if eos is None or pad is None:
        raise ValueError("generation_config needs eos_token_id and pad_token_id")
    return dict(eos_token_id=int(eos), pad_token_id=int(pad), suppress_tokens=getattr(gc, "suppress_tokens", None), begin_suppress_tokens=getattr(gc, "begin_suppress_tokens", None))


def _timestamp_rules(gc):
    """`greedy_decode`'s `timestamps` of a generation config: what `WhisperTimeStampLogitsProcessor.__init__` reads"""
    return dict(no_timestamps_token_id=gc.no_timestamps_token_id, max_initial_timestamp_index=getattr(gc, "max_initial_timestamp_index", None),
                detect_from_logprob=getattr(gc, "_detect_timestamp_from_logprob", True))


def _detected_prompt(model, gc, input_features, rows, detect, Lmax):
    """-> (prompt (B, P) on the device, state or None) of `prompt_template`'s (rows, detect): where the language has to be detected the encoder runs here, once — the
    detection step and the token loop share `state` (`encode_for_decoding` with a KV cache of Lmax positions)"""
    state = None
    if detect:
        dec_eng = _decoder_engine_for(model.model.decoder)
        dec_eng.ensure_positions(Lmax)
        state = encode_for_decoding(_engine_for(model.model.encoder), dec_eng, input_features, Lmax)
        for r, lid in zip(rows, detect_language(dec_eng, state, rows[0][0], gc.lang_to_id.values()).tolist()):
            r[1] = lid
    return torch.tensor(rows, dtype=torch.long, device=input_features.device), state


def hip_generate(model, input_features, decoder_input_ids=None, max_new_tokens=None, max_length=None, **kw):
    """Greedy transcription of one 30 s segment of a transformers `WhisperForConditionalGeneration` on the HIP path: the bound encoder, `WhisperDecoderEngine` and
    `greedy_decode` (the recipes' case: `--num_beams=1 --predict_with_generate`).  eos / pad / suppress_tokens / begin_suppress_tokens come from `model.generation_config`;
    the prompt is `decoder_input_ids`, or what transformers' `generate` builds (`build_prompt`): decoder_start_token_id, then — as far as the generation config defines them
    — the language (`language=`, one string or one per row; detected on the device when the model is multilingual and none is given), the task (`task=`), the
    `forced_decoder_ids` of the (generation) config when neither is set, and `<|notimestamps|>` unless `return_timestamps=True`, which decodes under the timestamp rules
    (`mi_whisper_timestamp_argmax`).  Returns (B, P + n) ids in `GenerationMixin`'s greedy layout, prompt included.  What it does not do is refused with
    NotImplementedError before the device is touched — beams, sampling, custom processors or stopping criteria, prompt_ids, and language / task / timestamps on a
    generation config that lacks their tables —: those stay `model.generate`.  CPU tensors raise RuntimeError (no fallback)."""
    gc, cfg = model.generation_config, model.config
    if kw.pop("num_beams", None) not in (None, 1) or (getattr(gc, "num_beams", 1) or 1) > 1:
        raise NotImplementedError("hip_generate is greedy: num_beams > 1 stays model.generate")
    if kw.pop("do_sample", None) or getattr(gc, "do_sample", False):
        raise NotImplementedError("hip_generate is greedy: do_sample stays model.generate")
    return_timestamps = kw.pop("return_timestamps", None)
    if return_timestamps is None:
        return_timestamps = getattr(gc, "return_timestamps", None)
    if return_timestamps not in (None, False, True):
        raise NotImplementedError("hip_generate takes return_timestamps as a bool")
    if return_timestamps and not hasattr(gc, "no_timestamps_token_id"):
        raise NotImplementedError("hip_generate cannot apply the timestamp rules: the generation config has no no_timestamps_token_id (it stays model.generate)")
    language, task, is_multilingual = kw.pop("language", None), kw.pop("task", None), kw.pop("is_multilingual", None)
    for name, val, table in (("language", language, "lang_to_id"), ("task", task, "task_to_id"), ("is_multilingual", is_multilingual, "is_multilingual")):
        if val is not None and not hasattr(gc, table):
            raise NotImplementedError(f"hip_generate does not take {name}= on a generation config without {table}: it stays model.generate")
    forced = kw.pop("forced_decoder_ids", None)
    if forced is not None:
        import copy
        gc = copy.copy(gc)
        gc.forced_decoder_ids = forced
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

    def new_tokens_for(P):
        n = max_new_tokens
        if n is None:
            n = (max_length if max_length is not None else (getattr(gc, "max_length", None) or cfg.max_target_positions)) - P
        if n < 1:
            raise ValueError(f"nothing to generate: max_new_tokens = {n}")
        if P + n > cfg.max_target_positions:
            raise ValueError(f"prompt ({P}) + max_new_tokens ({n}) exceeds max_target_positions = {cfg.max_target_positions}")
        return n
    B = input_features.shape[0]
    prompt_kw = dict(language=language, task=task, is_multilingual=is_multilingual, return_timestamps=bool(return_timestamps))
    rows, detect = prompt_template(gc, cfg, B, **prompt_kw)                                   # raises what transformers raises
    P = decoder_input_ids.shape[1] if decoder_input_ids is not None else len(rows[0])
    n_new = new_tokens_for(P)
    rules = _token_rules(gc, cfg)
    if not input_features.is_cuda or (decoder_input_ids is not None and not decoder_input_ids.is_cuda) or not next(model.parameters()).is_cuda:
        raise RuntimeError("hip_generate needs the model and its inputs on the GPU (no CPU fallback)")
    with torch.no_grad():
        prompt, state = (decoder_input_ids, None) if decoder_input_ids is not None else _detected_prompt(model, gc, input_features, rows, detect, P + n_new)
        return greedy_decode(_engine_for(model.model.encoder), _decoder_engine_for(model.model.decoder), input_features, prompt, max_new_tokens=n_new,
                             timestamps=_timestamp_rules(gc) if return_timestamps else None, state=state, **rules)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The Whisper branch of the reference (`src/utilities/model_utils.py:183`: `AutoModelForSpeechSeq2Seq.from_pretrained(...)` on a Whisper checkpoint, e.g.
# `recipes_v0.0.1/decred/out_of_domain/decode_whisper_lumi.sh:60-66` `--from_pretrained=openai/whisper-medium --predict_with_generate`) runs HuggingFace's
# `WhisperForConditionalGeneration` as it is, and `src/trainers/train_enc_dec_asr.py:82-83` tests `isinstance(model, WhisperForConditionalGeneration)` — so the class has
# to stay HuggingFace's.  The drop-in is therefore a replacement of `WhisperEncoder.forward`: the encoder (the whole cost of config 4) runs on the HIP engine above;
# `generate`, the loss and the checkpoint format stay transformers' own.  Greedy transcription on the HIP path is the separate entry `hip_generate` above, and — opt-in,
# `install_whisper(generate=True)` — `generate` itself for the recipes' short-form greedy calls (`hip_whisper_generate` below).
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


# ---------------------------------------------------------------------------------------------------------------------------------------------
# `WhisperForConditionalGeneration.generate` on the HIP path (opt-in: `install_whisper(generate=True)`, HFASR_WHISPER_GENERATE=1): what the reference's Whisper decoding
# recipes call through `Seq2SeqTrainer.prediction_step` (`--predict_with_generate --num_beams=1 --max_length=448`).  `generate_route` decides per call; the HIP side is
# short-form greedy decoding, everything else runs transformers' own `generate` (`_hfasr_reference_generate`).
_GENERATE_TAKEN = ("input_features", "generation_config", "attention_mask", "max_length", "max_new_tokens", "num_beams", "do_sample", "decoder_input_ids", "language", "task",
                   "is_multilingual", "return_timestamps", "return_dict_in_generate", "synced_gpus", "temperature",
                   "labels")              # `Seq2SeqTrainer.prediction_step` leaves the collator's labels among generate's inputs; transformers' generate does not read them
# keyword arguments of `generate` the HIP path hands over when they are set, and the reason it gives
_GENERATE_HANDED_OVER = (("prompt_ids", "prompt_ids"), ("prompt_condition_type", "prompt_ids"), ("condition_on_prev_tokens", "condition_on_prev_tokens"),
                         ("return_token_timestamps", "return_token_timestamps"), ("return_segments", "return_segments"),
                         ("no_speech_threshold", "no_speech_threshold / logprob_threshold / compression_ratio_threshold"),
                         ("logprob_threshold", "no_speech_threshold / logprob_threshold / compression_ratio_threshold"),
                         ("compression_ratio_threshold", "no_speech_threshold / logprob_threshold / compression_ratio_threshold"),
                         ("logits_processor", "custom logits processors / stopping criteria"), ("stopping_criteria", "custom logits processors / stopping criteria"),
                         ("prefix_allowed_tokens_fn", "custom logits processors / stopping criteria"), ("streamer", "streamer"), ("assistant_model", "assistant model"),
                         ("force_unique_generate_call", "force_unique_generate_call"), ("monitor_progress", "monitor_progress"), ("encoder_outputs", "encoder_outputs instead of input_features"))
# generation-config attributes that make `GenerationMixin.generate` add a logits processor or a stopping rule the device loop does not run: they must be unset (or neutral)
_GENERATION_CONFIG_NEUTRAL = dict(repetition_penalty=1.0, encoder_repetition_penalty=1.0, no_repeat_ngram_size=0, encoder_no_repeat_ngram_size=0, bad_words_ids=None,
                                  min_length=0, min_new_tokens=None, forced_bos_token_id=None, forced_eos_token_id=None, exponential_decay_length_penalty=None,
                                  sequence_bias=None, guidance_scale=None, watermarking_config=None, renormalize_logits=False, remove_invalid_values=False, stop_strings=None,
                                  max_time=None, num_return_sequences=1, output_scores=False, output_logits=False, output_attentions=False, output_hidden_states=False,
                                  num_beam_groups=1, penalty_alpha=None, prompt_lookup_num_tokens=None, cache_implementation=None)


BEAMS_ON_HIP = False            # the opt-in of `install_whisper(generate=True, beams=True)` / HFASR_WHISPER_BEAMS=1: `hip_whisper_generate` passes it to `generate_route`


def generate_route(kwargs: dict, generation_config, config, input_shape, beams: bool = False) -> tuple[str, str | None]:
    """Where a `WhisperForConditionalGeneration.generate(**kwargs)` call runs: ("hip", None) or ("stock", reason) — transformers' own generate, said once per reason;
    HFASR_WHISPER_STRICT=1 raises.  `kwargs`: the call's keyword arguments; `generation_config`: the one the call decodes under (the model's with the call's overrides
    applied, `GenerationMixin._prepare_generation_config`); `input_shape`: of input_features, or None.  Pure: tensors are only asked for `.is_cuda`.
    HIP: greedy (num_beams 1 / None, no sampling), short-form input (B, mel, 2 max_source_positions) on the GPU, max_length / max_new_tokens, decoder_input_ids, language
    (a string or one per row), task, is_multilingual, forced_decoder_ids of the (generation) config, return_timestamps as a bool, attention_mask (not read for short-form
    input, as in transformers), return_dict_in_generate False, labels (`Seq2SeqTrainer.prediction_step` passes the collator's along; not read, as in transformers).
    `beams` (the opt-in switch `BEAMS_ON_HIP`): num_beams 2 .. 64 — of the call or of the generation config — goes to the HIP path too (`beam_decode`, with the
    generation config's length_penalty and early_stopping and num_return_sequences 1 / None); a request outside the device beam loop's limits is handed over with a
    reason of its own.  With `beams` False every answer and every reason is what it was before the switch existed."""
    g, gc = kwargs.get, generation_config
    for name, why in _GENERATE_HANDED_OVER:
        if g(name) is not None and g(name) is not False:
            return "stock", why
    num_beams = g("num_beams") or getattr(gc, "num_beams", 1) or 1
    if num_beams > 1:
        if not beams:
            return "stock", "num_beams > 1"
        from .decoder import _ES_MODE, beam_loop_route
        if beam_loop_route(num_beams, config.vocab_size, config.max_target_positions) == "host":
            return "stock", "num_beams beyond the device beam loop (at most 64 beams, num_beams * vocab_size < 2^24)"
        es = g("early_stopping") if g("early_stopping") is not None else getattr(gc, "early_stopping", False)
        if (False if es is None else es) not in _ES_MODE:
            return "stock", "early_stopping that is not False, True or 'never'"
    temperature = g("temperature")
    if isinstance(temperature, (list, tuple)):
        if len(temperature) != 1:
            return "stock", "temperature fallback"
        temperature = temperature[0]
    if g("do_sample") or (g("do_sample") is None and getattr(gc, "do_sample", False)) or (temperature is not None and temperature > 0.0):
        return "stock", "sampling"
    if g("return_dict_in_generate") or (g("return_dict_in_generate") is None and getattr(gc, "return_dict_in_generate", False)):
        return "stock", "return_dict_in_generate"
    if g("synced_gpus"):
        return "stock", "synced_gpus"
    extra = sorted(k for k, v in kwargs.items() if k not in _GENERATE_TAKEN and k not in dict(_GENERATE_HANDED_OVER) and v is not None
                   and not hasattr(gc, k))                  # (a parameter of the generation config is judged there, below)
    if extra:
        return "stock", f"keyword arguments {extra}"
    for name in ("condition_on_prev_tokens", "no_speech_threshold", "logprob_threshold", "compression_ratio_threshold", "return_token_timestamps", "force_unique_generate_call"):
        if getattr(gc, name, None):
            return "stock", f"generation_config.{name}"
    for name, neutral in _GENERATION_CONFIG_NEUTRAL.items():
        val = getattr(gc, name, None)
        if val is not None and val != neutral:
            return "stock", f"generation_config.{name}"
    if input_shape is None or len(input_shape) != 3 or input_shape[-1] != 2 * config.max_source_positions:
        return "stock", "long-form input, or input features that are not (B, mel, 2 max_source_positions)"
    rt = g("return_timestamps")
    if rt is None:
        rt = getattr(gc, "return_timestamps", None)
    if rt not in (None, False, True):
        return "stock", "return_timestamps that is not a bool"
    if rt and not hasattr(gc, "no_timestamps_token_id"):
        return "stock", "return_timestamps on a generation config without no_timestamps_token_id"
    for name, table in (("language", "lang_to_id"), ("task", "task_to_id"), ("is_multilingual", "is_multilingual")):
        if g(name) is not None and not hasattr(gc, table):
            return "stock", f"{name} on a generation config without {table}"
    eos = gc.eos_token_id if getattr(gc, "eos_token_id", None) is not None else getattr(config, "eos_token_id", None)
    if eos is None or (isinstance(eos, (list, tuple)) and len(eos) != 1) or (getattr(gc, "pad_token_id", None) is None and getattr(config, "pad_token_id", None) is None):
        return "stock", "not exactly one eos_token_id, or no pad_token_id"
    if g("max_new_tokens") is None and g("max_length") is None and getattr(gc, "max_new_tokens", None) is None and getattr(gc, "max_length", None) is None:
        return "stock", "neither max_length nor max_new_tokens"
    if getattr(config, "scale_embedding", False):
        return "stock", "scale_embedding"
    for name in ("input_features", "decoder_input_ids"):
        if g(name) is not None and not getattr(g(name), "is_cuda", False):
            return "stock", "CPU tensors"
    return "hip", None


def _stock_generate(self, why, kwargs):
    """`_stock_forward` for `generate`: transformers' own `WhisperForConditionalGeneration.generate`, said once per reason; HFASR_WHISPER_STRICT=1 raises"""
    import os
    import warnings
    from transformers.models.whisper import modeling_whisper as MW
    if os.environ.get("HFASR_WHISPER_STRICT") == "1":
        raise NotImplementedError(f"huggingface_asr_amd: the HIP Whisper generate does not cover this call ({why}) and HFASR_WHISPER_STRICT=1 forbids transformers' own generate")
    if why not in _stock_generate.said:
        _stock_generate.said.add(why)
        warnings.warn(f"huggingface_asr_amd: WhisperForConditionalGeneration.generate runs transformers' own implementation for this call ({why}); the HIP path covers "
                      "short-form greedy decoding on GPU tensors (language / task prompts, language detection, return_timestamps)", stacklevel=3)
    return MW.WhisperForConditionalGeneration._hfasr_reference_generate(self, **kwargs)


_stock_generate.said = set()


def generate_segments(gc, config, input_features, decode_segment, *, init_tokens, decoder_input_ids=None, device=None):
    """What transformers' `WhisperGenerationMixin.generate` does around its calls of `GenerationMixin.generate`, for short-form input without temperature fallback or
    conditioning on previous text -> the ids `generate` returns: (B, longest) int64 — per row the generated tokens of its segments without the prompt columns and without
    EOS, padded on the right with pad_token_id.  Its loop: decode the 30 s window at `seek` (`decode_segment(segment_input, prompt, max_new_tokens, first)` -> (b, P + n) ids
    in `GenerationMixin`'s greedy layout), strip pads and EOS, cut at consecutive timestamp tokens and move `seek` behind the last closed one (`_retrieve_segment`), until
    every row's window is used up; rows that finish leave the batch.  The bookkeeping is transformers' own static helpers, so the layout is the installed version's.
    `gc.max_length` grows by the prompt length per segment, as transformers' generation config does across its loop."""
    from transformers.models.whisper import generation_whisper as GW
    mixin = GW.WhisperGenerationMixin
    B, total = input_features.shape[0], input_features.shape[-1]
    stride = 2                                             # conv1.stride * conv2.stride of every Whisper encoder
    nseg = stride * config.max_source_positions
    timestamp_begin = gc.no_timestamps_token_id + 1 if hasattr(gc, "no_timestamps_token_id") else config.vocab_size + 1
    max_frames, seek = torch.full((B,), total, dtype=torch.long), torch.zeros((B,), dtype=torch.long)
    batch_idx_map, cur_bsz, feats = list(range(B)), B, input_features
    segments = [[] for _ in range(B)]
    max_length, max_new = getattr(gc, "max_length", None), getattr(gc, "max_new_tokens", None)
    first = True
    while bool((seek < max_frames).any()):
        feats, cur_bsz, batch_idx_map = mixin._maybe_reduce_batch(feats, seek, max_frames, cur_bsz, batch_idx_map)
        time_offset = seek.to(torch.float64) * 0.02 / stride
        seek_num_frames = (max_frames - seek).clamp(max=nseg)
        segment_input = mixin._get_input_segment(feats, seek, seek_num_frames, nseg, cur_bsz, batch_idx_map)
        prompt = decoder_input_ids if decoder_input_ids is not None else init_tokens[batch_idx_map]
        P = prompt.shape[-1]
        if (max_new or 0) + P > config.max_target_positions:                # `_set_max_new_tokens_and_length`
            raise ValueError(f"The length of `decoder_input_ids`, including special start tokens, prompt tokens, and previous tokens, is {P},  and `max_new_tokens` is "
                             f"{max_new or 0}. Thus, the combined length of `decoder_input_ids` and `max_new_tokens` is: {(max_new or 0) + P}. This exceeds the "
                             f"`max_target_positions` of the Whisper model: {config.max_target_positions}. You should either reduce the length of your prompt, or reduce the "
                             f"value of `max_new_tokens`, so that their combined length is less than {config.max_target_positions}.")
        if max_length is not None and max_new is None:
            max_length = min(max_length + min(config.max_target_positions // 2 - 1, P), config.max_target_positions)
        n_new = max_new if max_new is not None else max_length - P
        if n_new < 1:
            raise ValueError(f"Input length of decoder_input_ids is {P}, but `max_length` is set to {P + n_new}. This can lead to unexpected behavior. You should consider "
                             "increasing `max_length` or, better yet, setting `max_new_tokens`.")
        out = decode_segment(segment_input, prompt, n_new, first)
        first = False
        for i, seq in enumerate(out[:, P:]):
            prev_i = batch_idx_map[i]
            if seq[-1] == gc.pad_token_id:                                  # `generate_with_fallback`: every pad goes, EOS stays for now
                n_pad = int((seq == gc.pad_token_id).sum())
                if gc.pad_token_id == gc.eos_token_id:
                    n_pad -= 1
                if n_pad != 0:
                    seq = seq[:-n_pad]
            if seq[-1] == gc.eos_token_id:
                seq = seq[:-1]
            segs, offset = mixin._retrieve_segment(seek_sequence=seq, seek_outputs=out, time_offset=time_offset, timestamp_begin=timestamp_begin, seek_num_frames=seek_num_frames,
                                                   time_precision=0.02, time_precision_features=0.01, input_stride=stride, prev_idx=prev_i, idx=i, return_token_timestamps=False,
                                                   decoder_input_ids=prompt)
            if int(offset) <= 0:                                            # two timestamps at <|0.00|>: transformers' loop would decode the same window for ever
                raise RuntimeError("Whisper segment loop does not advance: the decoded segment closes at timestamp 0")
            seek[prev_i] += offset
            segments[prev_i] += segs
    return GW._pad_to_max_length(current_segments=segments, pad_token_id=gc.pad_token_id, device=device if device is not None else input_features.device, padding_side="right",
                                 return_token_timestamps=False, force_unique_generate_call=False)


def resolved_generation_config(model, generation_config, kwargs: dict):
    """the generation config a `generate(generation_config=..., **kwargs)` call decodes under: a copy of the model's (or the given one) with the call's generation
    parameters applied — `GenerationMixin._prepare_generation_config` on the keyword arguments that are not parameters of Whisper's own `generate` (those never reach it
    in transformers either)"""
    import inspect
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin
    own = set(inspect.signature(WhisperGenerationMixin.generate).parameters)
    return model._prepare_generation_config(generation_config, **{k: v for k, v in kwargs.items() if k not in own})[0]


def hip_whisper_generate(self, input_features=None, generation_config=None, **kwargs):
    """`WhisperForConditionalGeneration.generate`: short-form greedy calls — `generate_route` — on the HIP path (`build_prompt`, `detect_language`, `greedy_decode`, the
    timestamp rules in `mi_whisper_timestamp_argmax`), returning what transformers' own generate returns for the call (`generate_segments`); every other call is
    transformers' own generate.  With `BEAMS_ON_HIP` set (`install_whisper(generate=True, beams=True)`) calls whose resolved num_beams is 2 .. 64 take the HIP path too:
    their `decode_segment` is `beam_decode`, whose layout `generate_segments` strips like the greedy one."""
    raw = dict(kwargs, input_features=input_features, generation_config=generation_config)
    gc = resolved_generation_config(self, generation_config, kwargs)
    route, why = generate_route(raw, gc, self.config, tuple(input_features.shape) if input_features is not None else None, beams=BEAMS_ON_HIP)
    if route == "hip" and not next(self.parameters()).is_cuda:
        route, why = "stock", "CPU tensors"
    if route != "hip":
        return _stock_generate(self, why, raw)
    g = kwargs.get
    rt = g("return_timestamps") if g("return_timestamps") is not None else getattr(gc, "return_timestamps", None)
    prompt_kw = dict(language=g("language"), task=g("task"), is_multilingual=g("is_multilingual"), return_timestamps=bool(rt))
    rules = _token_rules(gc, self.config)
    gc.eos_token_id, gc.pad_token_id = rules["eos_token_id"], rules["pad_token_id"]
    timestamps = _timestamp_rules(gc) if rt else None
    num_beams = int(getattr(gc, "num_beams", 1) or 1)                                             # > 1 only where `generate_route` let it through: BEAMS_ON_HIP
    length_penalty = float(gc.length_penalty if getattr(gc, "length_penalty", None) is not None else 1.0)
    early_stopping = getattr(gc, "early_stopping", False) or False
    cfg, B = self.config, input_features.shape[0]
    enc_eng, dec_eng = _engine_for(self.model.encoder), _decoder_engine_for(self.model.decoder)
    dec_in = g("decoder_input_ids")
    with torch.no_grad():
        rows, detect = prompt_template(gc, cfg, B, **prompt_kw)                                   # raises what transformers raises, also when decoder_input_ids is given
        P, mtp = len(rows[0]), cfg.max_target_positions                                           # the first segment's positions, as `generate_segments` will count them
        Lmax = min(P + gc.max_new_tokens, mtp) if getattr(gc, "max_new_tokens", None) is not None else min(gc.max_length + min(mtp // 2 - 1, P), mtp)
        if dec_in is not None:                                                                    # (the prompt as given: nothing to detect for)
            rows, detect = [[0 if t == LANGUAGE_TO_DETECT else t for t in r] for r in rows], False
        init_tokens, state = _detected_prompt(self, gc, input_features, rows, detect, max(Lmax, P + 1))

        def decode_segment(segment_input, prompt, n_new, first):
            st = state if first and state is not None and state["cache"]["Lmax"] >= prompt.shape[1] + n_new else None       # the detection step's encoder output and cache
            if num_beams > 1:
                return beam_decode(enc_eng, dec_eng, segment_input, prompt.contiguous(), max_new_tokens=n_new, num_beams=num_beams, length_penalty=length_penalty,
                                   early_stopping=early_stopping, timestamps=timestamps, state=st, **rules)
            return greedy_decode(enc_eng, dec_eng, segment_input, prompt.contiguous(), max_new_tokens=n_new, timestamps=timestamps, state=st, **rules)
        return generate_segments(gc, cfg, input_features, decode_segment, init_tokens=init_tokens, decoder_input_ids=dec_in, device=self.device)


def _replace_forward(cls, ours):
    if getattr(cls.forward, "_hfasr_hip", False):
        return
    cls._hfasr_reference_forward = cls.forward
    ours._hfasr_hip = True
    cls.forward = ours


def install_whisper(decoder: bool = False, fused_loss: bool = False, generate: bool = False, beams: bool = False):
    """Give transformers' `WhisperEncoder` the HIP forward (idempotent).  The original stays reachable as `WhisperEncoder._hfasr_reference_forward` (tests compare against it).
    Opt-in: decoder=True also replaces `WhisperDecoder.forward` (`hip_whisper_decoder_forward`: the teacher-forced training pass on the HIP engine), fused_loss=True
    (implies decoder=True) wraps `WhisperForConditionalGeneration.forward` (`hip_whisper_lm_forward`: the training loss out of the tied head's GEMM, no logits),
    generate=True replaces `WhisperForConditionalGeneration.generate` (`hip_whisper_generate`: short-form greedy decoding on the HIP path; the original stays reachable as
    `WhisperForConditionalGeneration._hfasr_reference_generate`); the other originals stay reachable under `_hfasr_reference_forward`.  With none of them, the decoder and
    `WhisperForConditionalGeneration` are left untouched.  generate=True with beams=True also sends beam search (num_beams 2 .. 64) to the HIP path (`beam_decode`): the
    module-level switch `BEAMS_ON_HIP`, which every call with generate=True sets — to off when `beams` is not given."""
    global BEAMS_ON_HIP
    from transformers.models.whisper import modeling_whisper as MW
    if beams and not generate:
        raise ValueError("install_whisper(beams=True) needs generate=True")
    if generate:
        BEAMS_ON_HIP = bool(beams)
    _replace_forward(MW.WhisperEncoder, hip_whisper_encoder_forward)
    if decoder or fused_loss:
        _replace_forward(MW.WhisperDecoder, hip_whisper_decoder_forward)
    if fused_loss:
        _replace_forward(MW.WhisperForConditionalGeneration, hip_whisper_lm_forward)
    if generate and not getattr(MW.WhisperForConditionalGeneration.generate, "_hfasr_hip", False):
        MW.WhisperForConditionalGeneration._hfasr_reference_generate = MW.WhisperForConditionalGeneration.generate
        hip_whisper_generate._hfasr_hip = True
        MW.WhisperForConditionalGeneration.generate = hip_whisper_generate
