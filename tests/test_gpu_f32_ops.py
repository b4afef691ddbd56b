"""The operators of the fp32 inference mode (huggingface_asr_amd/csrc/gemm_f32.hip, encoder_f32.hip; wrappers in huggingface_asr_amd/ops_f32.py), one by one, against
float64 references on the host.

  a. mi_gemm_f32 against a float64 host product at the tile (128) and K-pair edges, both load paths (16-byte and scalar: leading dimensions that are / are not a
     multiple of 4), every combination of bias, alpha and residual (none / distinct / aliasing the output).  Bound per element, computed here in float64:
         (K + 8) * 2**-24 * (sum_k |a_k w_k| + |bias| + |resid|)
     — the f32-input MFMA is a k-ordered fma chain with one rounding per step (<= K roundings), plus a handful for bias, scale and residual: the standard gamma_n
     bound to first order.  Two runs give the same bits.  The output is a view inside a NaN-filled buffer whose padding must stay NaN.
  b. the erf-GELU epilogue at K = 33: the bound above x 1.13 (max |GELU'|) + E, E = 2 x max |F.gelu (fp32, on the device) - float64 GELU| over the same
     pre-activations — two independent fp32 erf implementations, each a few ulp from the truth.
  c. the fp32 attention (projections, relative shift or rotary, masks, softmax, P.V, output projection) against oracle.ebranchformer_ref.self_attention evaluated
     in float64 on the CPU.  Allowance per case: 16 x max |oracle fp32 (CPU torch) - oracle float64| on the same inputs — torch's own fp32 is the reference's
     noise; serial MFMA chains and another softmax order may be several times worse than torch's blocked sums, not a hundred times.  Each case also runs with a
     scores workspace of one utterance and of 37 query rows: the chunked walks must give the bits of the un-chunked one.
  d. depthwise conv, CSGU (inside the cgMLP), LayerNorm and the Conv2d front end against their oracle functions in float64, same 16 x rule.
Every test prints its figures (pytest -s): `F32OPS <what> <case> err=<observed> allow=<allowance> ratio=<err / reference noise>`."""
import math

import pytest
import torch

from oracle import ebranchformer_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24


def _ops():
    from huggingface_asr_amd import ops_f32
    return ops_f32


def _rand(gen, *shape, scale=1.0):
    """uniform in [-scale, scale), float64 holding fp32-representable values: the float64 reference, torch's fp32 and the device all see the SAME inputs, so the
    difference between the first two is arithmetic noise alone (no input-rounding term that would widen the allowance)"""
    return ((torch.rand(*shape, generator=gen, dtype=F64) * 2 - 1) * scale).float().double()


def _strided(t, ld, fill=float("nan")):
    """a device copy of the 2-D fp32 tensor t as a view with row stride ld inside a `fill`ed buffer -> (view, buffer)"""
    buf = torch.full((t.shape[0] + 1, ld), fill, dtype=F32, device=DEV)
    buf[: t.shape[0], : t.shape[1]] = t.to(DEV)
    return buf[: t.shape[0], : t.shape[1]], buf


def _ld(K, vec):
    """a leading dimension > K: a multiple of 4 (the 16-byte load path) or = 1 mod 4 (the scalar path)"""
    base = (K + 3) // 4 * 4
    return base + 4 if vec else base + 5


# ----------------------------------------------------------------------------------------------------------------- a / b: GEMM
GEMM_SHAPES = [(M, N, K) for M in (1, 31, 33, 129) for N in (1, 33, 130) for K in (1, 2, 3, 33, 130, 2048)]


def _gemm_inputs(M, N, K):
    gen = torch.Generator().manual_seed(1000 * M + 10 * N + K)
    a, w = _rand(gen, M, K).float(), _rand(gen, N, K).float()
    bias, resid = _rand(gen, N).float(), _rand(gen, M, N, scale=2.0).float()
    a64, w64 = a.double(), w.double()
    return a, w, bias, resid, a64 @ w64.T, a64.abs() @ w64.abs().T


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in GEMM_SHAPES])
def test_gemm_f32_against_float64(M, N, K):
    O = _ops()
    a, w, bias, resid, prod, mag = _gemm_inputs(M, N, K)
    worst = 0.0
    for vec in (True, False):
        av, _ = _strided(a, _ld(K, vec), fill=7.0)           # finite junk beside the operands: a read past K would change every sum
        wv, _ = _strided(w, _ld(K, vec), fill=7.0)
        bd, rd = bias.to(DEV), resid.to(DEV)
        for use_bias in (False, True):
            for alpha in (1.0, 0.5):
                for rmode in ("none", "distinct", "alias"):
                    want = prod + (bias.double()[None] if use_bias else 0.0)
                    want = want * alpha + (resid.double() if rmode != "none" else 0.0)
                    bound = (K + 8) * U * (mag + (bias.double().abs()[None] if use_bias else 0.0) + (resid.double().abs() if rmode != "none" else 0.0))
                    got = []
                    for _ in range(2):
                        buf = torch.full((M + 1, N + 5), float("nan"), dtype=F32, device=DEV)
                        out = buf[:M, :N]
                        r = None
                        if rmode == "alias":
                            out.copy_(rd)
                            r = out
                        elif rmode == "distinct":
                            r = rd
                        O.gemm(av, wv, bd if use_bias else None, out, resid=r, alpha=alpha)
                        torch.cuda.synchronize()
                        assert torch.isnan(buf[:M, N:]).all() and torch.isnan(buf[M]).all(), "the GEMM wrote outside its output"
                        got.append(out.cpu())
                    assert torch.equal(got[0], got[1]), "two runs differ"
                    err = (got[0].double() - want).abs()
                    assert torch.isfinite(got[0]).all()
                    worst = max(worst, float((err / bound).max()))
                    assert bool((err <= bound).all()), (vec, use_bias, alpha, rmode, float((err / bound).max()))
    print(f"F32OPS gemm {M}x{N}x{K} worst err/bound={worst:.3f}")


GELU_SHAPES = [(M, N, 33) for M in (1, 31, 33, 129) for N in (1, 33, 130)]


@pytest.mark.parametrize("M,N,K", GELU_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in GELU_SHAPES])
def test_gemm_f32_gelu_epilogue(M, N, K):
    O = _ops()
    a, w, bias, _, _, _ = _gemm_inputs(M, N, K)
    a = a * 3                                                     # pre-activations over a few units: both tails of the GELU
    prod, mag = a.double() @ w.double().T, a.double().abs() @ w.double().abs().T
    gelu64 = lambda x: 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    pre = prod + bias.double()[None]
    want = gelu64(pre)
    pre32 = pre.float()
    E = 2 * float((torch.nn.functional.gelu(pre32.to(DEV)).cpu().double() - gelu64(pre32.double())).abs().max())
    bound = 1.13 * (K + 8) * U * (mag + bias.double().abs()[None]) + E
    for vec in (True, False):
        av, _ = _strided(a, _ld(K, vec), fill=7.0)
        wv, _ = _strided(w, _ld(K, vec), fill=7.0)
        got = [O.gemm(av, wv, bias.to(DEV), act="gelu").cpu() for _ in range(2)]
        assert torch.equal(got[0], got[1])
        err = (got[0].double() - want).abs()
        print(f"F32OPS gelu {M}x{N}x{K} vec={int(vec)} err={float(err.max()):.3e} E={E:.3e} worst err/bound={float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())


def test_gemm_f32_refuses_bad_arguments():
    O = _ops()
    a, w = torch.zeros((4, 8), device=DEV), torch.zeros((4, 8), device=DEV)
    with pytest.raises(ValueError):
        O.gemm(a, torch.zeros((4, 7), device=DEV))
    with pytest.raises(TypeError):
        O.gemm(a.bfloat16(), w)
    with pytest.raises(RuntimeError):
        O.gemm(a, w, out=torch.zeros((32,), device=DEV).as_strided((4, 4), (3, 1)))               # ldc < N: rows would overlap


# ----------------------------------------------------------------------------------------------------------------- c: attention
ATT_CASES = [(T, H, hd, full, ptype, causal) for T in (1, 31, 33, 65, 130) for H, hd in ((4, 16), (2, 64), (1, 128)) for full in (True, False)
             for ptype in ("relative", "rotary") for causal in (False, True)]


def _attn_sd(gen, d, H, ptype, dtype):
    pre = "a."
    sd = {}
    for n in ("q", "k", "v", "out"):
        sd[f"{pre}linear_{n}.weight"] = _rand(gen, d, d, scale=1.5 / math.sqrt(d)).to(dtype)
        sd[f"{pre}linear_{n}.bias"] = _rand(gen, d, scale=0.2).to(dtype)
    if ptype == "relative":
        sd[pre + "linear_pos.weight"] = _rand(gen, d, d, scale=1.5 / math.sqrt(d)).to(dtype)
        sd[pre + "pos_bias_u"] = _rand(gen, H, d // H, scale=0.5).to(dtype)
        sd[pre + "pos_bias_v"] = _rand(gen, H, d // H, scale=0.5).to(dtype)
    return sd


def _add_mask(lengths, T, dtype):
    mask = torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]
    am = (1.0 - mask[:, None, None, :].to(dtype)) * torch.finfo(torch.float32).min
    return am.expand(-1, 1, T, -1)


def _oracle_attention(sd64, cfg, x64, lengths, dtype):
    T, d, H = x64.shape[1], x64.shape[2], cfg["num_attention_heads"]
    sd = {k: v.to(dtype) for k, v in sd64.items()}
    if cfg["position_embeddings_type"] == "relative":
        pos = R.rel_pos_table(T, d).to(dtype)                   # the fp32 sinusoid table, as the device path is given it
    else:
        pos = tuple(t.to(dtype) for t in R.rotary_table(T, d // H))
    return R.self_attention(sd, "a.", cfg, x64.to(dtype), _add_mask(lengths, T, dtype), pos)


def _device_attention(O, sd64, cfg, x64, lengths, workspace_bytes=None):
    B, T, d = x64.shape
    H = cfg["num_attention_heads"]
    g = lambda k: sd64["a." + k].float().to(DEV).contiguous()
    x = x64.float().to(DEV).reshape(B * T, d)
    rel = cfg["position_embeddings_type"] == "relative"
    xq = x
    if not rel:
        cos, sin = R.rotary_table(T, d // H)
        xq = O.rotary(x, cos.to(DEV).contiguous(), sin.to(DEV).contiguous(), T, H)
    qkv = torch.empty((B * T, 3 * d), dtype=F32, device=DEV)      # [Q | K | V] row views, as the driver lays them out
    O.gemm(xq, g("linear_q.weight"), g("linear_q.bias"), qkv[:, :d])
    O.gemm(xq, g("linear_k.weight"), g("linear_k.bias"), qkv[:, d:2 * d])
    O.gemm(x, g("linear_v.weight"), g("linear_v.bias"), qkv[:, 2 * d:])
    kw = {}
    if rel:
        kw = dict(pos=O.gemm(R.rel_pos_table(T, d).to(DEV), g("linear_pos.weight")), bias_u=g("pos_bias_u").reshape(-1), bias_v=g("pos_bias_v").reshape(-1))
    ctx = O.attention(qkv[:, :d], qkv[:, d:2 * d], qkv[:, 2 * d:], B, T, H, lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV),
                      causal=cfg["is_causal"], workspace_bytes=workspace_bytes, **kw)
    return O.gemm(ctx, g("linear_out.weight"), g("linear_out.bias")).reshape(B, T, d).cpu()


@pytest.mark.parametrize("T,H,hd,full,ptype,causal", ATT_CASES,
                         ids=[f"T{t}-{h}x{e}-{'full' if f else 'short'}-{p[:3]}-{'causal' if c else 'bidir'}" for t, h, e, f, p, c in ATT_CASES])
def test_attention_f32_against_float64_oracle(T, H, hd, full, ptype, causal):
    O = _ops()
    B, d = 2, H * hd
    lengths = [T, 1] if full else [T - 1, T]
    cfg = dict(num_attention_heads=H, position_embeddings_type=ptype, is_causal=causal)
    gen = torch.Generator().manual_seed(7 * T + 3 * H + hd + 2 * int(full) + int(causal))
    sd64 = _attn_sd(gen, d, H, ptype, F64)
    x64 = _rand(gen, B, T, d, scale=1.7)
    with torch.no_grad():
        want = _oracle_attention(sd64, cfg, x64, lengths, F64)
        noise = float((_oracle_attention(sd64, cfg, x64, lengths, F32).double() - want).abs().max())
    got = _device_attention(O, sd64, cfg, x64, lengths)
    err = float((got.double() - want).abs().max())
    print(f"F32OPS attention T{T}-{H}x{hd}-{lengths}-{ptype}-causal{int(causal)} err={err:.3e} allow={16 * noise:.3e} ratio={err / max(noise, 1e-30):.2f}")
    assert torch.isfinite(got).all()
    assert err <= 16 * noise
    # chunk edges of the scores walk: one utterance per chunk; 37 query rows per chunk (row blocks that end inside an utterance)
    rowf = O.attention_workspace_bytes(B, T, H, hd, ptype == "relative") // (B * T)          # bytes per query row (these shapes are far below the bound)
    for rows in (T, 37):
        again = _device_attention(O, sd64, cfg, x64, lengths, workspace_bytes=rowf * rows)
        assert torch.equal(again, got), f"a scores workspace of {rows} query rows changed the result"


def test_attention_f32_workspace_is_bounded():
    O = _ops()
    assert O.attention_workspace_bytes(2, 33, 4, 16, True) == 2 * 33 * 4 * (2 * 4 * 16 + 4 * (36 + 68))
    for B, T in ((32, 250), (96, 500), (8, 6000)):
        assert O.attention_workspace_bytes(B, T, 8, 64, True) <= O.SCORES_BOUND
        assert B * 8 * T * (3 * T - 1) * 4 > O.SCORES_BOUND                # the un-chunked product would not fit


# ----------------------------------------------------------------------------------------------------------------- d: the other operators
def _report(what, case, got, want64, noise):
    err = float((got.double() - want64).abs().max())
    print(f"F32OPS {what} {case} err={err:.3e} allow={16 * noise:.3e} ratio={err / max(noise, 1e-30):.2f}")
    assert torch.isfinite(got).all()
    assert err <= 16 * noise, (what, case, err, noise)


@pytest.mark.parametrize("T", [1, 15, 16, 31, 33])
@pytest.mark.parametrize("causal", [False, True])
def test_dwconv_f32(T, causal):
    """k = 31 over T shorter than, equal to and longer than the half kernel; C = 260 spans two channel blocks; the causal form with the CSGU's dilation quirk"""
    O = _ops()
    B, C, K = 2, 260, 31
    gen = torch.Generator().manual_seed(31 * T + int(causal))
    x, w, b = _rand(gen, B, T, C), _rand(gen, C, 1, K, scale=0.3), _rand(gen, C, scale=0.2)
    dil = (K - 1) // 2
    ref = lambda dt: R.dwconv1d(x.to(dt), w.to(dt), b.to(dt), causal, dil)
    want, noise = ref(F64), float((ref(F32).double() - ref(F64)).abs().max())
    xd = x.float().to(DEV).reshape(B * T, C)
    wd, bd = w.float().to(DEV).reshape(C, K).contiguous(), b.float().to(DEV)
    pad = (K - 1) * dil if causal else (K - 1) // 2
    got = O.dwconv(xd, wd, bd, B, T, pad_left=pad, dilation=dil if causal else 1).reshape(B, T, C).cpu()
    _report("dwconv", f"T{T}-causal{int(causal)}", got, want, noise)
    if not causal:           # the merge: m + dwconv(m)   (e_branchformer.py:297-299)
        got = O.dwconv(xd, wd, bd, B, T, residual=True).reshape(B, T, C).cpu()
        res = lambda dt: x.to(dt) + R.dwconv1d(x.to(dt), w.to(dt), b.to(dt))
        _report("dwconv+residual", f"T{T}", got, res(F64), float((res(F32).double() - res(F64)).abs().max()))


CSGU_CASES = [("identity", False, False), ("gelu", True, False), ("identity", False, True), ("silu", True, True)]


@pytest.mark.parametrize("T", [1, 15, 16, 31, 33])
@pytest.mark.parametrize("act,linear,causal", CSGU_CASES, ids=[f"{a}-lin{int(l)}-causal{int(c)}" for a, l, c in CSGU_CASES])
def test_cgmlp_f32(T, act, linear, causal):
    """channel_proj1 + GELU, CSGU (LayerNorm over I/2, depthwise conv, optional Linear + activation, gate), channel_proj2 against oracle.cgmlp"""
    O = _ops()
    B, d, I, K = 2, 48, 72, 31
    cfg = dict(is_causal=causal, csgu_use_linear_after_conv=linear, csgu_activation=act)
    gen = torch.Generator().manual_seed(17 * T + len(act) + int(causal))
    sd = {"c.channel_proj1.0.weight": _rand(gen, I, d, scale=0.3), "c.channel_proj1.0.bias": _rand(gen, I, scale=0.2),
          "c.csgu.norm.weight": 1 + _rand(gen, I // 2, scale=0.3), "c.csgu.norm.bias": _rand(gen, I // 2, scale=0.2),
          "c.csgu.conv.weight": _rand(gen, I // 2, 1, K, scale=0.3), "c.csgu.conv.bias": _rand(gen, I // 2, scale=0.2),
          "c.csgu.linear.weight": _rand(gen, I // 2, I // 2, scale=0.3), "c.csgu.linear.bias": _rand(gen, I // 2, scale=0.2),
          "c.channel_proj2.weight": _rand(gen, d, I // 2, scale=0.3), "c.channel_proj2.bias": _rand(gen, d, scale=0.2)}
    x = _rand(gen, B, T, d, scale=1.5)
    ref = lambda dt: R.cgmlp({k: v.to(dt) for k, v in sd.items()}, "c.", cfg, x.to(dt))
    with torch.no_grad():
        want, noise = ref(F64), float((ref(F32).double() - ref(F64)).abs().max())
    g = lambda k: sd["c." + k].float().to(DEV).contiguous()
    h = O.gemm(x.float().to(DEV).reshape(B * T, d), g("channel_proj1.0.weight"), g("channel_proj1.0.bias"), act="gelu")
    s = O.csgu(h, g("csgu.norm.weight"), g("csgu.norm.bias"), g("csgu.conv.weight").reshape(I // 2, K), g("csgu.conv.bias"), B, T, causal=causal, act=act,
               lin_w=g("csgu.linear.weight") if linear else None, lin_b=g("csgu.linear.bias") if linear else None)
    got = O.gemm(s, g("channel_proj2.weight"), g("channel_proj2.bias")).reshape(B, T, d).cpu()
    _report("cgmlp", f"T{T}-{act}-lin{int(linear)}-causal{int(causal)}", got, want, noise)


@pytest.mark.parametrize("M,d", [(1, 1), (5, 63), (7, 64), (9, 65), (6, 513)])
def test_layernorm_f32(M, d):
    O = _ops()
    gen = torch.Generator().manual_seed(M * 1000 + d)
    x, g, b = _rand(gen, M, d, scale=3.0) + 0.5, 1 + _rand(gen, d, scale=0.3), _rand(gen, d, scale=0.2)
    for eps in (1e-5, 1e-3):
        ref = lambda dt: R.layer_norm(x.to(dt), g.to(dt), b.to(dt), eps)
        want, noise = ref(F64), float((ref(F32).double() - ref(F64)).abs().max())
        xv, _ = _strided(x.float(), d + 3)
        got = O.layernorm(xv, g.float().to(DEV), b.float().to(DEV), eps).cpu()
        if d == 1:           # (x - mean) is exactly 0: the output is beta in every arithmetic
            assert torch.equal(got, b.float()[None].expand(M, 1))
            continue
        _report("layernorm", f"{M}x{d}-eps{eps}", got, want, noise)


def test_layernorm_f32_zeroes_padded_frames():
    """tf:662-665: frames past an utterance's length are zeroed before the first LayerNorm — x_out receives them, their LayerNorm is beta"""
    O = _ops()
    B, T, d = 3, 5, 40
    gen = torch.Generator().manual_seed(5)
    x, g, b = _rand(gen, B * T, d).float(), (1 + _rand(gen, d, scale=0.3)).float(), _rand(gen, d, scale=0.2).float()
    lengths = [5, 2, 0]
    keep = (torch.arange(T)[None] < torch.tensor(lengths)[:, None]).reshape(-1)
    xd = x.to(DEV)
    y = O.layernorm(xd, g.to(DEV), b.to(DEV), lengths=torch.tensor(lengths, dtype=torch.int32, device=DEV), T=T, x_out=xd).cpu()
    assert torch.equal(xd.cpu(), x * keep[:, None])
    want = R.layer_norm((x * keep[:, None]).double(), g.double(), b.double())
    assert float((y.double() - want).abs().max()) < 1e-5
    assert torch.equal(y[~keep], b[None].expand(int((~keep).sum()), d))


@pytest.mark.parametrize("T", [3, 4, 5, 8, 9])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("C1", [8, 6], ids=["cin8-vec", "cin6-scalar"])
def test_conv_frontend_f32(T, causal, C1):
    """Conv2d + GELU twice and the `out` Linear (extractors.py:110-113; CausalConv2d's left padding) against oracle.conv_subsample; F = 8"""
    O = _ops()
    from huggingface_asr_amd import shapes
    B, Fq, C2, d = 2, 8, 12, 16
    cfg = dict(conv_kernel=[3, 3], conv_stride=[2, 2], conv_padding=[1, 1], is_causal=causal)
    F2 = shapes.conv_freq_out(Fq, cfg["conv_kernel"], cfg["conv_stride"], cfg["conv_padding"])
    cw = "" if causal else ".conv"
    p = "wav2vec2.feature_extractor."
    gen = torch.Generator().manual_seed(100 * T + C1 + int(causal))
    sd = {f"{p}conv.0.0{cw}.weight": _rand(gen, C1, 1, 3, 3, scale=0.5), f"{p}conv.0.0{cw}.bias": _rand(gen, C1, scale=0.2),
          f"{p}conv.1.0{cw}.weight": _rand(gen, C2, C1, 3, 3, scale=0.3), f"{p}conv.1.0{cw}.bias": _rand(gen, C2, scale=0.2),
          p + "out.weight": _rand(gen, d, C2 * F2, scale=0.3), p + "out.bias": _rand(gen, d, scale=0.2)}
    x = _rand(gen, B, T, Fq, scale=2.0)
    ref = lambda dt: R.conv_subsample({k: v.to(dt) for k, v in sd.items()}, cfg, x.to(dt))
    with torch.no_grad():
        want, noise = ref(F64), float((ref(F32).double() - ref(F64)).abs().max())
    f = lambda k: sd[p + k].float()
    w1 = f(f"conv.0.0{cw}.weight").reshape(C1, 9).to(DEV)
    w2 = f(f"conv.1.0{cw}.weight").permute(0, 2, 3, 1).reshape(C2, 9 * C1).contiguous().to(DEV)          # (Cout, (kh, kw, cin)): packing._enc_map
    wo = f("out.weight").reshape(d, C2, F2).permute(0, 2, 1).reshape(d, F2 * C2).contiguous().to(DEV)     # (c, f) -> (f, c) columns
    a1 = O.conv2d_first_gelu(x.float().to(DEV), w1, f(f"conv.0.0{cw}.bias").to(DEV), causal=causal)
    a2 = O.conv2d_cl(a1, w2, f(f"conv.1.0{cw}.bias").to(DEV), causal=causal)
    T2 = a2.shape[1]
    got = O.gemm(a2.reshape(B * T2, F2 * C2), wo, f("out.bias").to(DEV)).reshape(B, T2, d).cpu()
    assert got.shape == want.shape
    _report("conv_frontend", f"T{T}-causal{int(causal)}-cin{C1}", got, want, noise)
