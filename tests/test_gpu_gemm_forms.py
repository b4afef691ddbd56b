"""Every forward form of the dense GEMM dispatch (huggingface_asr_amd/csrc/gemm_bf16.hip `launch`, gemm_glds.hip `gemm_glds_launch`, gemm_8p.hip `gemm_8p_launch` / `gemm_8p128_launch`)
at the smallest sizes at which its tile masks, its K loop and its ring can go wrong, forced through `variant` and compared bit for bit.  The cases, the references
and the reasoning that makes zero tolerance legitimate live in tests/gemm_cases.py; tests/test_gemm_cases_cpu.py checks them without a GPU.

  a. exact: integer operands (every fp32 accumulation order gives the same representable value), `torch.equal` against the float64-derived expectation.  The
     output is a view inside a NaN-filled buffer: the columns beside it and 8 guard rows below it must still be NaN afterwards.  One documented exception: the fp32
     epilogue of the 256 x 256 kernel stores 16 B at a time and may touch a row's padding up to the next multiple of 4 columns (gemm_8p_supported), so for that
     form the cells from (N + 3) & ~3 on are checked.
  b. the form under test really ran: a forced variant falls through SILENTLY to another kernel when its form does not support the shape, so every launch is
     recorded by the library's profiling slots and must be exactly one launch of the expected family (gemm_args.hpp PF_*).  The three LDS-DMA tiles share PF_GLDS
     and the three rings of the 128 x 128 kernel share PF_8P128: WHICH of them ran cannot be observed this way and rests on the variant's documented meaning and
     on the restated dispatch conditions of tests/gemm_cases.py (`route`), which tests/test_gemm_cases_cpu.py pins.
  c. activations on float inputs against float64 erf-GELU / tanh-GELU of the float64 linear result.  bf16 out: the bounds of tests/test_gpu_ops.py
     assert_close_bf16 (atol 2e-2, rtol 1.2e-2).  fp32 out, erf-GELU: 2.6e-5 + 5e-4 |want| — the documented error of the fit (huggingface_asr_amd/csrc/common.hpp gelu_erf) — plus
     ACC_NOISE; tanh-GELU (`gelu_tanh`, evaluated in fp32 with __expf), for which no documented figure exists: |x| 2**-19 + 2**-22 |want| + ACC_NOISE, a worst-case
     bound derived at `_new_gelu_bound` from the formula's roundings (observed error / bound on the MI355X: 0.12 - 0.17; the erf form's sits at 0.80).
     ACC_NOISE = 2 x the largest |fp32-out linear result (act="none") - float64 linear result| measured over these same cases on the MI355X, i.e. what the
     accumulation order and the fp32 roundings of the K loop contribute before the activation (both GELUs have slope <= 1.13, inside the factor 2).
     Measured: see ACC_NOISE_MEASURED below; every test prints its own figure (`NOISE <case> <value>`, pytest -s) and asserts it stays below ACC_NOISE.
     Every launch of (c) and of (d) is repeated into the re-poisoned buffer and must give the same bits: between them these cover all nine forms on float inputs
     (the fp32 epilogue of the 256 x 256 kernel admits no activation and is repeated in (d)); tests/test_gemm_cases_cpu.py asserts that coverage.
  d. cross-form bit identity only where the source claims it: the 32 x 64, 128 x 64 and 128 x 128 LDS-DMA forms ("same accumulation order, hence the same bits",
     gemm_glds.hip), and the 256 x 256 against the 128 x 128 phase kernel at K % 128 == 0 ("Same K order and MFMA shape").  The pipelined against the
     loader / consumer ring is tests/test_gpu_ops.py's; variant 47 and the default ring at odd K-tile counts carry no such claim and are checked against the
     references only (whether they happen to give the pipelined ring's bits was not examined).
  e. the implicit-im2col loader: `ops.conv2d_cl(..., variant=v)` on integer inputs against float64 `F.conv2d`, on the generic kernel (Cin 8, 72), the 128 x 128
     LDS-DMA form (Cin 64) and the 256 kernel (variant 40, Cin 64 / 128, Cout 256); M = B T' F' ragged against both tile heights, symmetric and causal padding,
     and a time-only (3, 1) kernel; one float case per form with the fused GELU.
  f. refusals: lda % 8, ldw % 8, K % 8 raise and leave the output untouched; an A base pointer that is 8-B but not 16-B aligned runs — exactly — on the generic
     kernel whatever fast path the variant asks for (these are the `-a4` cases of the exact table).
"""
import ctypes as C

import pytest
import torch

import gemm_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32
GUARD = 8                    # rows below the output that no launch may touch
JUNK = 5.0                   # what the parts of an operand buffer hold that no kernel may use (exact in bf16; a product with it changes every sum)

# Largest |fp32-out linear result - float64 linear result| over ACT_CASES' shapes, measured on the MI355X with this file's test_accumulation_noise (K <= 448,
# |x| <= ~6): 1.19e-6 (generic, K = 136: 6.8e-7; LDS-DMA forms, K = 192 / 320: 7.6e-7 - 9.5e-7; 128 x 128 phase kernel, K = 384: 1.02e-6, K = 448: 1.19e-6), i.e. a few fp32 ulps of the largest outputs.
ACC_NOISE_MEASURED = 1.2e-6
ACC_NOISE = 2 * ACC_NOISE_MEASURED


def _mods():
    from huggingface_asr_amd import _lib, ops
    return _lib, ops


# ----------------------------------------------------------------------------------------------------------------- which kernel family ran
@pytest.fixture(scope="module")
def prof():
    """the library's profiling slots (huggingface_asr_amd/csrc/diag.hip mi_profile_*): created once per process — MI_ERR_ARG means an earlier user already made them, which is fine —
    enabled for this module, disabled at teardown"""
    _lib, _ = _mods()
    L = _lib.lib()
    rc = L.mi_profile_create(64)
    assert rc in (0, _lib.ERR_ARG), rc
    L.mi_profile_reset()
    L.mi_profile_enable(1)
    yield L
    L.mi_profile_enable(0)
    L.mi_profile_reset()


def families(L):
    """{family: launches} recorded since the last reset (after a device synchronisation: the summary reads the slots' events)"""
    torch.cuda.synchronize()
    out = {}
    ms, fl, n = C.c_double(), C.c_double(), C.c_int()
    for fam in range(G.PF_COUNT):
        assert L.mi_profile_summary_family(fam, C.byref(ms), C.byref(fl), C.byref(n)) == 0
        if n.value:
            out[fam] = n.value
    assert sum(out.values()) == L.mi_profile_count(), "a dense launch took no profiling slot"
    return out


def assert_one_launch(L, family, what):
    got = families(L)
    assert got == {family: 1}, f"{what}: expected one launch of {G.FAMILY_NAME[family]}, recorded {({G.FAMILY_NAME[k]: v for k, v in got.items()})}"


# ----------------------------------------------------------------------------------------------------------------- operands and launches
def place(x, cols, off, dtype):
    """x (R, W) float64 as a device view buf[:, off:off+W] of a (R, cols) buffer whose other columns hold JUNK"""
    R, W = x.shape
    buf = torch.full((R, cols), JUNK, device=DEV, dtype=dtype)
    v = buf[:, off:off + W]
    v.copy_(x.to(dtype))
    return v


class Out:
    """the output view of a case inside a NaN-filled (M + GUARD, ldc) buffer"""

    def __init__(self, c):
        lo = G.layout(c)
        self.c, self.lo = c, lo
        self.dtype = F32 if G.EPILOGUES[c.epi][0] else BF
        self.big = torch.full((c.M + GUARD, lo.ldc), float("nan"), device=DEV, dtype=self.dtype)
        self.view = self.big[:c.M, lo.c_off:lo.c_off + lo.ncols]

    def poison(self):
        self.big.fill_(float("nan"))

    def logical(self):
        """(M, N) values and the mask of the buffer's cells that belong to the output"""
        c, lo = self.c, self.lo
        own = torch.zeros_like(self.big, dtype=torch.bool)
        if G.EPILOGUES[c.epi][4]:
            T, Tp, B = G.remap_of(c.N)
            own[:c.M, lo.c_off:lo.c_off + lo.ncols].unflatten(1, (B, Tp))[:, :, :T] = True          # (splitting a dimension is always a view)
            return self.view.unflatten(1, (B, Tp))[:, :, :T].reshape(c.M, c.N), own
        own[:c.M, lo.c_off:lo.c_off + c.N] = True
        return self.view, own

    def assert_untouched_outside(self, own, what):
        c, lo = self.c, self.lo
        free = own.clone()
        if c.form == "p256_f32":                         # 16-B stores may touch the row's padding up to the next multiple of 4 columns
            free[:c.M, lo.c_off + c.N:lo.c_off + ((c.N + 3) & ~3)] = True
        touched = ~torch.isnan(self.big) & ~free
        assert not bool(touched.any()), f"{what}: {int(touched.sum())} cells outside the output were written, first at {touched.nonzero()[0].tolist()}"


def operands(c, inputs):
    a, w, bias, resid, alpha = inputs
    lo, L = G.layout(c), G.launch(c)
    ad = place(a, lo.lda, lo.a_off, BF)
    wd = place(w, lo.ldw, lo.w_off, BF)
    bd = None if bias is None else bias.to(DEV, F32)
    rd = None if resid is None else place(resid, lo.ldr, lo.r_off, F32)
    # the alignments gemm_cases.launch assumed are the ones the tensors really have
    assert (ad.data_ptr() % 16 == 0) == L.a16 and (wd.data_ptr() % 16 == 0) == L.w16 and ad.stride(0) == L.lda and wd.stride(0) == L.ldw
    assert rd is None or ((rd.data_ptr() % 16 == 0) == L.r16 and rd.stride(0) == L.ldr)
    assert bd is None or bd.data_ptr() % 16 == 0
    return ad, wd, bd, rd, alpha


def run(ops, c, opnds, out):
    ad, wd, bd, rd, alpha = opnds
    remap = G.EPILOGUES[c.epi][4]
    assert (out.view.data_ptr() % 16 == 0) == G.launch(c).c16 and out.view.stride(0) == G.launch(c).ldc
    ops.gemm(ad, wd, bd, out=out.view, act=c.act, resid=rd, alpha=alpha, bias_per_row=G.EPILOGUES[c.epi][1] == 2,
             col_remap=G.remap_of(c.N)[:2] if remap else None, variant=c.variant)


# ----------------------------------------------------------------------------------------------------------------- a + b (+ f's aligned-to-8-B cases)
@pytest.mark.parametrize("c", G.EXACT_CASES, ids=lambda c: c.id)
def test_exact(c, prof):
    _, ops = _mods()
    opnds = operands(c, G.exact_inputs(c))
    out = Out(c)
    prof.mi_profile_reset()
    run(ops, c, opnds, out)
    assert_one_launch(prof, G.route(G.launch(c))[1], c.id)
    got, own = out.logical()
    want = G.expected(c).to(DEV)
    bad = got != want                                   # (NaN left in an output cell compares unequal too)
    assert not bool(bad.any()), (f"{c.id}: {int(bad.sum())} / {bad.numel()} wrong, first at {bad.nonzero()[0].tolist()}: "
                                 f"got {float(got[tuple(bad.nonzero()[0])])}, want {float(want[tuple(bad.nonzero()[0])])}")
    assert torch.equal(got, want)
    out.assert_untouched_outside(own, c.id)


# ----------------------------------------------------------------------------------------------------------------- c
def _new_gelu_bound(x, want):
    """fp32 evaluation of gelu_tanh (huggingface_asr_amd/csrc/common.hpp): r = 0.5 x t, t = 2 - 2 / (e + 1), e = __expf(2u), u = 0.79788 (x + 0.044715 x^3).
    u carries <= 4 roundings (2**-22 relative); __expf(z) = exp2(z log2 e) has a relative error of about (|z| + 2) 2**-24 (the rounded product in the exponent, then one
    ulp), tripled here: de <= 3 (|2u| + 2) 2**-24 + |2u| 2**-22.  dt = 2 e / (e + 1)^2 de <= de / 2 (and -> 0 where |u| is large), plus two roundings of values <= 2:
    2**-22.  So |dr| <= 0.5 |x| (de / 2 + 2**-22) + 2**-23 |r|.  With |x| <= 8 (asserted), |2u| <= 50: de <= 2**-17.3 and |dr| <= |x| 2**-19 + 2**-23 |r|; the returned bound doubles the last term (2**-22 |r|) for the final product's own two roundings."""
    assert float(x.abs().max()) <= 8.0
    return x.abs() * 2.0 ** -19 + 2.0 ** -22 * want.abs()


@pytest.mark.parametrize("c", G.ACT_CASES, ids=lambda c: c.id)
def test_activation_epilogues(c, prof):
    _, ops = _mods()
    opnds = operands(c, G.float_inputs(c))
    out = Out(c)
    prof.mi_profile_reset()
    run(ops, c, opnds, out)
    assert_one_launch(prof, G.route(G.launch(c))[1], c.id)
    got = out.view.clone()
    lin, want = G.float_linear(c).to(DEV), G.float_reference(c).to(DEV)
    err = (got.double() - want).abs()
    if out.dtype == BF:
        tol = G.BF16_ATOL + G.BF16_RTOL * want.abs()
    else:
        # the accumulation noise of this very form and shape, before the activation
        c0 = c._replace(act="none")
        out0 = Out(c0)
        run(ops, c0, opnds, out0)
        noise = float((out0.view.double() - lin).abs().max())
        print(f"NOISE {c.id} {noise:.3g}")
        assert noise <= ACC_NOISE, (noise, ACC_NOISE)
        tol = (G.GELU_FIT_ATOL + G.GELU_FIT_RTOL * want.abs() if c.act == "gelu" else _new_gelu_bound(lin, want)) + ACC_NOISE
    ratio = float((err / tol).max())
    print(f"RATIO {c.id} {ratio:.3f} (max err {float(err.max()):.3g})")
    assert ratio <= 1.0, (c.id, ratio, float(err.max()))
    _, own = out.logical()
    out.assert_untouched_outside(own, c.id)
    out.poison()
    run(ops, c, opnds, out)
    assert torch.equal(out.view, got), f"{c.id}: not the same bits launch to launch"


def test_accumulation_noise():
    """the measurement behind ACC_NOISE (prints `NOISE-MAX`): fp32-out linear results of every float shape and form against float64"""
    _, ops = _mods()
    worst = 0.0
    for c in G.ACT_CASES:
        if not G.EPILOGUES[c.epi][0] or c.act != "gelu":
            continue
        c0 = c._replace(act="none")
        out = Out(c0)
        run(ops, c0, operands(c0, G.float_inputs(c0)), out)
        worst = max(worst, float((out.view.double() - G.float_linear(c0).to(DEV)).abs().max()))
    print(f"NOISE-MAX {worst:.3g}")
    assert worst <= ACC_NOISE


# ----------------------------------------------------------------------------------------------------------------- d
@pytest.mark.parametrize("group", G.SAME_BITS, ids=lambda g: "=".join(c.form for c in g) + "-" + g[0].id.split("-", 2)[2])
def test_forms_with_a_claimed_common_k_order_give_the_same_bits(group, prof):
    _, ops = _mods()
    opnds = operands(group[0], G.float_inputs(group[0]))
    outs = []
    for c in group:
        out = Out(c)
        prof.mi_profile_reset()
        run(ops, c, opnds, out)
        assert_one_launch(prof, G.route(G.launch(c))[1], c.id)
        first = out.view.clone()
        out.poison()
        run(ops, c, opnds, out)
        assert torch.equal(out.view, first), f"{c.id}: not the same bits launch to launch"
        _, own = out.logical()
        out.assert_untouched_outside(own, c.id)
        outs.append(first)
    want = G.float_reference(group[0]).to(DEV)
    tol = G.BF16_ATOL + G.BF16_RTOL * want.abs()           # (a sanity bound only: the forms are not all wrong together)
    assert bool(((outs[0].double() - want).abs() <= tol).all())
    for c, o in zip(group[1:], outs[1:]):
        assert torch.equal(outs[0], o), f"{group[0].id} vs {c.id}: {int((outs[0] != o).sum())} values differ"


# ----------------------------------------------------------------------------------------------------------------- e
def _conv(ops, c, exact, act):
    x, w, b = G.conv_inputs(c, exact)
    return ops.conv2d_cl(x.to(DEV, BF), w.to(DEV, BF), b.to(DEV, F32), K=c.K, stride=2, pad=c.pad, causal=c.causal, act=act, variant=c.variant)


@pytest.mark.parametrize("c", G.CONV_CASES, ids=lambda c: c.id)
def test_implicit_gemm_conv_exact(c, prof):
    _, ops = _mods()
    prof.mi_profile_reset()
    got = _conv(ops, c, True, "none")
    assert_one_launch(prof, c.family, c.id)
    want = G.conv_reference(c).to(BF).to(DEV)
    assert got.shape == want.shape
    bad = got != want
    assert not bool(bad.any()), f"{c.id}: {int(bad.sum())} / {bad.numel()} wrong, first at (b, t, f, c) = {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("c", [c for c in G.CONV_CASES if (c.B, c.causal, c.K) == (2, False, (3, 3))], ids=lambda c: c.id)
def test_implicit_gemm_conv_gelu(c, prof):
    _, ops = _mods()
    prof.mi_profile_reset()
    got = _conv(ops, c, False, "gelu")
    assert_one_launch(prof, c.family, c.id)
    want = G.gelu_erf64(G.conv_reference(c, False)).to(DEV)
    err = (got.double() - want).abs()
    ratio = float((err / (G.BF16_ATOL + G.BF16_RTOL * want.abs())).max())
    print(f"RATIO {c.id} {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(got, _conv(ops, c, False, "gelu"))


# ----------------------------------------------------------------------------------------------------------------- f
@pytest.mark.parametrize("variant", [0, 40, 42, 32])
@pytest.mark.parametrize("what", ["lda", "ldw", "K"])
def test_refusals_leave_the_output_untouched(what, variant, prof):
    """gemm_bf16.hip `launch`: lda % 8, ldw % 8 and K % 8 are argument errors before any kernel is chosen"""
    _, ops = _mods()
    M, N, K = 129, 128, 384
    a = torch.ones((M, K + 16), device=DEV, dtype=BF)
    w = torch.ones((N, K + 16), device=DEV, dtype=BF)
    out = torch.full((M + GUARD, N), float("nan"), device=DEV, dtype=F32)
    if what == "lda":
        av, wv = torch.ones((M, K + 12), device=DEV, dtype=BF)[:, :K], w[:, :K]
    elif what == "ldw":
        av, wv = a[:, :K], torch.ones((N, K + 4), device=DEV, dtype=BF)[:, :K]
    else:
        av, wv = a[:, :K - 4], w[:, :K - 4]
    assert G.refused(G.Launch(variant, M, N, av.shape[1], av.stride(0), wv.stride(0), N, 0, True, 0, False, 0, 0, True, True, True, True, True))
    prof.mi_profile_reset()
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.gemm(av, wv, None, out=out[:M], variant=variant)
    assert families(prof) == {}
    assert bool(torch.isnan(out).all())
