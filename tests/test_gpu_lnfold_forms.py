"""The LayerNorm-folded GEMM pair and the row kernel that feeds it (huggingface_asr_amd/csrc/gemm_8p.hip, gemm_bf16.hip, norm.hip) at tile, partial and row edges.  Cases, references and
the derivation of every bound live in tests/lnfold_cases.py; tests/test_lnfold_cases_cpu.py checks them — and that each defect named below lands >= 10 x outside
its bound — without a GPU.

Every output is a view inside a NaN-filled buffer (8 guard rows below it, columns beside it, ld > width; a statistics buffer: the floats of each 32-float record
beyond the pairs the launch owns); whatever is not output must still be NaN afterwards.  Every launch is repeated into the re-poisoned buffers and must give the
same bits.

  A. producer, mi_gemm_resid_stats_f32_v, variants 0 / 42 / 43 (128 x 128 kernel) and 40 (256 x 256): integer operands, `torch.equal` for C, C2 = bf16(C) and every
     (sum, sumsq) pair; in place (resid is C) against out of place; 42 and 43 bit for bit on float inputs; refusals leave everything untouched.
  B. consumer, mi_gemm_lnfold_bf16, against float64 of the folded formula from the fp32 statistics it is given, within the bound `lnfold_cases.folded_reference` derives
     (prints `RATIO <case> <observed / bound>`, asserts <= 1): every row with its own mean and scale, every npart (1, 4, 8, 12, 16), two to eight K tiles, one-row
     and 255-row tiles; rows of zeros with statistics (0, 0) give bf16(act(cbias)) exactly; NaN in every float of the statistics buffer that the kernel has no
     business with gives the same bits as zeros there.
  C. row kernel, mi_layernorm_fold / mi_layernorm_chain, all four `ln_chain_kernel<NV>` instantiations with partly valid lanes, against float64 layer_norm.
  D. producer -> consumer chained at the smallest shape, on both producer tiles.

Measured on the MI355X (observed / bound, the largest over each group's cases; every test prints its own with pytest -s):
  B  act none  1.000 (rounded; <= 1) in every case, 0.988 - 0.999 in row M - 1: nearly all of the bound is the bf16 half ulp, which the stored value's rounding
               error reaches among 65 000+ outputs — the derived fp32 part is three orders of magnitude smaller, and a defect moves an output by >= 100 bounds
     act gelu  0.826 - 0.904 (row M - 1: 0.826 - 0.880)
     rows of zeros: exact;  NaN against zeros in the unowned statistics floats: the same bits at every npart (before the prologue's weights became selects,
     npart = 1 gave whole rows of NaN)
  A  float inputs, C against float64: 0.001 - 0.002 of (K + 4) U (|A| |W|^T + |b| + |resid|); everything else in A is exact
  C  fp32 rows against 2e-5 + 1e-5 |want|: 0.004 - 0.013 (5e-5 behind a second norm: 0.004 - 0.011); bf16 rows against 2e-2 + 1.2e-2 |want|: 0.099 - 0.225;
     statistics against d 2**-24 sum|y| / d 2**-23 sum y^2: <= 0.004, and 0.162 - 0.194 at d = 4
  D  0.898 (128 tile, 8 pairs, gelu), 1.000 (256 tile, 4 pairs, none)
"""
import pytest
import torch

import lnfold_cases as L

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
GUARD = 8
JUNK = 5.0                   # what operand buffers hold beside the operand (exact in bf16; a product with it changes every sum)
NAN = float("nan")
REFUSED = "unsupported configuration|invalid argument"


def _mods():
    from huggingface_asr_amd import _lib, ops
    return _lib, ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def place(x, cols, off, dtype):
    """x (R, W) float64 as a device view buf[:, off:off+W] of a (R, cols) buffer whose other columns hold JUNK"""
    R, W = x.shape
    buf = torch.full((R, cols), JUNK, device=DEV, dtype=dtype)
    v = buf[:, off:off + W]
    v.copy_(x.to(dtype))
    return v


class Guarded:
    """an output view big[:rows, off:off+width] of a NaN-filled (rows + GUARD, ld) buffer"""

    def __init__(self, rows, width, ld, off, dtype):
        self.big = torch.full((rows + GUARD, ld), NAN, device=DEV, dtype=dtype)
        self.view = self.big[:rows, off:off + width]
        self.own = torch.zeros_like(self.big, dtype=torch.bool)
        self.own[:rows, off:off + width] = True

    def poison(self):
        self.big.fill_(NAN)

    def assert_clean_outside(self, what):
        touched = ~torch.isnan(self.big) & ~self.own
        assert not bool(touched.any()), f"{what}: {int(touched.sum())} cells outside the output were written, first at {touched.nonzero()[0].tolist()}"

    def assert_untouched(self, what):
        assert bool(torch.isnan(self.big).all()), f"{what}: a refused launch wrote"


def stats_buffer(M, npairs):
    """(M + GUARD, 32) fp32, NaN; the view is floats 0 .. 2 npairs - 1 of rows 0 .. M - 1"""
    return Guarded(M, 2 * npairs, L.LN_STATS_STRIDE, 0, F32)


def first_bad(got, want):
    bad = got != want
    if not bool(bad.any()):
        return ""
    i = tuple(bad.nonzero()[0].tolist())
    return f"{int(bad.sum())} / {bad.numel()} wrong, first at {list(i)}: got {float(got[i])}, want {float(want[i])}"


# ----------------------------------------------------------------------------------------------------------------- A. producer
class Producer:
    """operands and guarded outputs of one producer shape; run(variant, alpha, inplace) poisons, launches and returns clones of (C, C2, pairs (M, npairs, 2))"""

    def __init__(self, kernel, M, N, K, inputs, ldc2_pad=16):
        a, w, b, res = inputs
        self.M, self.N, self.K, self.kernel, self.res = M, N, K, kernel, res
        self.npairs = max(1, N // L.block_width(kernel))
        self.a, self.w = place(a, K + 16, 8, BF), place(w, K + 24, 16, BF)
        self.b = b.to(DEV, F32)
        self.r = place(res, N + 8, 4, F32)                                   # its own stride: ldr != ldc
        self.C, self.C2, self.st = Guarded(M, N, N + 16, 8, F32), Guarded(M, N, N + ldc2_pad, 8, BF), stats_buffer(M, min(self.npairs, 16))
        assert self.C.view.data_ptr() % 16 == 0 and self.r.data_ptr() % 16 == 0 and self.C2.view.data_ptr() % 8 == 0 and self.a.data_ptr() % 16 == 0 and self.w.data_ptr() % 16 == 0

    def launch(self, variant, alpha, inplace=False):
        _lib, _ = _mods()
        for g in (self.C, self.C2, self.st):
            g.poison()
        r = self.r
        if inplace:
            self.C.view.copy_(self.res.to(F32))
            r = self.C.view
        rc = _lib.lib().mi_gemm_resid_stats_f32_v(self.a.data_ptr(), self.a.stride(0), self.w.data_ptr(), self.w.stride(0), self.b.data_ptr(), self.C.view.data_ptr(), self.C.view.stride(0),
                                                  r.data_ptr(), r.stride(0), float(alpha), self.C2.view.data_ptr(), self.C2.view.stride(0), self.st.big.data_ptr(),
                                                  self.M, self.N, self.K, int(variant), _stream())
        _lib.check(rc, "mi_gemm_resid_stats_f32_v")

    def run(self, variant, alpha, inplace=False, what=""):
        self.launch(variant, alpha, inplace)
        for g in (self.C, self.C2, self.st):
            g.assert_clean_outside(what)
        return self.C.view.clone(), self.C2.view.clone(), self.st.view.clone().reshape(self.M, self.npairs, 2)


def _assert_producer_exact(c, got, what):
    C, C2, pairs = got
    wantC, want_pairs = L.producer_reference(c)
    wantC, want_pairs = wantC.to(DEV, F32), want_pairs.to(DEV, F32)
    assert torch.equal(C, wantC), f"{what} C: {first_bad(C, wantC)}"
    assert torch.equal(C2, wantC.to(BF)), f"{what} C2: {first_bad(C2.float(), wantC.to(BF).float())}"
    assert torch.equal(pairs, want_pairs), f"{what} statistics (row, slot, sum | sumsq): {first_bad(pairs, want_pairs)}"


@pytest.mark.parametrize("c", L.PRODUCER_CASES, ids=lambda c: c.id)
def test_producer_is_exact(c):
    P = Producer(c.kernel, c.M, c.N, c.K, L.producer_inputs(c))
    inplace = c.resid == "inplace"
    first = P.run(c.variant, c.alpha, inplace, c.id)
    _assert_producer_exact(c, first, c.id)
    again = P.run(c.variant, c.alpha, inplace, c.id)
    assert all(torch.equal(x, y) for x, y in zip(first, again)), f"{c.id}: not the same bits launch to launch"
    if inplace:                                                              # resid is C, as the layer calls it: the bits of the out-of-place call
        sep = P.run(c.variant, c.alpha, False, c.id)
        assert all(torch.equal(x, y) for x, y in zip(first, sep)), f"{c.id}: in place differs from out of place"


@pytest.mark.parametrize("M,N,K", L.PRODUCER_SAME_BITS, ids=lambda v: str(v))
def test_producer_pipelined_and_loader_rings_give_the_same_bits_on_float_inputs(M, N, K):
    """variants 42 and 43: "same ring, K order and MFMA shape" (gemm_8p.hip).  Against float64: |C - want| <= (K + 4) U (|A| |W|^T + |b| + |resid|), any fp32
    order of K products plus the epilogue's roundings; the pairs against float64 sums of the stored C within lnfold_cases.row_sum_bounds (32 terms)."""
    a, w, b, res = L.producer_float_inputs(M, N, K)
    P = Producer(128, M, N, K, (a, w, b, res))
    outs = {}
    for v in (42, 43, 0):
        outs[v] = P.run(v, 0.5, False, f"v{v}")
        again = P.run(v, 0.5, False, f"v{v}")
        assert all(torch.equal(x, y) for x, y in zip(outs[v], again)), f"variant {v}: not the same bits launch to launch"
    for x, y, name in zip(outs[42], outs[43], ("C", "C2", "statistics")):
        assert torch.equal(x, y), f"42 vs 43, {name}: {first_bad(x.float(), y.float())}"
    C, C2, pairs = (t.cpu() for t in outs[42])
    want = res + 0.5 * (a @ w.t() + b)
    tol = (K + 4) * L.U * (a.abs() @ w.abs().t() + b.abs() + res.abs())
    ratio = float(((C.double() - want).abs() / tol).max())
    print(f"RATIO producer-float-{M}x{N}x{K} {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(C2, C.to(BF))
    for s in range(N // 32):
        sm, dsm, sq, dsq = L.row_sum_bounds(C[:, 32 * s:32 * s + 32].double())
        assert bool(((pairs[:, s, 0].double() - sm).abs() <= dsm).all()) and bool(((pairs[:, s, 1].double() - sq).abs() <= dsq).all()), s


@pytest.mark.parametrize("r", L.PRODUCER_REFUSALS, ids=lambda r: r[0])
def test_producer_refusals_leave_everything_untouched(r):
    what, kernel, variant, N, K, pad2 = r
    M = 129
    g = torch.Generator().manual_seed(1)
    P = Producer(kernel, M, N, K, (torch.ones(M, K).double(), torch.ones(N, K).double(), torch.ones(N).double(), torch.randn(M, N, generator=g).double()), ldc2_pad=pad2)
    with pytest.raises(RuntimeError, match=REFUSED):
        P.launch(variant, 1.0)
    torch.cuda.synchronize()
    for g_ in (P.C, P.C2, P.st):
        g_.assert_untouched(what)


# ----------------------------------------------------------------------------------------------------------------- B. consumer
def lnfold(xb, wf, colsum, cbias, stats_ptr, npart, out, act, M, N, K):
    _lib, _ = _mods()
    rc = _lib.lib().mi_gemm_lnfold_bf16(xb.data_ptr(), xb.stride(0), wf.data_ptr(), wf.stride(0), _p(colsum), _p(cbias), stats_ptr, int(npart), L.EPS,
                                        out.data_ptr(), out.stride(0), int(act), M, N, K, _stream())
    _lib.check(rc, "mi_gemm_lnfold_bf16")


def _check_consumer(c, zero_rows=False):
    i, ref = L.consumer_inputs(c, zero_rows), L.consumer_reference(c, zero_rows)
    xb, wf = place(i.x, c.K + 16, 8, BF), place(i.wf, c.K + 24, 16, BF)              # lda > K
    cs, cb = i.colsum.to(DEV, F32), i.cbias.to(DEV, F32)
    out, st = Guarded(c.M, c.N, c.N + 16, 8, BF), stats_buffer(c.M, c.npart)         # ldc > N
    assert out.view.data_ptr() % 16 == 0 and cs.data_ptr() % 16 == 0 and cb.data_ptr() % 16 == 0
    act = {"none": 0, "gelu": 1}[c.act]

    def launch(pad):
        out.poison()
        st.big.fill_(pad)                                                            # the floats beyond the row's pairs, and the guard rows
        st.view.copy_(i.stats.reshape(c.M, -1).to(F32))
        lnfold(xb, wf, cs, cb, st.big.data_ptr(), c.npart, out.view, act, c.M, c.N, c.K)
        out.assert_clean_outside(c.id)
        return out.view.clone()

    got = launch(NAN)
    assert not bool(torch.isnan(got).any()), f"{c.id}: {int(torch.isnan(got).any(1).sum())} output rows are NaN with NaN in statistics floats the kernel does not own"
    ratio = (got.double().cpu() - ref.want).abs() / ref.bound
    worst = float(ratio.max())
    print(f"RATIO {c.id}{'-zero-rows' if zero_rows else ''} {worst:.3f} (row M - 1: {float(ratio[c.M - 1].max()):.3f})")
    assert worst <= 1.0, (c.id, worst, (ratio > 1).nonzero()[0].tolist())
    assert float(ratio[c.M - 1].max()) <= 1.0                                        # the rows of the last tile beyond M read row M - 1's record: it must not feel them
    assert torch.equal(launch(NAN), got), f"{c.id}: not the same bits launch to launch"
    assert torch.equal(launch(0.0), got), f"{c.id}: the bits depend on statistics floats beyond the row's {c.npart} pairs"
    return got, cb, wf


@pytest.mark.parametrize("c", L.CONSUMER_CASES, ids=lambda c: c.id)
def test_consumer_against_the_folded_formula(c):
    _check_consumer(c)


@pytest.mark.parametrize("c", [L.CONSUMER_CASES[0], L.CONSUMER_CASES[1], L.CONSUMER_CASES[2]], ids=lambda c: c.id)
def test_consumer_rows_of_zeros_give_the_bias(c):
    """masked frames: x = 0, statistics (0, 0) -> acc = 0, mean = 0, r = eps^-1/2 and the output is bf16(act(cbias)) exactly.  act = gelu: `act` is the library's
    GELU (common.hpp gelu_erf, a fit), so the exact expectation is the plain 256 x 256 GEMM's GELU epilogue on the same fp32 argument — A = 0, bias = cbias — and
    float64 erf-GELU(cbias) within the bound like every other row."""
    _, ops = _mods()
    got, cb, wf = _check_consumer(c, zero_rows=True)
    rows = got[1::4]
    assert rows.shape[0] >= 64
    if c.act == "none":
        want = cb.to(BF)
    else:
        want = ops.gemm(torch.zeros((256, c.K), device=DEV, dtype=BF), wf, cb, act="gelu", variant=40)[0]
    assert torch.equal(rows, want[None, :].expand_as(rows)), first_bad(rows.float(), want[None, :].expand_as(rows).float())


@pytest.mark.parametrize("r", L.CONSUMER_REFUSALS, ids=lambda r: r[0])
def test_consumer_refusals_leave_the_output_untouched(r):
    what, N, K, npart, act, mis = r
    M = 129
    xb, wf = torch.ones((M, K + 16), device=DEV, dtype=BF)[:, 8:8 + K], torch.ones((N, K + 24), device=DEV, dtype=BF)[:, 16:16 + K]
    cs = torch.ones(N + 4, device=DEV)[2:2 + N] if mis == "colsum" else torch.ones(N, device=DEV)
    cb = torch.ones(N, device=DEV)
    st = torch.ones((M + GUARD) * 32 + 4, device=DEV)
    st_ptr = st.data_ptr() + (8 if mis == "stats" else 0)
    assert (cs.data_ptr() % 16 == 8) == (mis == "colsum") and (st_ptr % 16 == 8) == (mis == "stats")
    out = Guarded(M, N, N + 16, 8, BF)
    with pytest.raises(RuntimeError, match=REFUSED):
        lnfold(xb, wf, cs, cb, st_ptr, npart, out.view, act, M, N, K)
    torch.cuda.synchronize()
    out.assert_untouched(what)


# ----------------------------------------------------------------------------------------------------------------- C. row kernel
class RowBuffers:
    def __init__(self, d, M):
        self.d, self.M = d, M
        self.y, self.yb, self.st = Guarded(M, d, d + 8, 4, F32), Guarded(M, d, d + 8, 4, BF), stats_buffer(M, 1)
        self.a32, self.ab, self.bb = Guarded(M, d, d + 12, 8, F32), Guarded(M, d, d + 16, 8, BF), Guarded(M, d, d + 8, 4, BF)
        self.all = (self.y, self.yb, self.st, self.a32, self.ab, self.bb)

    def poison(self):
        for g in self.all:
            g.poison()

    def assert_clean_outside(self, what, used):
        for g in self.all:
            if g in used:
                g.assert_clean_outside(what)
            else:
                g.assert_untouched(what)


def fold(x, lens, T, g, b, y, yb, st_ptr, M, d, ldx=None):
    _lib, _ = _mods()
    rc = _lib.lib().mi_layernorm_fold(x.data_ptr(), x.stride(0) if ldx is None else ldx, _p(lens), T, _p(g), _p(b), L.EPS, _p(y), y.stride(0) if y is not None else 0,
                                      _p(yb), yb.stride(0) if yb is not None else 0, st_ptr, M, d, _stream())
    _lib.check(rc, "mi_layernorm_fold")


def _assert_row_stats(pair, y, what):
    """pair (M, 2) fp32 against float64 sums of the kernel's own stored fp32 y: d 2**-24 sum|y| for the sum, d 2**-23 sum y^2 for the sum of squares"""
    sm, dsm, sq, dsq = L.row_sum_bounds(y.double().cpu())
    p = pair.double().cpu()
    rs, rq = (p[:, 0] - sm).abs() / dsm.clamp_min(1e-300), (p[:, 1] - sq).abs() / dsq.clamp_min(1e-300)
    zero = dsq == 0                                                                  # a row of zeros: (0, 0) exactly
    assert bool((p[zero] == 0).all()), what
    worst = max(float(rs[~zero].max()) if bool((~zero).any()) else 0.0, float(rq[~zero].max()) if bool((~zero).any()) else 0.0)
    assert worst <= 1.0, (what, worst)
    return worst


@pytest.mark.parametrize("d,M", L.ROW_CASES, ids=lambda v: str(v))
def test_layernorm_fold(d, M):
    x64, gs, bs = L.row_inputs(d, M)
    T, lens, masked = L.row_mask(M)
    x = place(x64, d + 4, 0, F32)                                                    # ldx > d
    g, b, lens_d = gs[0].to(DEV, F32), bs[0].to(DEV, F32), lens.to(DEV)
    R = RowBuffers(d, M)
    worst_y = worst_s = 0.0
    for with_g in (True, False):
        for with_len in (False, True):
            what = f"fold d={d} M={M} g1={with_g} lengths={with_len}"
            xm = x64.clone()
            if with_len:
                xm[masked] = 0.0
            want = L.ln64(xm, gs[0], bs[0]) if with_g else xm

            def launch(inplace):
                R.poison()
                src = x
                if inplace:
                    R.y.view.copy_(x)
                    src = R.y.view
                fold(src, lens_d if with_len else None, T, g if with_g else None, b if with_g else None, R.y.view, R.yb.view, R.st.big.data_ptr(), M, d)
                R.assert_clean_outside(what, (R.y, R.yb, R.st))                      # of a record: floats 0 and 1 only; nothing in the guard rows
                return R.y.view.clone(), R.yb.view.clone(), R.st.view.clone()

            y, yb, st = launch(False)
            if with_g:
                torch.testing.assert_close(y.double().cpu(), want, atol=2e-5, rtol=1e-5, msg=lambda m: f"{what}: {m}")
                worst_y = max(worst_y, float(((y.double().cpu() - want).abs() / (2e-5 + 1e-5 * want.abs())).max()))
            else:
                assert torch.equal(y.double().cpu(), want), what                     # mask only: x, or exactly 0
            assert torch.equal(yb, y.to(BF)), what
            if with_len:                                                             # masked rows: exactly beta with g1, exactly 0 (and statistics (0, 0)) without
                ym = y[masked.to(DEV)]
                assert torch.equal(ym, (b if with_g else torch.zeros_like(b))[None, :].expand_as(ym)), what
            worst_s = max(worst_s, _assert_row_stats(st, y, what))
            for again in (launch(False), launch(True)):                              # repeated; and y32 is x
                assert all(torch.equal(p, q) for p, q in zip((y, yb, st), again)), f"{what}: not the same bits (repeat / in place)"
    print(f"RATIO fold-{d}x{M} y {worst_y:.3f} statistics {worst_s:.3f}")


@pytest.mark.parametrize("d,M", L.ROW_CASES, ids=lambda v: str(v))
def test_layernorm_chain(d, M):
    _, ops = _mods()
    x64, gs, bs = L.row_inputs(d, M)
    T, lens, masked = L.row_mask(M)
    x = place(x64, d + 4, 0, F32)
    gd, bd = [t.to(DEV, F32) for t in gs], [t.to(DEV, F32) for t in bs]
    lens_d = lens.to(DEV)
    R = RowBuffers(d, M)
    worst = {"y": 0.0, "a32": 0.0, "bf16": 0.0}
    for with_len in (False, True):
        for with_g in (True, False):
            what = f"chain d={d} M={M} g1={with_g} lengths={with_len}"
            xm = x64.clone()
            if with_len:
                xm[masked] = 0.0
            y64 = L.ln64(xm, gs[0], bs[0]) if with_g else xm
            a64, b64 = L.ln64(y64, gs[1], bs[1]), L.ln64(y64, gs[2], bs[2])

            def launch(inplace):
                R.poison()
                src = x
                if inplace:
                    R.y.view.copy_(x)
                    src = R.y.view
                ops.layernorm_chain(src, lengths=lens_d if with_len else None, T=T, ln1=(gd[0], bd[0]) if with_g else None, eps1=L.EPS, store_y=R.y.view,
                                    lna=(gd[1], bd[1]), eps2=L.EPS, outa=R.ab.view, outa32=R.a32.view, lnb=(gd[2], bd[2]), outb=R.bb.view)
                R.assert_clean_outside(what, (R.y, R.a32, R.ab, R.bb))
                return R.y.view.clone(), R.a32.view.clone(), R.ab.view.clone(), R.bb.view.clone()

            y, a32, ab, bb = launch(False)
            if with_g:
                torch.testing.assert_close(y.double().cpu(), y64, atol=2e-5, rtol=1e-5, msg=lambda m: f"{what} y: {m}")
                worst["y"] = max(worst["y"], float(((y.double().cpu() - y64).abs() / (2e-5 + 1e-5 * y64.abs())).max()))
            else:
                assert torch.equal(y.double().cpu(), y64), what
            atol2 = 5e-5 if with_g else 2e-5                                         # the project's figures: 2e-5 for one norm, 5e-5 behind a second
            torch.testing.assert_close(a32.double().cpu(), a64, atol=atol2, rtol=1e-5, msg=lambda m: f"{what} outa32: {m}")
            worst["a32"] = max(worst["a32"], float(((a32.double().cpu() - a64).abs() / (atol2 + 1e-5 * a64.abs())).max()))
            assert torch.equal(ab, a32.to(BF)), what
            for got, w64 in ((ab, a64), (bb, b64)):
                r = float(((got.double().cpu() - w64).abs() / (L.BF16_ATOL + L.BF16_RTOL * w64.abs())).max())
                worst["bf16"] = max(worst["bf16"], r)
                assert r <= 1.0, (what, r)
            if with_len:
                mk = masked.to(DEV)
                ym = y[mk]
                assert torch.equal(ym, (bd[0] if with_g else torch.zeros_like(bd[0]))[None, :].expand_as(ym)), what
                if not with_g:                                                       # LN of a row of zeros is its beta, exactly
                    assert torch.equal(a32[mk], bd[1][None, :].expand_as(a32[mk])) and torch.equal(bb[mk], bd[2].to(BF)[None, :].expand_as(bb[mk])), what
            for again in (launch(False), launch(True)):
                assert all(torch.equal(p, q) for p, q in zip((y, a32, ab, bb), again)), f"{what}: not the same bits (repeat / in place)"
    print(f"RATIO chain-{d}x{M} y {worst['y']:.3f} outa32 {worst['a32']:.3f} bf16 {worst['bf16']:.3f}")


@pytest.mark.parametrize("entry,what", [(e, w) for e in ("fold", "chain") for w in L.ROW_REFUSALS if (e, w) != ("chain", "null-yb")])       # (the chain has no yb)
def test_row_kernel_refusals_leave_the_outputs_untouched(entry, what):
    _, ops = _mods()
    M = 5
    d = {"d2052": 2052, "d6": 6}.get(what, 256)
    ldx = d + 2 if what == "ldx" else d + 4
    x = torch.ones((M, ldx), device=DEV)[:, :d]
    g, b = torch.ones(2052, device=DEV), torch.zeros(2052, device=DEV)
    R = RowBuffers(d + (d % 4), M)
    y, yb = R.y.big[:M, 4:4 + d], R.yb.big[:M, 4:4 + d]
    with pytest.raises(RuntimeError, match=REFUSED):
        if entry == "fold":
            fold(x, None, 1, g, b, y, None if what == "null-yb" else yb, R.st.big.data_ptr(), M, d)
        else:
            ops.layernorm_chain(x, ln1=(g, b), store_y=y, lna=(g, b), outa=R.ab.big[:M, 8:8 + d], outa32=R.a32.big[:M, 8:8 + d])
    torch.cuda.synchronize()
    R.assert_clean_outside(f"{entry} {what}", ())


# ----------------------------------------------------------------------------------------------------------------- D. chained
@pytest.mark.parametrize("kernel,variant,npart,act", [(128, 0, 8, "gelu"), (256, 40, 4, "none")], ids=["tile128-p8", "wide-p4"])
def test_producer_feeds_consumer(kernel, variant, npart, act):
    """producer (257, 256, 384) -> its C2 and its statistics buffer, NaN beyond the pairs it wrote, straight into the consumer (N = 256, K = 256); compared as in B,
    with the reference built from what the producer left (exact by A)"""
    pc = L.ProdCase("chain", kernel, variant, 257, 256, 384, 0.5, "sep")
    P = Producer(kernel, pc.M, pc.N, pc.K, L.producer_inputs(pc))
    first = P.run(variant, pc.alpha, False, "chain producer")
    _assert_producer_exact(pc, first, "chain producer")
    assert P.npairs == npart
    M, K, N = pc.M, pc.N, 256
    g = torch.Generator().manual_seed(11)
    wf64 = torch.randint(-2, 3, (N, K), generator=g).double()
    cb64 = torch.randn(N, generator=g).float().double()
    xb64, st64 = first[1].double().cpu(), first[2].double().cpu()
    # exactness of acc and of the sums of the partials: multiples of 0.5 (0.25) whose magnitudes sum below 2**24 lsb
    assert bool((xb64 * 2 == (xb64 * 2).round()).all()) and float((xb64.abs() @ wf64.abs().t()).max()) * 2 < L.EXACT_LIMIT
    assert float(st64[..., 0].abs().sum(1).max()) * 2 < L.EXACT_LIMIT and float(st64[..., 1].sum(1).max()) * 4 < L.EXACT_LIMIT
    colsum = wf64.sum(1)
    ref = L.folded_reference(xb64 @ wf64.t(), colsum, cb64, st64, K, L.EPS, act)
    wf, cs, cb = place(wf64, K + 24, 16, BF), colsum.to(DEV, F32), cb64.to(DEV, F32)
    out = Guarded(M, N, N + 16, 8, BF)

    def launch():
        out.poison()
        lnfold(P.C2.view, wf, cs, cb, P.st.big.data_ptr(), npart, out.view, {"none": 0, "gelu": 1}[act], M, N, K)
        out.assert_clean_outside("chain consumer")
        return out.view.clone()

    got = launch()
    ratio = float(((got.double().cpu() - ref.want).abs() / ref.bound).max())
    print(f"RATIO chain-{kernel}-p{npart}-{act} {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(launch(), got)
