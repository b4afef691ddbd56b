"""Cases, inputs, float64 references and bounds for the LayerNorm-folded GEMM pair (huggingface_asr_amd/csrc/gemm_8p.hip, gemm_bf16.hip, norm.hip; algebra in gemm_args.hpp),
shared by tests/test_lnfold_cases_cpu.py (no GPU) and tests/test_gpu_lnfold_forms.py.  Nothing here touches a GPU.

A. PRODUCER, mi_gemm_resid_stats_f32_v: C fp32 = resid + alpha (A W^T + b), C2 = bf16(C), and one (sum, sumsq) pair per row and column block — 32 columns on the
   128 x 128 kernel (variants 0, 42, 43), 64 columns on the 256 x 256 one (variant 40); pair s of a row lives in floats 2s, 2s + 1 of its 32-float record and
   covers columns [s bw, (s + 1) bw).  Inputs are integers: A in {-2..2}, W in {-1, 0, 1}, bias in {-4..4}, residual in {-8..8}, alpha in {1, 0.5}.  Every value
   the kernel forms is then a multiple of lsb (1, or 0.5 with alpha = 0.5; squares: lsb^2) and every partial sum, in ANY order, is bounded by the sum of the
   terms' magnitudes: while that stays below 2**24 lsb the fp32 result is exact whatever the K loop, the MFMA shape or the lane reduction do.
   `producer_exactness` computes those sums for a case and tests/test_lnfold_cases_cpu.py asserts them; the GPU test is `torch.equal`.

B. CONSUMER, mi_gemm_lnfold_bf16: out bf16 = act(r acc - r mean colsum + cbias), acc = xb Wf^T, with (mean, r) from the row's `npart` partial pairs.
   xb is integer valued: row m is scale_m (off_m + lvl + e), off_m = m % 7 - 3, scale_m = 2**(m % 3), e uniform in {-2..2}, and lvl in {-1, 0, 1} changes from one
   statistics block to the next ((block + m) % 3 - 1), so every row has its own mean and scale and neighbouring blocks of a row carry different sums.
   |x| <= 24, Wf in {-2..2}: acc, colsum and all statistics are exact integers in fp32 (`consumer_exactness`).  The K columns are split into `npart` blocks as
   torch.tensor_split does — equal blocks wherever npart divides K, sizes one apart otherwise (K = 128 with 12 partials has no equal split; the kernel only sums
   the pairs, their widths are the producer's business).
   The reference is float64 of the formula AS THE KERNEL WRITES IT, from the fp32 statistics it is given (`folded_reference`), and the bound is derived from
   that formula's roundings (`folded_bound`), never from what the kernel returned.

C. ROW KERNEL, mi_layernorm_fold / mi_layernorm_chain (`ln_chain_kernel<1 | 2 | 4 | 8>`): d and M below; float64 layer_norm of the masked input.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from gemm_cases import BF16_ATOL, BF16_RTOL, GELU_FIT_ATOL, GELU_FIT_RTOL, gelu_erf64  # noqa: F401  (re-exported: one definition of the project's figures)

U = 2.0 ** -24                    # fp32 unit roundoff: a correctly rounded operation is off by at most U |result|
EXACT_LIMIT = 2 ** 24             # integers (in units of the lsb) below this are exact in fp32
LN_STATS_STRIDE = 32              # floats per row of a statistics buffer (gemm_args.hpp)
EPS = 1e-5
GELU_MAX_SLOPE = 1.13             # max |d erf-GELU / dx| = 1.1290 (at x = sqrt 2)

# ----------------------------------------------------------------------------------------------------------------------------------------
# A. producer
ProdCase = namedtuple("ProdCase", "id kernel variant M N K alpha resid")         # kernel: 128 | 256;  resid: "sep" (its own buffer, ldr != ldc) | "inplace" (resid is C)

P128_M, P128_N, P128_K = (1, 127, 129, 257), (128, 256, 384, 512), (384, 512, 640)
P256_M, P256_N, P256_K = (1, 255, 257, 513), (256, 512, 768, 1024), (128, 192, 320)
P128_VARIANTS, P256_VARIANTS = (0, 42, 43), (40,)


def block_width(kernel):
    return 32 if kernel == 128 else 64


def _pcase(kernel, variant, M, N, K, alpha, resid="sep"):
    return ProdCase(f"p{kernel}-v{variant}-{M}x{N}x{K}-a{alpha}" + ("" if resid == "sep" else f"-{resid}"), kernel, variant, M, N, K, alpha, resid)


def _build_producer():
    cases = []
    # not the cross product: every M, N and K of a form's list once, the same four shapes for each variant of the 128 kernel
    for v in P128_VARIANTS:
        for i, (M, N, K) in enumerate(((1, 128, 384), (127, 256, 512), (129, 384, 640), (257, 512, 384))):
            cases.append(_pcase(128, v, M, N, K, (0.5, 1.0)[i % 2]))
    for i, (M, N, K) in enumerate(((1, 256, 128), (255, 512, 192), (257, 768, 320), (513, 1024, 128))):
        cases.append(_pcase(256, 40, M, N, K, (1.0, 0.5)[i % 2]))
    # in place (resid is C, as the layer calls it), once per form, at a shape with more than one tile in both directions
    for v in P128_VARIANTS:
        cases.append(_pcase(128, v, 129, 256, 384, 0.5, "inplace"))
    cases.append(_pcase(256, 40, 257, 512, 192, 0.5, "inplace"))
    assert len({c.id for c in cases}) == len(cases) and len(cases) <= 40
    return tuple(cases)


PRODUCER_CASES = _build_producer()
# float inputs: the pipelined (42) and the loader / consumer (43) ring claim the same K order and MFMA shape, hence the same bits
PRODUCER_SAME_BITS = ((129, 256, 384), (257, 512, 640))


def producer_supported(kernel, M, N, K, ldc2=8):
    """gemm_8p128_supported / gemm_8p_supported as far as the producer's shape goes (operands aligned)"""
    if ldc2 % 4:
        return False
    if kernel == 128:
        return N % 128 == 0 and N <= 512 and K % 128 == 0 and K >= 320
    return N % 256 == 0 and N <= 1024 and K % 64 == 0 and K >= 128


# (what, kernel, variant, N, K, ldc2 padding): each must raise and leave C, C2 and the statistics untouched
PRODUCER_REFUSALS = (("N640", 128, 0, 640, 384, 16), ("K448", 128, 0, 256, 448, 16), ("K256", 128, 0, 256, 256, 16), ("N1280-wide", 256, 40, 1280, 192, 16),
                     ("N384-wide", 256, 40, 384, 192, 16), ("variant7", 128, 7, 256, 384, 16), ("ldc2-128", 128, 0, 256, 384, 18), ("ldc2-wide", 256, 40, 256, 192, 18))


@functools.lru_cache(maxsize=4)
def _producer_operands(M, N, K):
    g = torch.Generator().manual_seed(77 + 1000003 * M + 1009 * N + K)
    a = torch.randint(-2, 3, (M, K), generator=g).double()
    w = torch.randint(-1, 2, (N, K), generator=g).double()
    b = torch.randint(-4, 5, (N,), generator=g).double()
    res = torch.randint(-8, 9, (M, N), generator=g).double()
    return a, w, b, res


def producer_inputs(c):
    """(A, W, bias, resid) float64, integer valued"""
    return _producer_operands(c.M, c.N, c.K)


def block_stats(x, bw):
    """x (M, N) float64 -> (M, N // bw, 2): the (sum, sum of squares) of every bw-column block"""
    xs = x.reshape(x.shape[0], x.shape[1] // bw, bw)
    return torch.stack((xs.sum(-1), (xs * xs).sum(-1)), -1)


def producer_reference(c):
    """(C float64 (M, N), pairs float64 (M, N // bw, 2)) — exact, see producer_exactness"""
    a, w, b, res = producer_inputs(c)
    C = res + c.alpha * (a @ w.t() + b)
    return C, block_stats(C, block_width(c.kernel))


def producer_exactness(c):
    """The largest sum of |terms|, in units of the least significant bit, of (the K sums, the block sums, the block sums of squares): each must stay below
    2**24 for every fp32 summation order to give the same, exactly representable value.  Also checks that every value IS a multiple of its lsb."""
    a, w, b, res = producer_inputs(c)
    lsb = 0.5 if c.alpha == 0.5 else 1.0
    C, _ = producer_reference(c)
    assert bool((C / lsb == (C / lsb).round()).all()) and bool((C.float().double() == C).all())
    k_sum = float((a.abs() @ w.abs().t() + b.abs()).max())                       # acc + b: integers
    st = block_stats(C.abs(), block_width(c.kernel))
    return k_sum, float(st[..., 0].max()) / lsb, float(st[..., 1].max()) / (lsb * lsb)


@functools.lru_cache(maxsize=2)
def producer_float_inputs(M, N, K):
    g = torch.Generator().manual_seed(5 + 1000003 * M + 1009 * N + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).double()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).double()
    b = (0.1 * torch.randn(N, generator=g)).float().double()
    res = (2.0 * torch.randn(M, N, generator=g) + 0.7).float().double()
    return a, w, b, res


# ----------------------------------------------------------------------------------------------------------------------------------------
# B. consumer
ConsCase = namedtuple("ConsCase", "id M N K npart act")
C_M, C_N, C_K, C_NPART, C_ACT = (1, 255, 257, 513), (256, 512), (128, 192, 320, 512), (1, 4, 8, 12, 16), ("none", "gelu")


def _ccase(M, N, K, npart, act):
    return ConsCase(f"c-{M}x{N}x{K}-p{npart}-{act}", M, N, K, npart, act)


def _build_consumer():
    cases = []
    # every npart at M = 257 (a second row tile of ONE row) with K = 128 (two K tiles: the main loop body runs zero times) ...
    for i, npart in enumerate(C_NPART):
        cases.append(_ccase(257, C_N[i % 2], 128, npart, C_ACT[i % 2]))
    # ... and every npart at each other K (three tiles: the loop body once; five; eight) and M, walking the lists so that each (K, npart) pair occurs
    for ki, K in enumerate(C_K[1:]):
        for pi, npart in enumerate(C_NPART):
            cases.append(_ccase((1, 255, 513, 257)[(ki + pi) % 4], C_N[(ki + pi + 1) % 2], K, npart, C_ACT[(ki + pi + 1) % 2]))
    # the remaining M at K = 128, both activations on one shape, and both N with each activation at M = 513 (three row tiles)
    cases += [_ccase(1, 256, 128, 1, "gelu"), _ccase(255, 512, 128, 16, "none"), _ccase(513, 256, 128, 8, "gelu"), _ccase(513, 512, 128, 4, "none"),
              _ccase(257, 512, 128, 1, "gelu"), _ccase(257, 256, 128, 4, "none")]
    assert len({c.id for c in cases}) == len(cases) and len(cases) <= 40
    return tuple(cases)


CONSUMER_CASES = _build_consumer()
# (what, N, K, npart, act code, misaligned operand): each must raise and leave the output untouched
CONSUMER_REFUSALS = (("N384", 384, 128, 4, 0, None), ("K64", 256, 64, 4, 0, None), ("K200", 256, 200, 4, 0, None), ("npart0", 256, 128, 0, 0, None),
                     ("npart2", 256, 128, 2, 0, None), ("npart5", 256, 128, 5, 0, None), ("npart20", 256, 128, 20, 0, None), ("act2", 256, 128, 4, 2, None),
                     ("colsum8B", 256, 128, 4, 0, "colsum"), ("stats8B", 256, 128, 4, 0, "stats"))


def consumer_supported(N, K, npart, act):
    """mi_gemm_lnfold_bf16 / gemm_8p_supported as far as shape, partial count and activation go"""
    return N % 256 == 0 and K % 64 == 0 and K >= 128 and (npart == 1 or (4 <= npart <= 16 and npart % 4 == 0)) and act in (0, 1)


def block_index(K, npart):
    """(K,) long: the statistics block of every column — torch.tensor_split's sections"""
    idx = torch.empty(K, dtype=torch.long)
    for j, part in enumerate(torch.tensor_split(torch.arange(K), npart)):
        idx[part] = j
    return idx


def partial_stats(x, npart):
    """x (M, K) float64 -> (M, npart, 2): exact (sum, sumsq) of every column block"""
    parts = torch.tensor_split(x, npart, dim=1)
    return torch.stack([torch.stack((p.sum(1), (p * p).sum(1)), -1) for p in parts], 1)


ConsInputs = namedtuple("ConsInputs", "x wf colsum cbias stats acc")


@functools.lru_cache(maxsize=4)
def _consumer_inputs(M, N, K, npart, zero_rows):
    g = torch.Generator().manual_seed(19 + 1000003 * M + 1009 * N + 31 * K + npart)
    r = torch.arange(M)
    off, scale = ((r % 7) - 3).double(), (2.0 ** (r % 3)).double()
    lvl = ((block_index(K, npart)[None, :] + r[:, None]) % 3 - 1).double()
    e = torch.randint(-2, 3, (M, K), generator=g).double()
    x = scale[:, None] * (off[:, None] + lvl + e)
    if zero_rows:
        x[1::4] = 0.0                                     # masked frames: x = 0, statistics (0, 0)
    wf = torch.randint(-2, 3, (N, K), generator=g).double()
    cbias = torch.randn(N, generator=g).float().double()
    return ConsInputs(x, wf, wf.sum(1), cbias, partial_stats(x, npart), x @ wf.t())


def consumer_inputs(c, zero_rows=False) -> ConsInputs:
    """x = xb (M, K), Wf (N, K), colsum (N), cbias (N), stats (M, npart, 2), acc = x Wf^T (M, N): float64, everything but cbias integer valued"""
    return _consumer_inputs(c.M, c.N, c.K, c.npart, bool(zero_rows))


def consumer_exactness(c):
    """largest sum of |terms| of (acc, a row's sum, a row's sum of squares): below 2**24 each, so xb Wf^T and the statistics are exact in fp32 in any order;
    and the largest |mean| / sigma of a row, which the bound's cancellation term depends on (must be <= 4)"""
    i = consumer_inputs(c)
    assert bool((i.x.to(torch.bfloat16).double() == i.x).all()) and bool((i.wf.to(torch.bfloat16).double() == i.wf).all())
    mean = i.x.mean(1)
    sigma = i.x.var(1, unbiased=False).sqrt()
    return float((i.x.abs() @ i.wf.abs().t()).max()), float(i.x.abs().sum(1).max()), float((i.x * i.x).sum(1).max()), float((mean.abs() / sigma).max())


def act64(name):
    return {"none": lambda t: t, "gelu": gelu_erf64}[name]


Folded = namedtuple("Folded", "want bound pre")


def bf16_half_ulp(a):
    """half a bf16 ulp (8 significant bits) at magnitude a >= 0: 2**(floor(log2 a) - 8); the smallest normal's below 2**-126"""
    _, e = torch.frexp(a.clamp_min(2.0 ** -126))          # a = m 2**e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(a), e - 9)


def folded_reference(acc, colsum, cbias, stats, K, eps, act):
    """float64 of the kernel's formula (gemm_8p.hip, LNF prologue and epilogue), from the statistics it is given:
        mean = (sum of the sums) / K,  var = max((sum of the sumsqs) / K - mean^2, 0),  r = (var + eps)^-1/2,  want = act(r acc - r mean colsum + cbias)
    and the bound on |kernel's bf16 output - want| from that formula's fp32 roundings.  The sums of the partials and acc are exact for these inputs
    (consumer_exactness).  With U = 2**-24 and correctly rounded operations off by <= U relative (the divisions and rsqrtf are given 2 U: rsqrtf is the hardware's
    1-ulp v_rsq_f32):
        mean^ = mean (1 + 2U),  q^ = q (1 + 2U)  (q = sumsq / K);
        var^ = fl(q^ - fl(mean^ mean^)): |var^ - var| <= 2U q + (4U + U) mean^2 + U var =: dv      (the cancellation: dv / var <= U (2 (1 + c^2) + 5 c^2 + 1), c = |mean| / sigma
                                                                                                       <= 4: 115 U; contracting the product into an fma only removes a term);
        r^ = rsqrtf(fl(var^ + eps)): relative error rho = dv / (2 (var + eps)) + U / 2 + 2U;
        t^ = fl(r^ mean^): relative rho + 3U;
        z^ = fmaf(r^, acc, -fl(t^ colsum)): |z^ - z| <= rho |r acc| + (rho + 4U) |t colsum| + U |z|;
        pre^ = fl(z^ + cbias): + U |pre|.
    E = that sum, times (1 + 2**-10) for every second-order term.  act = gelu: the fit's documented error (common.hpp gelu_erf; GELU_FIT_ATOL + GELU_FIT_RTOL |want|) and
    the slope of GELU (<= 1.13) on E.  Then the bf16 rounding of the stored value: half an ulp at |want| + E.
    Returns (want, bound, pre)."""
    sm, sq = stats[..., 0].sum(1), stats[..., 1].sum(1)
    mean, q = sm / K, sq / K
    var = (q - mean * mean).clamp_min(0.0)
    r = (var + eps) ** -0.5
    t = r * mean
    ra, tc = r[:, None] * acc, t[:, None] * colsum[None, :]
    z = ra - tc
    pre = z + cbias[None, :]
    want = act64(act)(pre)
    dv = U * (2 * q + 5 * mean * mean + var)
    rho = (dv / (2 * (var + eps)) + 2.5 * U)[:, None]
    E = (rho * ra.abs() + (rho + 4 * U) * tc.abs() + U * z.abs() + U * pre.abs()) * (1 + 2.0 ** -10)
    if act == "gelu":
        E = GELU_MAX_SLOPE * E + GELU_FIT_ATOL + GELU_FIT_RTOL * want.abs()
    return Folded(want, E + bf16_half_ulp(want.abs() + E), pre)


def consumer_reference(c, zero_rows=False) -> Folded:
    i = consumer_inputs(c, zero_rows)
    return folded_reference(i.acc, i.colsum, i.cbias, i.stats.float().double(), c.K, EPS, c.act)


def unfolded_reference(c):
    """float64 layer_norm -> linear on the same operands: what the folded formula stands for (gamma is folded into Wf, cbias = W beta + b)"""
    i = consumer_inputs(c)
    return act64(c.act)(F.linear(F.layer_norm(i.x, (c.K,), None, None, EPS), i.wf, i.cbias))


def wrong_references(c):
    """{name: want} of the defects the consumer test must catch: (a) row m + 1's statistics (the last row takes row 0's; M = 1 has no other row), (b) one slot
    dropped and (c) one slot counted twice, for EVERY slot, (d) colsum moved by one wave column block (64) and, with two column tiles, by one tile (256)"""
    i = consumer_inputs(c)
    st = i.stats.float().double()
    ref = lambda s, cs: folded_reference(i.acc, cs, i.cbias, s, c.K, EPS, c.act).want
    out = {}
    if c.M > 1:
        out["a-next-row"] = ref(st.roll(-1, 0), i.colsum)
    for j in range(c.npart):
        drop = st.clone(); drop[:, j] = 0.0
        twice = st.clone(); twice[:, j] *= 2.0
        out[f"b-drop{j}"] = ref(drop, i.colsum)
        out[f"c-twice{j}"] = ref(twice, i.colsum)
    out["d-colsum64"] = ref(st, i.colsum.roll(64))
    if c.N > 256:
        out["d-colsum256"] = ref(st, i.colsum.roll(256))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------------
# C. the row kernel
ROW_D = (4, 252, 256, 260, 768, 1028, 1280, 2048)        # NV = 1 (4, 252, 256), 2 (260), 4 (768), 8 (1028, 1280, 2048); d / 4 % 64 != 0: 4, 252, 260, 1028
ROW_M = (1, 5, 9)                                        # four rows per block: a partly filled block, alone and behind full ones
ROW_CASES = tuple((d, M) for d in ROW_D for M in ROW_M)
ROW_REFUSALS = ("d2052", "d6", "ldx", "null-yb")


def row_nv(d):
    """the ln_chain_kernel<NV> instantiation norm.hip launches for d"""
    nv = -(-(d // 4) // 64)
    return 1 if nv <= 1 else (2 if nv <= 2 else (4 if nv <= 4 else 8))


def row_mask(M):
    """(T, lengths (B,), masked (M,) bool) of the `lengths` form: row = b T + t is masked when t >= lengths[b]"""
    T, lens = {1: (1, [0]), 5: (3, [2, 1]), 9: (3, [3, 1, 0])}[M]
    masked = torch.tensor([(m % T) >= lens[m // T] for m in range(M)])
    return T, torch.tensor(lens, dtype=torch.int32), masked


@functools.lru_cache(maxsize=4)
def row_inputs(d, M):
    """x (M, d) fp32-valued float64 with a row mean of about 0.5, and three (gamma, beta) pairs"""
    g = torch.Generator().manual_seed(3 + 4099 * d + M)
    x = (2.0 * torch.randn(M, d, generator=g) + 0.5).float().double()
    gs = [(1.0 + 0.1 * torch.randn(d, generator=g)).float().double() for _ in range(3)]
    bs = [(0.1 * torch.randn(d, generator=g)).float().double() for _ in range(3)]
    return x, gs, bs


def ln64(x, g, b, eps=EPS):
    return F.layer_norm(x, (x.shape[-1],), g, b, eps)


def row_sum_bounds(y):
    """y (M, d) float64 (the kernel's stored fp32 rows) -> (sum, its bound, sumsq, its bound): any fp32 summation order of d terms is within (d - 1) U sum|terms| of the
    exact sum; the squares carry one more rounding each"""
    d = y.shape[1]
    return y.sum(1), d * U * y.abs().sum(1), (y * y).sum(1), d * 2 * U * (y * y).sum(1)
