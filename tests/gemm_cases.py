"""Cases and exact references for the dense GEMM family (huggingface_asr_amd/csrc/gemm_bf16.hip, gemm_glds.hip, gemm_8p.hip), shared by tests/test_gemm_cases_cpu.py (no GPU) and
tests/test_gpu_gemm_forms.py.  Nothing here touches a GPU.

Exact inputs.  A and W are integers uniform in {-3..3}, bias and residual in {-8..8}, alpha in {1, 0.5}.  With K <= 4096 every partial sum of a row's products is an
integer of magnitude <= 9 * 4096 < 2**24, so EVERY fp32 accumulation order (any K-tile order, any MFMA shape, any split) gives the same, exactly representable value;
bias, alpha = 0.5 and the residual keep it a multiple of 0.5 below 2**24.  The reference is float64 `resid + alpha * (A @ W.T + bias)`; the fp32-out expectation is that
value bit for bit and the bf16-out one is its round-to-nearest-even cast, which is what the kernels' `f2bf` does (huggingface_asr_amd/csrc/common.hpp).  A test on these inputs cannot pass
with a missing, duplicated or stale k-slice and its tolerance is zero.  tests/test_gemm_cases_cpu.py checks the bound and the order independence on the CPU.

Float inputs (activation epilogues, cross-form bit identity): A = bf16(N(0,1)), W = bf16(N(0,1) / sqrt(K)), as in tests/test_gpu_ops.py.

Forms.  `variant` (mi_gemm_bf16_v; gemm_glds.hip `gemm_glds_launch`) lets a test reach any kernel at a small size.  The names used here:
    generic      gemm_bf16_kernel (register staged): whatever gemm_glds_supported refuses — K % 64 != 0, or an operand that is not 16-B aligned
    glds32       LDS-DMA 32 x 64 tiles, two waves, four-stage ring (variant 32)
    glds128x64   LDS-DMA 128 x 64 tiles, two-stage ring (variant 41 = "this file's kernels only"; the shape must also fail the 32 x 64 rule and have
                 <= 48 K steps per CU, see `route`)
    glds128      LDS-DMA 128 x 128 tiles, two-stage ring, persistent grid with the next tile's first K tile prefetched (variant 30; 31 = one block per tile)
    p256_bf16    256 x 256 phase kernel, bf16 out (variant 40)            p256_f32   the same kernel's fp32 epilogue (ragged N allowed)
    p128_pipe    128 x 128 phase kernel, register-pipelined ring (variant 42, and 40 where the 256 kernel does not take the shape; even number of K tiles)
    p128_loader  its loader / consumer ring (variant 43; even number of K tiles)
    p128_ring4   its default four-deep ring: every odd number of K tiles whatever the variant, and variant 47 at any K

THE WEAK POINT.  `glds_supported`, `p256_supported`, `p128_supported` and `route` below are Python copies of gemm_glds_supported, gemm_8p_supported,
gemm_8p128_supported and gemm_glds_launch's selection.  Each case's form is DERIVED with them and the GPU tests check the launched kernel FAMILY (profiling slots),
but the three LDS-DMA tiles and the three 128 x 128 rings share one family each: that a case reaches the sub-form it names rests on these copies.  If the C++
predicates or the dispatch change, change the copies with them (tests/test_gemm_cases_cpu.py pins the conditions they restate).
"""
from __future__ import annotations

import functools
import itertools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

# profiling families (huggingface_asr_amd/csrc/gemm_args.hpp)
PF_8P, PF_8P_GELU, PF_8P_CONV, PF_8P_OUT32, PF_8P128, PF_GLDS, PF_GENERIC = 0, 1, 2, 3, 4, 5, 6
PF_COUNT = 9
FAMILY_NAME = {0: "PF_8P", 1: "PF_8P_GELU", 2: "PF_8P_CONV", 3: "PF_8P_OUT32", 4: "PF_8P128", 5: "PF_GLDS", 6: "PF_GENERIC", 7: "PF_8P_AMAX", 8: "PF_8P_CE"}

FORMS = ("generic", "glds32", "glds128x64", "glds128", "p256_bf16", "p256_f32", "p128_pipe", "p128_loader", "p128_ring4")
TILE_M = {"generic": 128, "glds32": 32, "glds128x64": 128, "glds128": 128, "p256_bf16": 256, "p256_f32": 256, "p128_pipe": 128, "p128_loader": 128, "p128_ring4": 128}

# the K edges of every form (the issue's table): where its K loop, ring depth or support minimum can go wrong
K_EDGES = {
    "generic": (8, 72, 136),                    # less than one 16-B chunk row; one tile + one chunk; two tiles + ONE valid 16-B chunk in the last
    "glds32": (64, 128, 192, 256, 320),         # one K tile in a four-stage ring; two; three (= tiles in flight); exactly the ring depth; one more
    "glds128x64": (64, 128, 192),               # one tile in a two-stage ring; the ring depth; one more
    "glds128": (64, 128, 192),
    "p256_bf16": (128, 192, 320),               # the support minimum (only the two peeled tail tiles); odd count, one steady-state tile; five tiles, three steady-state
    "p256_f32": (128, 192, 320),
    "p128_pipe": (384, 512),                    # even tile counts >= 320: six tiles, eight tiles
    "p128_loader": (384, 512),
    "p128_ring4": (320, 384, 448, 512),         # the minimum (five tiles: odd, so this ring whatever the variant); 47 at an even count; seven tiles; 47 again
}
K_BIG = 4096                                    # one case per form at the exactness bound
M_EDGES = {32: (1, 31, 32, 33, 127, 257), 128: (1, 33, 127, 128, 129, 257), 256: (1, 129, 255, 256, 257)}

# epilogue name -> (out_f32, bias mode (0 none / 1 column / 2 row), residual, alpha, column remap)
EPILOGUES = {
    "f32": (True, 0, False, 1.0, False),
    "f32_bias": (True, 1, False, 1.0, False),
    "f32_resid": (True, 1, True, 0.5, False),            # fp32 out + residual + alpha (+ column bias)
    "f32_resid1": (True, 0, True, 1.0, False),
    "bf16": (False, 0, False, 1.0, False),
    "bf16_bias": (False, 1, False, 1.0, False),
    "bf16_rowbias": (False, 2, False, 1.0, False),       # bias_per_row=True
    "f32_remap": (True, 2, False, 1.0, True),            # the V^T projection's form: per-row bias + col_remap=(T, Tp)
    "bf16_remap": (False, 2, False, 1.0, True),
}
# what each form's *_supported admits (gemm_8p_supported / gemm_8p128_supported: no col_T, no bias_mode 2; residual with fp32 out only — the 256 kernel: whole tiles only)
FORM_EPILOGUES = {
    "generic": tuple(EPILOGUES), "glds32": tuple(EPILOGUES), "glds128x64": tuple(EPILOGUES), "glds128": tuple(EPILOGUES),
    "p256_bf16": ("bf16", "bf16_bias"),
    "p256_f32": ("f32", "f32_bias", "f32_resid", "f32_resid1"),
    "p128_pipe": ("f32", "f32_bias", "f32_resid", "f32_resid1", "bf16", "bf16_bias"),
    "p128_loader": ("f32", "f32_bias", "f32_resid", "f32_resid1", "bf16", "bf16_bias"),
    "p128_ring4": ("f32", "f32_bias", "f32_resid", "f32_resid1", "bf16", "bf16_bias"),
}
FORM_N = {
    "generic": (72, 130, 300), "glds32": (72, 130, 300), "glds128": (72, 130, 300),
    "p256_bf16": (256, 512), "p256_f32": (72, 130, 300, 256),            # 256: a whole tile, which the residual form needs
    "p128_pipe": (128, 384), "p128_loader": (128, 384), "p128_ring4": (128, 384),
}
# glds128x64 is reachable only when the 32 x 64 rule fails, i.e. ceil(M / 128) * ceil(N / 64) >= 128 (gemm_glds.hip:362): at <= 257 rows that takes a wide N.
# Per number of M tiles: (a ragged N, not a multiple of 64; the N used at M = 128 and M = 257, a whole one where there is one).
GLDS128X64_N = {1: (8200, 8192), 2: (4100, 4100), 3: (2760, 2752)}

# act: "none" | "gelu" | "gelu_new";  a_off: column of A inside its buffer when `views` (8 = 16-B aligned; 4 = 8-B aligned only: every fast path must refuse it)
Case = namedtuple("Case", "id form variant M N K epi views a_off act")


def cdiv(a, b):
    return (a + b - 1) // b


def _rup(x, m):
    return (x + m - 1) // m * m


def remap_of(N):
    """(T, Tp, B) of a column-remapped case: N = B * T logical columns, stored Tp apart (Tp - T padding columns per group that no launch may touch)"""
    B = 6 if N % 6 == 0 else (5 if N % 5 == 0 else 4)
    T = N // B
    assert B * T == N
    return T, _rup(T + 1, 8), B


Layout = namedtuple("Layout", "a_off lda w_off ldw c_off ldc ncols r_off ldr")


def layout(c) -> Layout:
    """Where the operands of a case live.  views: A = buf[:, 8:8+K] (or a_off), W = wbuf[:, 16:16+K], out = cat[:, 8:8+ncols] inside a wider row, residual with ldr > N.
    Every leading dimension keeps the alignment the phase kernels ask for (lda, ldw, ldc(bf16) % 8, ldc(fp32), ldr % 4) so that a refusal is never an accident of the layout;
    the LDS-DMA kernels' element-store edge path is reached by the ragged N and, without views, by ldc = N (130: rows not 16-B aligned)."""
    out_f32, _, _, _, remap = EPILOGUES[c.epi]
    ncols = c.N
    if remap:
        T, Tp, B = remap_of(c.N)
        ncols = B * Tp
    if c.views:
        return Layout(c.a_off, c.K + 16, 16, c.K + 24, 8, _rup(8 + ncols + 8, 8), ncols, 4, _rup(c.N + 8, 4))
    ldc = _rup(ncols, 4) if c.form == "p256_f32" else ncols          # the 256 kernel's fp32 form: ldc % 4 == 0 and ldc >= (N + 3) & ~3
    return Layout(0, c.K, 0, c.K, 0, ldc, ncols, 0, c.N)


# ----------------------------------------------------------------------------------------------------------------------------------------
# Python copies of the C++ predicates (see THE WEAK POINT above).  `L` = launch(case).
Launch = namedtuple("Launch", "variant M N K lda ldw ldc ldr out_f32 bias_mode resid act col_T a16 w16 c16 r16 b16")


def launch(c) -> Launch:
    out_f32, bias_mode, resid, _, remap = EPILOGUES[c.epi]
    lo = layout(c)
    es = 4 if out_f32 else 2
    return Launch(c.variant, c.M, c.N, c.K, lo.lda, lo.ldw, lo.ldc, lo.ldr if resid else 0, out_f32, bias_mode, resid, {"none": 0, "gelu": 1, "gelu_new": 2}[c.act],
                  remap_of(c.N)[0] if remap else 0, (lo.a_off * 2) % 16 == 0, (lo.w_off * 2) % 16 == 0, (lo.c_off * es) % 16 == 0, (lo.r_off * 4) % 16 == 0, True)


def refused(L):
    """gemm_bf16.hip `launch`: MI_ERR_ARG"""
    return L.M <= 0 or L.N <= 0 or L.K <= 0 or L.K % 8 != 0 or L.lda % 8 != 0 or L.ldw % 8 != 0


def glds_supported(L):
    """gemm_glds_supported (dense): K % 64 == 0; A, W, C and the residual 16-B aligned; lda, ldw % 8 == 0"""
    if L.K % 64 != 0 or L.M <= 0 or L.N <= 0:
        return False
    if not L.w16 or L.ldw % 8 != 0 or not L.a16 or L.lda % 8 != 0:
        return False
    return L.c16 and (not L.resid or L.r16)


def p256_supported(L):
    """gemm_8p_supported (dense, none of the LayerNorm / training / LSE / CE extras): K % 64 == 0, K >= 128; no column remap, no per-row bias; a residual only with
    fp32 out, N % 256 == 0, ldr % 4 == 0; fp32 out: no activation, ldc % 4 == 0, ldc >= (N + 3) & ~3 (ragged N allowed); bf16 out: N % 256 == 0, ldc % 8 == 0,
    16-B aligned bias; 32-bit byte offsets into A and W"""
    if L.M <= 0 or L.N <= 0 or L.K % 64 != 0 or L.K < 128:
        return False
    if L.col_T or L.bias_mode == 2:
        return False
    if L.resid and (not L.out_f32 or L.N % 256 != 0 or not L.r16 or L.ldr % 4 != 0):
        return False
    if not (L.a16 and L.w16 and L.c16) or L.ldw % 8 != 0:
        return False
    if L.out_f32:
        if L.act != 0 or L.ldc % 4 != 0 or L.ldc < ((L.N + 3) & ~3):
            return False
    else:
        if L.N % 256 != 0 or L.ldc % 8 != 0 or (L.bias_mode == 1 and not L.b16):
            return False
    if L.N * L.ldw * 2 >= 2 ** 32 or L.lda % 8 != 0 or L.M * L.lda * 2 >= 2 ** 32:
        return False
    return True


def p128_supported(L):
    """gemm_8p128_supported: N % 128 == 0, K % 64 == 0, K >= 320; no column remap, no per-row bias; a residual only with fp32 out (ldr % 4 == 0);
    ldc % 4 (fp32) / % 8 (bf16); everything 16-B aligned; 32-bit byte offsets"""
    if L.M <= 0 or L.N <= 0 or L.N % 128 != 0 or L.K % 64 != 0 or L.K < 320:
        return False
    if L.col_T or L.bias_mode == 2 or (L.resid and not L.out_f32):
        return False
    if not (L.a16 and L.w16 and L.c16) or L.lda % 8 != 0 or L.ldw % 8 != 0:
        return False
    if (L.ldc % 4 != 0) if L.out_f32 else (L.ldc % 8 != 0):
        return False
    if L.resid and (not L.r16 or L.ldr % 4 != 0):
        return False
    if L.bias_mode == 1 and not L.b16:
        return False
    return L.M * L.lda * 2 < 2 ** 32 and L.N * L.ldw * 2 < 2 ** 32


def route(L):
    """(form, profiling family) that mi_gemm_bf16_v launches for L: gemm_bf16.hip `launch` + gemm_glds_launch.  The tail-round split (variant 0, more than 256
    tiles of 256 x 256) is outside these sizes and asserted away."""
    if refused(L):
        return "refused", None
    if not glds_supported(L):
        return "generic", PF_GENERIC
    v = L.variant
    phase_ok = v not in (41, 30, 31, 32)
    t256 = cdiv(L.M, 256) * cdiv(L.N, 256)
    assert t256 <= 256, "the tail-round split is not restated here"
    if phase_ok and v not in (42, 43, 47) and p256_supported(L) and (t256 >= 128 or v == 40):
        return ("p256_f32", PF_8P_OUT32) if L.out_f32 else ("p256_bf16", PF_8P_GELU if L.act else PF_8P)
    if phase_ok and p128_supported(L) and (cdiv(L.M, 128) * (L.N // 128) >= 128 or v in (40, 42, 43, 47)):
        ring = (2 if v == 43 else 3) if (v != 47 and L.K % 128 == 0) else 4          # ring 0 (variants 0, 40) = the pipelined form in the product build
        return {2: "p128_loader", 3: "p128_pipe", 4: "p128_ring4"}[ring], PF_8P128
    if v not in (30, 31) and (v == 32 or (L.M <= 2048 and cdiv(L.M, 128) * cdiv(L.N, 64) < 128)):
        return "glds32", PF_GLDS
    steps_per_cu = cdiv(L.M, 128) * cdiv(L.N, 128) * (L.K // 64) // 256
    if v not in (30, 31) and steps_per_cu <= 48:
        return "glds128x64", PF_GLDS
    return "glds128", PF_GLDS


def glds_grid(L):
    """blocks the 128 x 128 / 128 x 64 LDS-DMA forms launch.  128 x 128: variant 30 keeps the product's cap of 512 persistent blocks, 31 is one block per tile;
    128 x 64: capped at 768.  Beyond the cap a block walks several tiles and prefetches the next one's first K tile under its epilogue."""
    if route(L)[0] == "glds128x64":
        return min(cdiv(L.M, 128) * cdiv(L.N, 64), 768)
    g = cdiv(L.M, 128) * cdiv(L.N, 128)
    return g if L.variant == 31 else min(g, 512)


# ----------------------------------------------------------------------------------------------------------------------------------------
# the exact case table
def _variants(form, K):
    if form == "generic":
        return (0, 40, 32)              # not aligned / K % 64 != 0: whatever is forced, the generic kernel runs
    if form == "p128_ring4":
        return (42, 43, 47, 40) if K % 128 else (47,)
    return {"glds32": (32,), "glds128x64": (41,), "glds128": (30, 31), "p256_bf16": (40,), "p256_f32": (40,), "p128_pipe": (42, 40), "p128_loader": (43,)}[form]


def _make(form, variant, M, N, K, epi, views, a_off=None, act="none"):
    a_off = (8 if views else 0) if a_off is None else a_off
    cid = f"{form}-v{variant}-{M}x{N}x{K}-{epi}" + ("-views" if views else "") + (f"-a{a_off}" if a_off not in (0, 8) else "") + ("" if act == "none" else f"-{act}")
    return Case(cid, form, variant, M, N, K, epi, bool(views), a_off, act)


def _rot(seq, i):
    return seq[i % len(seq):] + seq[:i % len(seq)]


def _admissible(form, M, K, vs, Ns, epis, views):
    """The cross product variants x epilogues x N in the order given, filtered to what the dispatch really takes to `form` at (M, K) — the 256 kernel's residual form
    needs a whole N tile; variant 40 reaches the 128 kernel only where the 256 kernel refuses (bf16 out at N % 256 != 0, or a residual at such an N)."""
    out = []
    for v, epi, N in itertools.product(vs, epis, Ns):
        c = _make(form, v, M, N, K, epi, views)
        if route(launch(c))[0] == form:
            out.append(c)
    return out


def _build_exact():
    """Per form: EVERY (K edge, M edge) pair once.  The pair (ki-th K, mi-th M), i = its running number, takes the first admissible combination of the form's lists
    rotated so that they start at variant i, epilogue i + ki and N mi + ki (cyclically), and uses views when ki + mi is odd — every M meets views and contiguous operands.
    tests/test_gemm_cases_cpu.py asserts what this must reach: all K x M pairs, every epilogue, N and variant of the form, both layouts for every M."""
    cases = []
    for form in FORMS:
        Ms = M_EDGES[TILE_M[form]]
        for i, ((ki, K), (mi, M)) in enumerate(itertools.product(enumerate(K_EDGES[form]), enumerate(Ms))):
            if form == "glds128x64":
                ns = GLDS128X64_N[cdiv(M, 128)]
                ns = (ns[1] if M in (128, 257) else ns[0],)
            else:
                ns = FORM_N[form]
            cases.append(_admissible(form, M, K, _rot(_variants(form, K), i), _rot(ns, mi + ki), _rot(FORM_EPILOGUES[form], i + ki), (ki + mi) % 2 == 1)[0])
    # one case per form at K = 4096, the exactness bound (generic: K % 64 == 0, so the A view that is only 8-B aligned is what sends it there)
    big = (("generic", 0, 129, 130, "f32_resid"), ("glds32", 32, 33, 130, "f32_resid"), ("glds128x64", 41, 257, 2760, "f32_resid"), ("glds128", 30, 129, 130, "f32_resid"),
           ("p256_bf16", 40, 257, 256, "bf16_bias"), ("p256_f32", 40, 257, 130, "f32_bias"), ("p128_pipe", 42, 129, 128, "f32_resid"),
           ("p128_loader", 43, 129, 128, "f32_resid"), ("p128_ring4", 47, 129, 128, "f32_resid"))
    for form, v, M, N, epi in big:
        cases.append(_make(form, v, M, N, K_BIG, epi, True, a_off=4 if form == "generic" else None))
    # the 128 x 128 LDS-DMA form with more tiles than its persistent grid: 3 x 172 = 516 tiles on 512 blocks (variant 30), so four blocks walk a second tile whose
    # first K tile they prefetched under the first one's epilogue — and the same shape one block per tile (variant 31)
    cases.append(_make("glds128", 30, 257, 21900, 128, "bf16_bias", True))
    cases.append(_make("glds128", 31, 257, 21900, 128, "bf16_bias", True))
    # the same path of the 128 x 64 form, whose grid is capped at 768 blocks: 3 x 257 = 771 tiles, so three blocks walk a second tile (it has no one-block-per-tile variant)
    cases.append(_make("glds128x64", 41, 257, 16400, 128, "bf16_bias", True))
    # the A base pointer 8-B but not 16-B aligned (buf[:, 4:4+K], lda % 8 == 0): every fast path reports unsupported, whatever the variant asks for
    for v, (M, N, K) in ((0, (129, 130, 192)), (40, (257, 256, 320)), (42, (129, 128, 384)), (32, (33, 72, 256)), (30, (127, 300, 128))):
        cases.append(_make("generic", v, M, N, K, "f32_bias", True, a_off=4))
    assert len({c.id for c in cases}) == len(cases)
    assert all(route(launch(c))[0] == c.form for c in cases)
    return tuple(cases)


EXACT_CASES = _build_exact()
BY_ID = {c.id: c for c in EXACT_CASES}


@functools.lru_cache(maxsize=4)
def _exact_operands(M, N, K):
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).double()
    w = torch.randint(-3, 4, (N, K), generator=g).double()
    bcol = torch.randint(-8, 9, (N,), generator=g).double()
    brow = torch.randint(-8, 9, (M,), generator=g).double()
    res = torch.randint(-8, 9, (M, N), generator=g).double()
    return a, w, bcol, brow, res, a @ w.t()


def exact_inputs(c):
    """(A, W, bias or None, resid or None, alpha) as float64 tensors of the case; the integers above"""
    _, bias_mode, resid, alpha, _ = EPILOGUES[c.epi]
    a, w, bcol, brow, res, _ = _exact_operands(c.M, c.N, c.K)
    return a, w, (None, bcol, brow)[bias_mode], res if resid else None, alpha


def exact_reference(c):
    """float64 (M, N): resid + alpha * (A @ W.T + bias).  Exact: every value is a multiple of 0.5 below 2**24."""
    _, bias_mode, resid, alpha, _ = EPILOGUES[c.epi]
    a, w, bcol, brow, res, lin = _exact_operands(c.M, c.N, c.K)
    if bias_mode == 1:
        lin = lin + bcol
    elif bias_mode == 2:
        lin = lin + brow[:, None]
    return res + alpha * lin if resid else lin          # alpha belongs to the residual form (gemm_args.hpp: out = resid + alpha * (acc + bias))


def reference_f32_chunked(c, reverse):
    """the same value accumulated in float32 over K chunks of 64, first to last or last to first: what a kernel's K loop does, in two different orders"""
    _, bias_mode, resid, alpha, _ = EPILOGUES[c.epi]
    a, w, bcol, brow, res, _ = _exact_operands(c.M, c.N, c.K)
    a, w = a.float(), w.float()
    acc = torch.zeros((c.M, c.N), dtype=torch.float32)
    ks = list(range(0, c.K, 64))
    for k0 in (reversed(ks) if reverse else ks):
        acc = acc + a[:, k0:k0 + 64] @ w[:, k0:k0 + 64].t()
    if bias_mode == 1:
        acc = acc + bcol.float()
    elif bias_mode == 2:
        acc = acc + brow.float()[:, None]
    return res.float() + torch.tensor(alpha, dtype=torch.float32) * acc if resid else acc


def expected(c, ref=None):
    """what the launch must leave, bit for bit, in the output's dtype"""
    ref = exact_reference(c) if ref is None else ref
    return ref.to(torch.float32 if EPILOGUES[c.epi][0] else torch.bfloat16)


# ----------------------------------------------------------------------------------------------------------------------------------------
# float cases: the activation epilogues (every form that admits them; bf16 out, and fp32 out where the form allows an activation with it) ...
def _build_act():
    shapes = {"generic": (0, 129, 130, 136), "glds32": (32, 33, 130, 320), "glds128x64": (41, 257, 2760, 192), "glds128": (30, 129, 300, 192),
              "p256_bf16": (40, 257, 256, 192), "p128_pipe": (42, 129, 128, 384), "p128_loader": (43, 129, 128, 384), "p128_ring4": (47, 129, 384, 448)}
    cases = []
    for form, (v, M, N, K) in shapes.items():
        for act in ("gelu", "gelu_new"):
            for epi in ("bf16_bias", "f32_bias"):
                c = _make(form, v, M, N, K, epi, True, act=act)
                if form == "p256_bf16" and epi == "f32_bias":
                    assert route(launch(c))[0] != "p256_f32"          # gemm_8p_supported: fp32 out admits no activation; the launch falls through to another kernel
                    continue
                cases.append(c)
    return tuple(cases)


ACT_CASES = _build_act()

# ... and cross-form bit identity, only where the source claims it: lists of cases (same shape, same epilogue) whose outputs must be identical
def _build_same_bits():
    groups = []
    for M, N, K in ((257, 2760, 192), (129, 4100, 64)):              # shapes that variant 41 takes to the 128 x 64 tiles; 32 and 30 force the other two anywhere
        for epi, act in (("f32_bias", "none"), ("bf16_bias", "gelu")):
            groups.append(tuple(_make(f, v, M, N, K, epi, True, act=act) for f, v in (("glds32", 32), ("glds128x64", 41), ("glds128", 30))))
    for M, N, K in ((257, 512, 384), (129, 256, 512)):               # K % 128 == 0: the 128 kernel runs its pipelined ring
        for epi, act in (("f32_resid", "none"), ("bf16_bias", "gelu"), ("bf16", "none")):
            groups.append((_make("p256_f32" if epi.startswith("f32") else "p256_bf16", 40, M, N, K, epi, True, act=act), _make("p128_pipe", 42, M, N, K, epi, True, act=act)))
    return tuple(groups)


SAME_BITS = _build_same_bits()


@functools.lru_cache(maxsize=4)
def _float_operands(M, N, K):
    g = torch.Generator().manual_seed(7 + 1000003 * M + 1009 * N + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).double()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).double()
    b = torch.randn(N, generator=g).double()
    res = torch.randn(M, N, generator=g).double()
    return a, w, b, res, a @ w.t()


def float_inputs(c):
    _, bias_mode, resid, alpha, _ = EPILOGUES[c.epi]
    assert bias_mode in (0, 1)
    a, w, b, res, _ = _float_operands(c.M, c.N, c.K)
    return a, w, b if bias_mode else None, res.float().double() if resid else None, alpha


def float_linear(c):
    """float64 A @ W.T + bias of the float inputs (the pre-activation)"""
    a, w, b, res, lin = _float_operands(c.M, c.N, c.K)
    return lin + b if EPILOGUES[c.epi][1] else lin


def gelu_erf64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def float_reference(c):
    lin = float_linear(c)
    y = {"none": lambda t: t, "gelu": gelu_erf64, "gelu_new": gelu_tanh64}[c.act](lin)
    _, _, resid, alpha, _ = EPILOGUES[c.epi]
    if resid:
        y = float_inputs(c)[3] + alpha * y
    return y


# ----------------------------------------------------------------------------------------------------------------------------------------
# implicit-GEMM convolution (mi_conv2d_cl_bf16_v): the im2col loader of the generic kernel, of the 128 x 128 LDS-DMA form and of the 256 kernel
ConvCase = namedtuple("ConvCase", "id form variant B T F Cin Cout K pad causal family")
GEOMETRIES = ((1, 9, 7), (2, 61, 39), (3, 50, 19))      # M = B T' F' = 20 / 1240 / 750: ragged against 128 and 256, border taps in the first and last row of a tile


def conv_out_shape(c):
    KH, KW = c.K
    pt, pf = c.pad
    return (c.T + 2 * pt - KH) // 2 + 1, (c.F + 2 * pf - KW) // 2 + 1


def _build_conv():
    cases = []
    forms = (("generic", 0, 8, 72, PF_GENERIC), ("generic", 0, 72, 130, PF_GENERIC),          # Cin % 64 != 0: gemm_glds_supported(conv) refuses
             ("glds128", 0, 64, 72, PF_GLDS), ("glds128", 0, 64, 128, PF_GLDS),               # Cin % 64 == 0, default variant: too few tiles for the 256 kernel (t256 < 128)
             ("p256", 40, 64, 256, PF_8P_CONV), ("p256", 40, 128, 256, PF_8P_CONV))           # variant 40: the 256 kernel wherever gemm_8p_supported (Cout % 256 == 0)
    for form, v, Cin, Cout, fam in forms:
        for gi, (B, T, Fd) in enumerate(GEOMETRIES):
            for causal in (False, True):
                cases.append(ConvCase(f"{form}-v{v}-{B}x{T}x{Fd}-c{Cin}-o{Cout}-" + ("causal" if causal else "sym"), form, v, B, T, Fd, Cin, Cout, (3, 3), (1, 1), causal, fam))
        cases.append(ConvCase(f"{form}-v{v}-2x61x39-c{Cin}-o{Cout}-time3x1", form, v, 2, 61, 39, Cin, Cout, (3, 1), (1, 0), False, fam))
    return tuple(cases)


CONV_CASES = _build_conv()


def conv_route(c):
    """the family mi_conv2d_cl_bf16_v launches, restated from gemm_bf16.hip `launch`, gemm_glds_supported(conv) and gemm_glds_launch: Cin % 8 == 0 or refused;
    the LDS-DMA path needs K % 64 == 0 and Cin % 64 == 0; on it the 256 kernel takes Cout % 256 == 0 (K >= 128) when forced (40) or at >= 128 tiles"""
    KH, KW = c.K
    K = KH * KW * c.Cin
    T1, F1 = conv_out_shape(c)
    M = c.B * T1 * F1
    if c.Cin % 8 or K % 8:
        return None
    if K % 64 or c.Cin % 64:
        return PF_GENERIC
    if c.Cout % 256 == 0 and K >= 128 and (cdiv(M, 256) * cdiv(c.Cout, 256) >= 128 or c.variant == 40):
        return PF_8P_CONV
    return PF_GLDS


@functools.lru_cache(maxsize=4)
def conv_inputs(c, exact=True):
    """x (B, T, F, Cin) channels-last, w (Cout, KH*KW*Cin) with k = (kh*KW + kw)*Cin + c, bias (Cout): float64"""
    KH, KW = c.K
    g = torch.Generator().manual_seed(31 + c.B * 7919 + c.T * 131 + c.Cin * 17 + c.Cout)
    if exact:
        x = torch.randint(-3, 4, (c.B, c.T, c.F, c.Cin), generator=g).double()
        w = torch.randint(-3, 4, (c.Cout, KH * KW * c.Cin), generator=g).double()
        b = torch.randint(-8, 9, (c.Cout,), generator=g).double()
    else:
        x = torch.randn(c.B, c.T, c.F, c.Cin, generator=g).to(torch.bfloat16).double()
        w = (torch.randn(c.Cout, KH * KW * c.Cin, generator=g) / math.sqrt(KH * KW * c.Cin)).to(torch.bfloat16).double()
        b = torch.randn(c.Cout, generator=g).double()
    return x, w, b


def conv_reference(c, exact=True):
    """float64 F.conv2d, channels-last (B, T', F', Cout); causal = all the padding in front (time and frequency), as ops.conv2d_cl lays it out"""
    KH, KW = c.K
    pt, pf = c.pad
    x, w, b = conv_inputs(c, exact)
    xn = x.permute(0, 3, 1, 2)
    wn = w.reshape(c.Cout, KH, KW, c.Cin).permute(0, 3, 1, 2)
    if c.causal:
        y = F.conv2d(F.pad(xn, (2 * pf, 0, 2 * pt, 0)), wn, b, stride=2)
    else:
        y = F.conv2d(xn, wn, b, stride=2, padding=(pt, pf))
    return y.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------------------------------------------------------------------
# tolerances of the float tests
BF16_ATOL, BF16_RTOL = 2e-2, 1.2e-2             # tests/test_gpu_ops.py assert_close_bf16: ~1 bf16 ulp of the reference value + the small-value floor
GELU_FIT_ATOL, GELU_FIT_RTOL = 2.6e-5, 5e-4     # huggingface_asr_amd/csrc/common.hpp gelu_erf: the fit's documented error
