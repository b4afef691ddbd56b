"""tests/gemm_cases.py without a GPU: the integer cases really are exact in every fp32 accumulation order (which is what makes the zero tolerance of
tests/test_gpu_gemm_forms.py legitimate), the case table reaches every form at every K edge with ragged and whole M, and every case is admissible for the form it
names under the Python copies of the C++ `*_supported` predicates — whose conditions are pinned here one by one, so that an edit of a copy is as visible as an
edit of the table."""
import pytest
import torch

import gemm_cases as G

SMALL = [c for c in G.EXACT_CASES if c.M * c.N * c.K <= 257 * 512 * 512]
LARGE = [c for c in G.EXACT_CASES if c not in SMALL]


def _check_exact(c):
    ref = G.exact_reference(c)
    assert float(ref.abs().max()) < 2 ** 24
    a, w, bias, resid, alpha = G.exact_inputs(c)
    assert float(a.abs().max()) <= 3 and float(w.abs().max()) <= 3 and alpha in (1.0, 0.5)
    assert 9 * c.K < 2 ** 24 and c.K <= G.K_BIG                     # |any partial sum| <= 9 K: no order of the k terms can round
    for t in (bias, resid):
        assert t is None or float(t.abs().max()) <= 8
    for reverse in (False, True):
        r32 = G.reference_f32_chunked(c, reverse)
        assert r32.dtype == torch.float32 and torch.equal(r32.double(), ref), (c.id, reverse)
    exp = G.expected(c, ref)
    assert exp.dtype == (torch.float32 if G.EPILOGUES[c.epi][0] else torch.bfloat16)
    if exp.dtype == torch.float32:
        assert torch.equal(exp.double(), ref)                      # the fp32 expectation IS the float64 value
    else:
        assert torch.equal(exp, ref.float().to(torch.bfloat16))    # one rounding: float64 -> bf16 equals fp32 -> bf16, since the fp32 value is the float64 one


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_exact_case_is_exact_in_any_k_order(c):
    _check_exact(c)


def test_exact_cases_at_the_large_sizes_are_exact_in_any_k_order():
    """K = 4096 (the bound: 9 * 4096 = 36864), the wide-N shapes of the 128 x 64 form and the 516-tile one"""
    assert {c.K for c in LARGE} >= {G.K_BIG}
    seen = set()
    for c in LARGE:
        if (c.M, c.N, c.K, c.epi) not in seen:
            seen.add((c.M, c.N, c.K, c.epi))
            _check_exact(c)


def test_a_dropped_k_slice_changes_the_exact_reference():
    """the net's mesh: with integer operands a missing or doubled 64-wide k-slice moves at least one output of every row block by at least 1 (0.5 under alpha)"""
    for c in (G.BY_ID[i] for i in ("glds32-v32-33x130x4096-f32_resid-views", "p256_bf16-v40-257x256x4096-bf16_bias-views")):
        a, w, *_ = G.exact_inputs(c)
        ref = a @ w.t()
        for k0 in (0, c.K - 64):
            part = a[:, k0:k0 + 64] @ w[:, k0:k0 + 64].t()
            for m0 in range(0, c.M, 32):
                assert bool((part[m0:m0 + 32] != 0).any())
            if not G.EPILOGUES[c.epi][0]:
                assert not torch.equal((ref - part).to(torch.bfloat16), ref.to(torch.bfloat16))


def test_table_covers_every_form_k_edge_and_row_edge():
    cases = G.EXACT_CASES
    assert {c.form for c in cases} == set(G.FORMS)
    for form in G.FORMS:
        mine = [c for c in cases if c.form == form]
        tile = G.TILE_M[form]
        for K in G.K_EDGES[form] + (G.K_BIG,):
            at_k = [c for c in mine if c.K == K]
            assert at_k, (form, K)
            if K != G.K_BIG:
                ms = {c.M for c in at_k}
                assert ms >= set(G.M_EDGES[tile]), (form, K, ms)
                assert any(m % tile == 0 for m in ms) and any(m % tile for m in ms) and 1 in ms and any(m > tile for m in ms)
        assert {c.epi for c in mine} == set(G.FORM_EPILOGUES[form]), form
        for M in G.M_EDGES[tile]:                      # every row edge with contiguous operands AND with views (ragged last M tile next to ldc > N padding cells)
            assert {c.views for c in mine if c.M == M} == {False, True}, (form, M)
        ns = {c.N for c in mine}
        assert ns >= ({2760, 2752, 4100, 8200, 8192} if form == "glds128x64" else set(G.FORM_N[form])), (form, ns)
    assert set().union(*(set(v) for v in G.M_EDGES.values())) >= {1, 31, 33, 127, 129, 255, 257}
    # every variant the dispatch knows is used, on the form its comment names
    by_form = {f: {c.variant for c in cases if c.form == f} for f in G.FORMS}
    assert by_form["glds32"] == {32} and by_form["glds128x64"] == {41} and by_form["glds128"] == {30, 31}
    assert by_form["p256_bf16"] == {40} and by_form["p256_f32"] == {40}
    assert by_form["p128_pipe"] == {42, 40} and by_form["p128_loader"] == {43} and by_form["p128_ring4"] == {42, 43, 47, 40}
    assert {c.variant for c in cases if c.form == "p128_ring4" and c.K % 128 == 0} == {47}
    assert {c.variant for c in cases if c.form == "p128_ring4" and c.K == 320} >= {42, 43, 47}
    assert {0, 40, 42, 32, 30} <= {c.variant for c in cases if c.form == "generic" and c.a_off == 4}       # the misaligned A base under every forced fast path
    assert {c.K for c in cases if c.form == "generic" and c.a_off != 4} == {8, 72, 136}
    # the persistent grids of the 128 x 128 and 128 x 64 LDS-DMA forms walk more than one tile (next-tile prefetch) in exactly these cases
    walk = [c for c in cases if c.form == "glds128" and G.cdiv(c.M, 128) * G.cdiv(c.N, 128) > 512]
    assert [c.variant for c in walk] == [30, 31]
    assert G.glds_grid(G.launch(walk[0])) == 512 < G.glds_grid(G.launch(walk[1])) == 516
    walk64 = [c for c in cases if c.form == "glds128x64" and G.cdiv(c.M, 128) * G.cdiv(c.N, 64) > 768]
    assert len(walk64) == 1 and G.glds_grid(G.launch(walk64[0])) == 768 < G.cdiv(walk64[0].M, 128) * G.cdiv(walk64[0].N, 64) == 771
    # sizes stay small: at most 257 rows; only the K = 4096 cases go beyond K = 512
    assert all(c.M <= 257 for c in cases) and all(c.K <= 512 or c.K == G.K_BIG for c in cases)
    assert sum(c.K == G.K_BIG for c in cases) == len(G.FORMS)


@pytest.mark.parametrize("c", G.EXACT_CASES + G.ACT_CASES + tuple(x for g in G.SAME_BITS for x in g), ids=lambda c: c.id)
def test_case_is_admissible_for_its_form(c):
    """why the case reaches the form it names: the restated `*_supported` conditions and the dispatch rule, spelled out per form"""
    L, lo = G.launch(c), G.layout(c)
    form, family = G.route(L)
    assert form == c.form
    assert c.epi in G.FORM_EPILOGUES[c.form] or c.act != "none"
    assert not G.refused(L) and L.lda % 8 == 0 and L.ldw % 8 == 0 and L.K % 8 == 0
    assert lo.lda >= lo.a_off + c.K and lo.ldw >= lo.w_off + c.K and lo.ldc >= lo.c_off + lo.ncols
    if c.views:
        assert lo.lda > c.K and lo.ldw > c.K and lo.ldc > lo.ncols and (not L.resid or lo.ldr > c.N)
    if c.form == "generic":
        assert family == G.PF_GENERIC and (c.K % 64 != 0 or not L.a16)
        return
    assert c.K % 64 == 0 and L.a16 and L.w16 and L.c16 and (L.r16 or not L.resid) and G.glds_supported(L)
    if c.form.startswith("glds"):
        assert family == G.PF_GLDS
        assert c.variant in (41, 30, 31, 32)                                       # the phase kernels are switched off, not merely unsupported
        if c.form == "glds32":
            assert c.variant == 32
        if c.form == "glds128x64":
            # gemm_glds.hip:362-367: NOT (M <= 2048 and ceil(M/128) * ceil(N/64) < 128), and at most 48 K steps of 128 x 128 work per CU
            assert G.cdiv(c.M, 128) * G.cdiv(c.N, 64) >= 128
            assert G.cdiv(c.M, 128) * G.cdiv(c.N, 128) * (c.K // 64) // 256 <= 48
        if c.form == "glds128":
            assert c.variant in (30, 31)
    elif c.form in ("p256_bf16", "p256_f32"):
        assert c.variant == 40 and c.K >= 128 and not L.col_T and L.bias_mode != 2 and G.p256_supported(L)
        if c.form == "p256_bf16":
            assert family == (G.PF_8P_GELU if c.act != "none" else G.PF_8P)
            assert c.N % 256 == 0 and lo.ldc % 8 == 0 and not L.resid and not L.out_f32
        else:
            assert family == G.PF_8P_OUT32 and c.act == "none"
            assert lo.ldc % 4 == 0 and lo.ldc >= ((c.N + 3) & ~3)
            assert not L.resid or (c.N % 256 == 0 and L.ldr % 4 == 0)
    else:
        assert family == G.PF_8P128 and G.p128_supported(L)
        assert c.N % 128 == 0 and c.K >= 320 and not L.col_T and L.bias_mode != 2
        assert (lo.ldc % 4 == 0) if L.out_f32 else (lo.ldc % 8 == 0 and not L.resid)
        assert not L.resid or L.ldr % 4 == 0
        if c.variant == 40:
            assert not G.p256_supported(L)                                         # 40 asks for the 256 kernel first
        even = c.K % 128 == 0
        if c.form == "p128_pipe":
            assert even and c.variant in (42, 40)
        elif c.form == "p128_loader":
            assert even and c.variant == 43 and c.K // 64 >= 4
        else:
            assert c.variant == 47 or not even


def _L(**kw):
    base = dict(variant=0, M=129, N=256, K=384, lda=384, ldw=384, ldc=256, ldr=0, out_f32=False, bias_mode=1, resid=False, act=0, col_T=0,
                a16=True, w16=True, c16=True, r16=True, b16=True)
    base.update(kw)
    return G.Launch(**base)


def test_restated_predicates_pin_each_condition():
    """one assertion per condition of the C++ predicates that the table relies on (gemm_bf16.hip `launch`, gemm_glds_supported, gemm_8p_supported, gemm_8p128_supported)"""
    ok = _L()
    assert not G.refused(ok) and G.glds_supported(ok) and G.p256_supported(ok) and G.p128_supported(ok)
    for bad in (_L(K=380), _L(lda=388), _L(ldw=388), _L(K=0)):
        assert G.refused(bad)
    for bad in (_L(K=136, lda=136, ldw=136), _L(a16=False), _L(w16=False), _L(c16=False), _L(out_f32=True, resid=True, ldr=256, r16=False)):
        assert not G.refused(bad) and not G.glds_supported(bad)
    # 256 kernel: K % 64, K >= 128, N % 256 / ldc % 8 with bf16 out, no remap, no row bias, residual rules, fp32: no activation, ldc % 4, ldc >= (N + 3) & ~3
    assert G.p256_supported(_L(K=128, lda=128, ldw=128)) and not G.p256_supported(_L(K=64, lda=64, ldw=64))
    for bad in (_L(N=384, ldc=384), _L(ldc=260), _L(col_T=64), _L(bias_mode=2), _L(resid=True, ldr=256), _L(b16=False), _L(a16=False)):
        assert not G.p256_supported(bad)
    f32 = dict(out_f32=True, ldc=132, N=130)
    assert G.p256_supported(_L(**f32))
    for bad in (_L(**dict(f32, act=1)), _L(**dict(f32, ldc=130)), _L(**dict(f32, ldc=128)), _L(**dict(f32, resid=True, ldr=132)),
                _L(out_f32=True, resid=True, ldr=258), _L(out_f32=True, resid=True, ldr=256, r16=False)):
        assert not G.p256_supported(bad)
    assert G.p256_supported(_L(out_f32=True, resid=True, ldr=256))
    # 128 kernel: N % 128, K % 64, K >= 320, ldc % 4 / % 8, residual with fp32 out only and ldr % 4
    assert G.p128_supported(_L(K=320, lda=320, ldw=320, N=128, ldc=128)) and not G.p128_supported(_L(K=256, lda=256, ldw=256))
    for bad in (_L(N=192, ldc=192), _L(ldc=260), _L(out_f32=True, ldc=258), _L(resid=True, ldr=256), _L(out_f32=True, resid=True, ldr=258), _L(col_T=64), _L(bias_mode=2),
                _L(b16=False), _L(w16=False), _L(K=352, lda=352, ldw=352)):
        assert not G.p128_supported(bad)
    assert G.p128_supported(_L(out_f32=True, ldc=260)) and G.p128_supported(_L(out_f32=True, resid=True, ldr=260, act=1))


def test_route_restates_the_dispatch():
    r = lambda **kw: G.route(_L(**kw))[0]
    assert r() == "glds32"                                              # product dispatch at a small size: 2 x 4 = 8 tiles of 128 x 64 < 128
    assert r(variant=40) == "p256_bf16" and r(variant=40, out_f32=True) == "p256_f32"
    assert r(variant=40, N=384, ldc=384) == "p128_pipe" and r(variant=40, N=384, ldc=384, K=320, lda=320, ldw=320) == "p128_ring4"
    assert r(variant=42) == "p128_pipe" and r(variant=43) == "p128_loader" and r(variant=47) == "p128_ring4"
    assert r(variant=42, K=448, lda=448, ldw=448) == r(variant=43, K=448, lda=448, ldw=448) == "p128_ring4"
    assert r(variant=42, K=256, lda=256, ldw=256) == "glds32"            # K below the 128 kernel's minimum: a forced variant falls through silently
    assert r(variant=41) == "glds32" and r(variant=41, M=257, N=2760, ldc=2760) == "glds128x64" and r(variant=41, M=257, N=2752, ldc=2752) == "glds128x64"
    assert r(variant=41, M=257, N=2688, ldc=2688) == "glds32"            # 3 x 42 = 126 < 128
    assert r(variant=41, M=257, N=2760, ldc=2760, K=64 * 208, lda=64 * 208, ldw=64 * 208) == "glds128"      # 3 * 22 * 208 / 256 = 53 K steps per CU > 48
    assert r(variant=30) == r(variant=31) == "glds128" and r(variant=32, M=4000) == "glds32"
    assert r(variant=40, a16=False) == r(variant=42, K=136, lda=136, ldw=136) == "generic"
    assert G.route(_L(lda=388)) == ("refused", None)
    assert G.route(_L(variant=40, act=1))[1] == G.PF_8P_GELU and G.route(_L(variant=40))[1] == G.PF_8P


def test_float_cases_cover_every_form_that_admits_an_activation():
    forms = {c.form for c in G.ACT_CASES}
    assert forms == set(G.FORMS) - {"p256_f32"}                        # gemm_8p_supported: the fp32 epilogue of the 256 kernel takes no activation
    for form in forms:
        got = {(c.act, G.EPILOGUES[c.epi][0]) for c in G.ACT_CASES if c.form == form}
        want = {(a, f) for a in ("gelu", "gelu_new") for f in ((False,) if form == "p256_bf16" else (False, True))}
        assert got == want, form
    # launch-to-launch reproducibility is checked on float inputs by test_activation_epilogues and by every case of a SAME_BITS group: together, every form
    assert forms | {c.form for g in G.SAME_BITS for c in g} == set(G.FORMS)
    for group in G.SAME_BITS:
        assert len({(c.M, c.N, c.K, c.epi, c.act, c.views) for c in group}) == 1 and len({c.form for c in group}) == len(group)
        if group[0].form.startswith("p256"):
            assert group[0].K % 128 == 0                                # the claim of gemm_glds.hip:324 is about the pipelined ring's K order
    assert {tuple(c.form for c in g) for g in G.SAME_BITS} == {("glds32", "glds128x64", "glds128"), ("p256_f32", "p128_pipe"), ("p256_bf16", "p128_pipe")}


def test_gelu_references():
    x = torch.linspace(-6, 6, 1001, dtype=torch.float64)
    assert torch.allclose(G.gelu_erf64(x), torch.nn.functional.gelu(x), rtol=0, atol=1e-15)
    assert torch.allclose(G.gelu_tanh64(x), torch.nn.functional.gelu(x, approximate="tanh"), rtol=0, atol=1e-15)


@pytest.mark.parametrize("c", G.CONV_CASES, ids=lambda c: c.id)
def test_conv_case_is_exact_and_routed(c):
    KH, KW = c.K
    K = KH * KW * c.Cin
    assert 9 * K < 2 ** 24 and K <= G.K_BIG
    assert G.conv_route(c) == c.family
    x, w, b = G.conv_inputs(c)
    ref = G.conv_reference(c)
    T1, F1 = G.conv_out_shape(c)
    assert ref.shape == (c.B, T1, F1, c.Cout) and float(ref.abs().max()) < 2 ** 24
    # the same convolution as an explicit im2col GEMM in float32 with the taps reversed: exact in any order, and the (kh, kw, c) weight layout is the documented one
    pt, pf = c.pad
    front_t, front_f = (2 * pt, 2 * pf) if c.causal else (pt, pf)
    xp = torch.zeros((c.B, c.T + 2 * pt, c.F + 2 * pf, c.Cin), dtype=torch.float32)
    xp[:, front_t:front_t + c.T, front_f:front_f + c.F] = x.float()
    acc = torch.zeros((c.B, T1, F1, c.Cout), dtype=torch.float32)
    for tap in reversed(range(KH * KW)):
        kh, kw = divmod(tap, KW)
        patch = xp[:, kh:kh + 2 * (T1 - 1) + 1:2, kw:kw + 2 * (F1 - 1) + 1:2]
        acc = acc + patch @ w[:, tap * c.Cin:(tap + 1) * c.Cin].float().t()
    assert torch.equal((acc + b.float()).double(), ref)


def test_conv_table_covers_forms_and_geometry():
    for form, cins in (("generic", {8, 72}), ("glds128", {64}), ("p256", {64, 128})):
        mine = [c for c in G.CONV_CASES if c.form == form]
        assert {c.Cin for c in mine} == cins
        assert {(c.B, c.T, c.F) for c in mine} == set(G.GEOMETRIES) and {c.causal for c in mine} == {False, True} and {c.K for c in mine} == {(3, 3), (3, 1)}
        for c in mine:
            T1, F1 = G.conv_out_shape(c)
            assert (c.B * T1 * F1) % 128 != 0
    assert all(c.Cout == 256 and c.variant == 40 for c in G.CONV_CASES if c.form == "p256")
