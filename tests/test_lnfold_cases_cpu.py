"""tests/lnfold_cases.py without a GPU: the producer's integer cases are exact in every fp32 summation order (what makes `torch.equal` legitimate in
tests/test_gpu_lnfold_forms.py), the case tables cover what the issue lists, the consumer's folded float64 reference IS layer_norm -> linear, and — the point of
the consumer test — every wrong row, wrong slot and wrong partial lands at least 10 x outside the derived bound in every row tile, so a kernel with such a
defect cannot pass."""
import pytest
import torch

import lnfold_cases as L


# ----------------------------------------------------------------------------------------------------------------- A. producer
@pytest.mark.parametrize("c", L.PRODUCER_CASES, ids=lambda c: c.id)
def test_producer_case_is_exact_in_any_order(c):
    k_sum, s_sum, q_sum = L.producer_exactness(c)
    print(f"EXACT {c.id} K-sum {k_sum:.0f} block sum {s_sum:.0f} lsb, block sumsq {q_sum:.0f} lsb^2 (limit {L.EXACT_LIMIT})")
    assert k_sum < L.EXACT_LIMIT and s_sum < L.EXACT_LIMIT and q_sum < L.EXACT_LIMIT
    a, w, b, res = L.producer_inputs(c)
    assert float(a.abs().max()) <= 2 and float(w.abs().max()) <= 1 and float(b.abs().max()) <= 4 and float(res.abs().max()) <= 8 and c.alpha in (0.5, 1.0)
    C, pairs = L.producer_reference(c)
    assert torch.equal(pairs.float().double(), pairs)                          # the expected statistics are fp32 values
    # the same sums in fp32, accumulated forwards and backwards over the columns of a block: the same bits
    bw = L.block_width(c.kernel)
    xs = C.float().reshape(c.M, c.N // bw, bw)
    for order in (range(bw), reversed(range(bw))):
        s = torch.zeros(xs.shape[:2]); q = torch.zeros(xs.shape[:2])
        for k in order:
            s = s + xs[..., k]; q = q + xs[..., k] * xs[..., k]
        assert torch.equal(s.double(), pairs[..., 0]) and torch.equal(q.double(), pairs[..., 1])


def test_producer_table_covers_the_listed_shapes_and_forms():
    for kernel, variants, Ms, Ns, Ks in ((128, L.P128_VARIANTS, L.P128_M, L.P128_N, L.P128_K), (256, L.P256_VARIANTS, L.P256_M, L.P256_N, L.P256_K)):
        for v in variants:
            cs = [c for c in L.PRODUCER_CASES if c.variant == v]
            assert all(c.kernel == kernel for c in cs)
            assert {c.M for c in cs} >= set(Ms) and {c.N for c in cs} >= set(Ns) and {c.K for c in cs} >= set(Ks), v
            assert any(c.resid == "inplace" for c in cs) and {c.alpha for c in cs} == {0.5, 1.0}
    assert len(L.PRODUCER_CASES) <= 40
    assert all(L.producer_supported(c.kernel, c.M, c.N, c.K) for c in L.PRODUCER_CASES)
    # a dropped, doubled or misplaced block is visible: no two blocks of a row share their (sum, sumsq) in every row, and no block's sumsq is 0
    for c in L.PRODUCER_CASES:
        pairs = L.producer_reference(c)[1]
        assert bool((pairs[..., 1] > 0).all())
        for s in range(1, pairs.shape[1]):
            assert bool((pairs[:, s] != pairs[:, s - 1]).any())


def test_refusals_are_outside_what_the_kernels_take():
    for what, kernel, variant, N, K, pad2 in L.PRODUCER_REFUSALS:
        assert variant == 7 or not L.producer_supported(kernel, 129, N, K, N + pad2), what
    for what, N, K, npart, act, mis in L.CONSUMER_REFUSALS:
        assert mis is not None or not L.consumer_supported(N, K, npart, act), what
    assert {r[3] for r in L.CONSUMER_REFUSALS} >= {0, 2, 5, 20} and {(r[1], r[2]) for r in L.CONSUMER_REFUSALS} >= {(384, 128), (256, 64), (256, 200)}


# ----------------------------------------------------------------------------------------------------------------- B. consumer
def test_consumer_table_covers_the_listed_edges():
    cs = L.CONSUMER_CASES
    assert len(cs) <= 40 and all(L.consumer_supported(c.N, c.K, c.npart, 0) for c in cs)
    assert {c.M for c in cs} == set(L.C_M) and {c.N for c in cs} == set(L.C_N) and {c.K for c in cs} == set(L.C_K) and {c.act for c in cs} == set(L.C_ACT)
    assert {c.K // 64 for c in cs} >= {2, 3, 5, 8}                             # the main loop body runs 0, 1, 3 and 6 times
    assert {c.M % 256 for c in cs} >= {1, 255}                                 # a row tile of one row; one that lacks one
    assert {c.npart for c in cs if c.M == 257} == set(L.C_NPART) and {c.npart for c in cs if c.K == 128} == set(L.C_NPART)
    assert {(c.K, c.npart) for c in cs} == {(K, p) for K in L.C_K for p in L.C_NPART}
    for p in L.C_NPART:
        assert {c.act for c in cs if c.npart == p} == set(L.C_ACT) and {c.N for c in cs if c.npart == p} == set(L.C_N)


@pytest.mark.parametrize("c", L.CONSUMER_CASES, ids=lambda c: c.id)
def test_consumer_inputs_are_exact_and_rows_differ(c):
    acc_sum, s_sum, q_sum, ratio = L.consumer_exactness(c)
    assert acc_sum < L.EXACT_LIMIT and s_sum < L.EXACT_LIMIT and q_sum < L.EXACT_LIMIT
    assert ratio <= 4.0, ratio
    i = L.consumer_inputs(c)
    assert torch.equal(i.stats.float().double(), i.stats) and torch.equal(i.stats.sum(1)[:, 0], i.x.sum(1)) and torch.equal(i.stats.sum(1)[:, 1], (i.x * i.x).sum(1))
    assert torch.equal(i.colsum, i.wf.sum(1))
    if c.npart > 1:                                                            # neighbouring blocks of a row carry clearly different sums: a level apart
        sizes = torch.bincount(L.block_index(c.K, c.npart)).double()
        m = i.stats[..., 0] / sizes
        assert float((m[:, 1:] - m[:, :-1]).abs().median()) >= 0.5
    if c.M > 1:                                                                # neighbouring rows: different (mean, sigma)
        mean, sd = i.x.mean(1), i.x.std(1)
        assert bool(((mean[1:] - mean[:-1]).abs() + (sd[1:] - sd[:-1]).abs() > 0.25).all())


@pytest.mark.parametrize("c", L.CONSUMER_CASES, ids=lambda c: c.id)
def test_folded_reference_is_layer_norm_then_linear(c):
    ref = L.consumer_reference(c)
    want = L.unfolded_reference(c)
    assert float(((ref.want - want).abs() / (1.0 + want.abs())).max()) < 1e-9
    assert bool((ref.bound > 0).all()) and bool((ref.bound < 0.02 + 0.01 * ref.want.abs()).all())     # the bound is about a bf16 half ulp, not a licence


@pytest.mark.parametrize("c", L.CONSUMER_CASES, ids=lambda c: c.id)
def test_every_wrong_row_slot_and_partial_is_ten_bounds_away_in_every_row_tile(c):
    ref = L.consumer_reference(c)
    wrong = L.wrong_references(c)
    assert (c.M == 1 or "a-next-row" in wrong) and sum(k.startswith("b-") for k in wrong) == c.npart and sum(k.startswith("c-") for k in wrong) == c.npart
    worst = {}
    for name, w in wrong.items():
        ratio = (w - ref.want).abs() / ref.bound
        per_tile = [float(ratio[m0:m0 + 256].max()) for m0 in range(0, c.M, 256)]
        worst[name] = min(per_tile)
    low = min(worst, key=worst.get)
    print(f"DISCRIMINATION {c.id} weakest {low} {worst[low]:.1f} x bound")
    assert worst[low] >= 10.0, (low, worst[low])


def test_zero_rows_have_zero_statistics_and_the_bias_as_output():
    for c in L.CONSUMER_CASES[:3]:
        i, ref = L.consumer_inputs(c, True), L.consumer_reference(c, True)
        assert bool((i.stats[1::4] == 0).all()) and bool((i.x[0] != 0).any())
        assert torch.equal(ref.want[1::4], L.act64(c.act)(i.cbias)[None, :].expand(len(ref.want[1::4]), -1))


def test_half_ulp_of_bf16():
    a = torch.tensor([1.0, 1.99, 2.0, 0.75, 100.0, 0.0], dtype=torch.float64)
    assert L.bf16_half_ulp(a).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -2, 2.0 ** -134]
    x = torch.linspace(-300, 300, 20001, dtype=torch.float32)                  # fp32 values, as the kernel rounds them: one rounding
    assert bool(((x.to(torch.bfloat16).double() - x.double()).abs() <= L.bf16_half_ulp(x.double().abs())).all())


# ----------------------------------------------------------------------------------------------------------------- C. row kernel
def test_row_cases_reach_every_instantiation_and_partly_valid_lanes():
    assert {L.row_nv(d) for d in L.ROW_D} == {1, 2, 4, 8} and L.row_nv(2048) == 8 and L.row_nv(1028) == 8 and L.row_nv(260) == 2 and L.row_nv(768) == 4
    assert sum((d // 4) % 64 != 0 for d in L.ROW_D) >= 4 and all(d % 4 == 0 and d <= 2048 for d in L.ROW_D)
    assert all(M % 4 != 0 for M in L.ROW_M) and set(L.ROW_CASES) == {(d, M) for d in L.ROW_D for M in L.ROW_M}
    for M in L.ROW_M:
        T, lens, masked = L.row_mask(M)
        assert (M - 1) // T < len(lens) and bool(masked.any()) and (M == 1 or not bool(masked.all()))
    x, gs, bs = L.row_inputs(256, 9)
    assert 0.2 < float(x.mean()) < 0.8 and torch.equal(x.float().double(), x)
