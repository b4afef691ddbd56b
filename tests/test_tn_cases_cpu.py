"""tests/tn_cases.py without a GPU: the integer cases really are exact in every fp32 accumulation order (which is what makes the zero tolerance of
tests/test_gpu_tn_forms.py legitimate), a dropped or doubled row, stage or split moves the reference, the tables reach every kernel form, stage count, ragged-row
class and split class they claim, the Python copies of the C++ dispatch are pinned value by value at their thresholds, and the argument checks of the three entry
points refuse before anything is launched (fake addresses: there is no GPU here)."""
import ctypes as C

import pytest
import torch

import tn_cases as T


# ----------------------------------------------------------------------------------------------------------------- exactness
def _orders(n):
    g = torch.Generator().manual_seed(n)
    return list(range(n)), list(reversed(range(n))), torch.randperm(n, generator=g).tolist()


def _check_tn_exact(M, dy, x, want_prod, want_col):
    assert M <= T.M_BOUND and 2 * 9 * M + 8 < 2 ** 24
    assert float(dy.abs().max()) <= 3 and float(x.abs().max()) <= 3 and float(dy.abs().min()) >= 1
    assert float(want_prod.abs().max()) <= 9 * M and float(want_col.abs().max()) <= 3 * M
    for order in _orders(T.cdiv(M, 64)):
        acc, col = T.tn_reference_f32(dy, x, order)
        assert acc.dtype == torch.float32 and torch.equal(acc.double(), want_prod) and torch.equal(col.double(), want_col)


SMALL_TN = [c for c in T.TN_CASES if c.M <= 2049]


@pytest.mark.parametrize("c", SMALL_TN, ids=lambda c: c.id)
def test_weight_gradient_case_is_exact_in_any_row_order(c):
    dy, x, bw, bb = T.tn_inputs(c)
    assert float(x.abs().min()) >= 1 and float(bw.abs().max()) <= 8 and float(bb.abs().max()) <= 8
    w1, b1 = T.tn_reference(c)
    _check_tn_exact(c.M, dy, x, (w1 - bw) if c.n_store == c.N else dy.t() @ x, dy.sum(0))
    assert torch.equal(w1, bw + (dy.t() @ x)[:c.n_store]) and torch.equal(b1, bb + dy.sum(0)[:c.n_store])
    w2, b2 = T.tn_reference(c, calls=2)
    assert torch.equal(w2 - w1, w1 - bw) and float(w2.abs().max()) < 2 ** 24 and torch.equal(w2.float().double(), w2) and torch.equal(b2.float().double(), b2)


def test_weight_gradient_cases_on_the_long_routes_are_exact_in_any_row_order():
    """M >= 32767: one check per distinct (M, N, K), stages of 64 rows forward, backward and shuffled"""
    seen = set()
    for c in T.TN_CASES:
        if c not in SMALL_TN and (c.M, c.N, c.K) not in seen:
            seen.add((c.M, c.N, c.K))
            dy, x, _, _ = T.tn_inputs(c)
            _check_tn_exact(c.M, dy, x, dy.t() @ x, dy.sum(0))
    assert len(seen) >= 12


@pytest.mark.parametrize("c", [c for c in T.CONV_CASES if T.conv_mnk(c)[0] < 32768], ids=lambda c: c.id)
def test_conv_weight_gradient_case_is_exact_and_is_the_im2col_product(c):
    """the autograd reference equals dY^T im2col(x) with the im2col operand restated by index arithmetic, in any order of 64-row stages in fp32"""
    M, N, K = T.conv_mnk(c)
    x, dy, bw, bb = T.conv_inputs(c)
    prod, col = T.conv_products(c)
    cols = T.conv_im2col(c)
    assert cols.shape == (M, K) and prod.shape == (N, K)
    assert float(cols.abs().max()) <= 3 and float(dy.abs().min()) >= 1 and 2 * 9 * M + 8 < 2 ** 24
    for order in _orders(T.cdiv(M, 64)):
        acc, cs = T.tn_reference_f32(dy, cols, order)
        assert torch.equal(acc.double(), prod) and torch.equal(cs.double(), col)


def test_the_long_conv_cases_stay_inside_the_bound():
    big = [c for c in T.CONV_CASES if T.conv_mnk(c)[0] >= 32768]
    assert len(big) == 4 and all(T.conv_mnk(c)[0] <= T.M_BOUND for c in big)


def test_group_problems_are_exact():
    for c in T.GROUP_CASES:
        for i, p in enumerate(c.problems):
            dy, x, bw, bb, prod, col = T.prob_inputs(p, i)
            acc, cs = T.tn_reference_f32(dy, x, list(reversed(range(T.cdiv(p.M, 64)))))
            assert torch.equal(acc.double()[:p.n_store], prod) and torch.equal(cs.double()[:p.n_store], col) and float(dy.abs().min()) >= 1


def test_a_dropped_or_doubled_row_stage_or_split_changes_the_reference():
    """the net's mesh.  No operand holds a zero, so ONE missing or doubled row moves every element of dW and db.  A 64-row stage or a whole split is a sum of such
    terms and can cancel in single elements (at 64 rows about one element in a hundred): losing or doubling it must change at least 90 % of the stored dW elements and
    of the db elements (half of them where fewer than 32 rows are stored: three elements prove no fraction), compared as `ref - part != ref` and `ref + part != ref`."""
    for M in (193, 1025, 2049):
        c = [c for c in T.TN_CASES if c.variant == 0 and c.M == M][0]
        p = T.tn_case_plan(c)
        dy, x, _, _ = T.tn_inputs(c)
        ref_w, ref_b = T.tn_reference(c)
        for r in (0, c.M // 2, c.M - 1):
            one = torch.outer(dy[r], x[r])[:c.n_store]
            assert bool((one != 0).all()) and bool((dy[r] != 0).all())
            assert bool((ref_w - one != ref_w).all()) and bool((ref_w + one != ref_w).all()) and bool((ref_b - dy[r][:c.n_store] != ref_b).all())
        live = [s for s, n in enumerate(p.rows) if n > 0]
        for s in (live[0], live[-1]):
            lo = s * p.rps
            for rows in (slice(lo, lo + min(64, p.rows[s])), slice(lo, lo + p.rows[s])):          # the split's first stage; the whole split
                part, pcol = (dy[rows].t() @ x[rows])[:c.n_store], dy[rows].sum(0)[:c.n_store]
                for sign in (-1, 1):                       # dropped; doubled
                    assert float((ref_w + sign * part != ref_w).double().mean()) >= 0.9 and float((ref_b + sign * pcol != ref_b).double().mean()) >= (0.9 if c.n_store >= 32 else 0.5)
                    assert not torch.equal((ref_w + sign * part).float(), ref_w.float())


def _check_bg_exact(a, b, alpha, ref_prod):
    K = a.shape[-1]
    assert K <= T.BG_KBIG and 9 * K + 8 < 2 ** 24 and float(a.abs().max()) <= 3 and float(b.abs().max()) <= 3 and alpha in (1.0, 0.5)
    a32, b32 = a.float(), b.float()
    for order in _orders(T.cdiv(K, 32)):
        acc = torch.zeros(ref_prod.shape, dtype=torch.float32)
        for i in order:
            acc = acc + torch.einsum("abmk,abnk->abmn", a32[..., 32 * i:32 * i + 32], b32[..., 32 * i:32 * i + 32])
        assert torch.equal(acc.double(), ref_prod)


@pytest.mark.parametrize("c", [c for c in T.BG_CASES if c.Z1 * c.Z2 <= 6 or c.K in (33, 129)], ids=lambda c: c.id)
def test_bgemm_case_is_exact_in_any_k_order(c):
    a, b, base = T.bg_inputs(c)
    ref = T.bg_reference(c)
    prod = torch.einsum("abmk,abnk->abmn", a, b)
    _check_bg_exact(a, b, c.alpha, prod)
    assert torch.equal(ref, c.alpha * prod + (base if c.accumulate else 0))
    assert float(ref.abs().max()) < 2 ** 24 and torch.equal(ref.float().double(), ref) and torch.equal(ref * 2, (ref * 2).round())
    exp = T.bg_expected(ref, c.out_f32)
    if c.out_f32:
        assert exp.dtype == torch.float32 and torch.equal(exp.double(), ref)
    else:
        # the kernel's bf16 path: v = fp32(alpha * acc); v += fp32(bf16 C); f2bf(v) — every step before the cast exact
        v = torch.tensor(c.alpha, dtype=torch.float32) * prod.float()
        if c.accumulate:
            assert torch.equal(base.to(torch.bfloat16).double(), base)
            v = v + base.to(torch.bfloat16).float()
        assert exp.dtype == torch.bfloat16 and torch.equal(exp, v.to(torch.bfloat16))


def test_every_bgemm_case_meets_its_bound():
    """the cheap part of the check above over the whole table (the any-order fp32 walk stays on the subset): K, the operand ranges, and a reference that is a multiple
    of 0.5 below 2**24, i.e. exactly representable in fp32"""
    for c in T.BG_CASES:
        a, b, base = T.bg_inputs(c)
        ref = T.bg_reference(c)
        assert c.K <= T.BG_KBIG and c.alpha in (1.0, 0.5) and a.shape == (c.Z1, c.Z2, c.M, c.K) and b.shape == (c.Z1, c.Z2, c.N, c.K), c.id
        assert float(a.abs().max()) <= 3 and float(b.abs().max()) <= 3 and (base is None or float(base.abs().max()) <= 8), c.id
        assert float(ref.abs().max()) <= 9 * c.K + 8 < 2 ** 24 and torch.equal(ref * 2, (ref * 2).round()) and torch.equal(ref.float().double(), ref), c.id


def test_every_group_problem_meets_its_bound():
    for c in T.GROUP_CASES:
        assert 1 <= len(c.problems) <= T.TN_GROUP
        for i, p in enumerate(c.problems):
            dy, x, bw, bb, prod, col = T.prob_inputs(p, i)
            assert p.M <= T.M_BOUND and 2 * 9 * p.M + 8 < 2 ** 24 and 1 <= p.n_store <= p.N, (c.id, i)
            assert float(dy.abs().min()) >= 1 and float(x.abs().min()) >= 1 and float(dy.abs().max()) <= 3 and float(x.abs().max()) <= 3, (c.id, i)
            assert float(bw.abs().max()) <= 8 and float(bb.abs().max()) <= 8 and float(prod.abs().max()) <= 9 * p.M and float(col.abs().max()) <= 3 * p.M, (c.id, i)
            assert torch.equal(prod, (dy.t() @ x)[:p.n_store]) and torch.equal(col, dy.sum(0)[:p.n_store]), (c.id, i)


def test_band_and_dead_row_references_are_exact():
    for c in T.BAND_CASES:
        dbd, qv = T.band_inputs(c)
        off, Kp = T.band_geometry(c.Tt)
        assert c.cg * c.Tt <= T.BG_KBIG and float(dbd.abs().max()) <= 3 and float(qv.abs().max()) <= 3 and dbd.shape[-1] == Kp
        for i in (0, c.Tt - 1):                                # the band of row i, and true zeros outside it
            assert float(dbd[:, :, i, :c.Tt - 1 - i + off].abs().max() if c.Tt - 1 - i + off else 0.0) == 0 and float(dbd[:, :, i, 2 * c.Tt - 1 - i + off:].abs().sum()) == 0
        ref = T.band_reference(c)
        assert torch.equal(ref.float().double(), ref) and float(ref.abs().max()) <= 9 * c.cg * c.Tt < 2 ** 24
        # the same sums with the utterances of a group walked last to first, in fp32
        d32, q32 = dbd.float().view(c.H, c.G, c.cg, c.Tt, Kp), qv.float().view(c.G, c.cg, c.Tt, c.H, c.hd)
        acc = torch.zeros(c.G, Kp, c.H, c.hd)
        for u in reversed(range(c.cg)):
            acc = acc + torch.einsum("hbip,bihc->bphc", d32[:, :, u], q32[:, u])
        assert torch.equal(acc.reshape(c.G, -1).double(), ref)
    for c in T.MV_CASES:
        a, b, base = T.mv_inputs(c)
        ref = T.mv_reference(c)
        assert torch.equal(ref.float().double(), ref) and c.K <= T.BG_KBIG and float(ref.abs().max()) <= 9 * c.K + 8 < 2 ** 24
        assert float(a.abs().max()) <= 3 and float(b.abs().max()) <= 3 and float(base.abs().max()) <= 8
        tile = T.mv_form(c)
        assert set(c.lens) >= {0, 1, tile - 1, tile, tile + 1, c.M}
        for z, n in enumerate(c.lens):
            assert float(a[:, z, n:].abs().sum()) == 0 and T.mv_dead_rows(c, z) % tile in (0, c.M % tile)
            if not c.accumulate:
                assert float(ref[:, z, n:].abs().sum()) == 0


# ----------------------------------------------------------------------------------------------------------------- coverage
def test_weight_gradient_table_reaches_every_form_stage_count_ragged_class_and_split_class():
    plans = {c.id: T.tn_case_plan(c) for c in T.TN_CASES}
    assert {p.form for p in plans.values()} == {"t128-desc", "t128x64-desc", "t128-ptr", "big-desc", "big-ptr"}
    for variant, form in ((0, "t128-desc"), (1, "t128x64-desc")):
        mine = [c for c in T.TN_CASES if c.variant == variant and plans[c.id].form == form and c.M <= 1025]
        assert {c.M for c in mine} == set(T.M_SINGLE + T.M_SPLIT)
        single = [c for c in mine if plans[c.id].splits == 1]
        assert {c.M for c in single} == set(T.M_SINGLE)
        assert {plans[c.id].stages[0] for c in single} == {1, 2, 3, 4}                              # below, at and beyond the two-stage ring's depth
        assert {plans[c.id].last_rows[0] for c in single} >= {1, 15, 16, 17, 63, 64}                # one row; one short of / exactly / one past a 16-row k-step; 63; whole
        assert {c.M: plans[c.id].splits for c in mine if c.M in T.M_SPLIT} == {257: 2, 513: 3, 1025: 5}
        assert plans[[c for c in mine if c.M == 1025][0].id].rows[-1] == 1
        assert {c.N for c in mine} == set(T.NK_EDGES) and {c.K for c in mine} == set(T.NK_EDGES)
        assert {(c.n_store == c.N, c.n_store == c.N - 5, c.n_store == 1) for c in mine} >= {(True, False, False), (False, True, False), (False, False, True)}
        assert {c.db for c in mine} == {False, True} and {c.views for c in mine} == {False, True}
        assert {c.views for c in mine if plans[c.id].splits > 1} == {False, True}
    # a split with no rows at all
    e = plans["v0-2049x1024x1024-ns1019-db-views"]
    assert e.form == "t128-desc" and e.splits == 8 and e.rps == 320 and e.rows[-1] < 0 and e.rows[-2] == 129 and e.stages[-1] == 0 and e.empty
    # the 256 x 256 tile: every M x (N, K) of the issue, db on and off, n_store < N; and one row fewer on the 128 tile
    big = [c for c in T.TN_CASES if plans[c.id].form == "big-desc"]
    assert {(c.M, c.N, c.K) for c in big} == {(M, N, K) for M in T.BIG_M for N, K in T.BIG_NK}
    assert {c.db for c in big} == {False, True} and all(c.n_store < c.N for c in big)
    assert {plans[c.id].last_rows[plans[c.id].splits - 1] for c in big if not plans[c.id].empty} >= {64, 1, 17}
    assert any(plans[c.id].empty for c in big)
    assert {(c.N, c.K) for c in T.TN_CASES if c.M == 32767 and plans[c.id].form == "t128-desc"} == set(T.BIG_NK)
    # the per-lane pointer fallback on both tiles
    ptr = {plans[c.id].form: c for c in T.TN_CASES if c.xwide}
    assert set(ptr) == {"t128-ptr", "big-ptr"} and ptr["t128-ptr"].N == 128 and (ptr["big-ptr"].M, ptr["big-ptr"].N, ptr["big-ptr"].K) == (32776, 256, 256)
    assert all(c.xwide == 65544 and T.tn_layout(c).x_off % 8 == 0 and T.tn_layout(c).x_off + c.K + 8 <= c.xwide for c in ptr.values())


def test_conv_table_reaches_both_gathered_forms_and_every_wrap_class():
    plans = {c.id: T.conv_plan(c) for c in T.CONV_CASES}
    small = [c for c in T.CONV_CASES if T.conv_mnk(c)[0] < 32768]
    assert all(plans[c.id].form == "t128-gather" for c in small)
    assert {c.Cin for c in small} == {128, 256} and {c.Fout for c in small} >= {1, 7, 19, 64, 70}
    assert {(c.pad_t, c.pad_f) for c in small} >= {(0, 0), (1, 1), (2, 2), (1, 0), (2, 0)} and {(c.KH, c.KW) for c in small} == {(3, 3), (3, 1)}
    assert {T.conv_mnk(c)[0] for c in small} >= {1, 63, 65, 257} and all(c.stride == 2 for c in T.CONV_CASES)
    assert any(plans[c.id].splits > 1 for c in small) and any(c.trail for c in small) and {c.db for c in small} == {False, True}
    big = [c for c in T.CONV_CASES if plans[c.id].form == "big-gather"]
    assert len(big) == 2 and all(c.Cin == 256 and c.Cout >= 256 for c in big) and 32768 in {T.conv_mnk(c)[0] for c in big} and any(T.conv_mnk(c)[0] > 32768 for c in big)
    for c in big:                                            # the same geometry at Cin = 128: `big` refused, the 128 tile runs
        twin = [d for d in T.CONV_CASES if d.Cin == 128 and (d.B, d.Tout, d.Fout, d.Cout, d.KH, d.KW) == (c.B, c.Tout, c.Fout, c.Cout, c.KH, c.KW)]
        assert len(twin) == 1 and plans[twin[0].id].form == "t128-gather"


def test_group_table_reaches_every_stage_count_block_count_and_problem_count():
    for xw, ring in ((128, 3), (256, 2)):
        mine = [c for c in T.GROUP_CASES if c.tile_k == xw]
        assert all(T.group_plan(c)[:2] == (xw, ring) for c in mine)
        probs = [p for c in mine for p in c.problems]
        assert {p.M for p in probs if True} == set(T.GROUP_M)
        assert {T.cdiv(p.M, 64) for p in probs} == {1, 2, 3, 4, 5}                                  # below, at and beyond either ring depth
        assert {p.M % 64 for p in probs} >= {1, 63, 0}
        assert {sum(T.group_plan(c)[2]) for c in mine} >= {1, 7, 8, 9, 13} and {len(c.problems) for c in mine} == {1, 2, 3, 47, 48}
        assert any(sum(T.group_plan(c)[2]) % 8 for c in mine if len(c.problems) >= 47)
        assert {c.overwrite for c in mine} == {False, True} and {p.N for p in probs} >= {8, 264} and {p.db for p in probs} == {False, True}
        for c in mine:
            if len(c.problems) > 1:
                assert {p.db for p in c.problems} == {False, True}, c.id                            # db for some problems only
    auto = {T.group_plan(c)[0]: c for c in T.GROUP_CASES if c.tile_k == 0}
    assert set(auto) == {128, 256} and len(auto[256].problems) == 48
    assert sum(T.cdiv(p.N, 256) * T.cdiv(p.K, 256) for p in auto[256].problems) >= 200 > sum(T.cdiv(p.N, 256) * T.cdiv(p.K, 256) for p in auto[128].problems)


def test_the_block_permutation_of_the_grouped_launch_is_a_bijection():
    for nwg in list(range(1, 70)) + [288, 511, 513]:
        assert sorted(T.group_permute(b, nwg) for b in range(nwg)) == list(range(nwg)), nwg


def test_bgemm_table_reaches_all_sixteen_instantiations_at_every_k_edge():
    forms = {}
    for c in T.BG_CASES:
        forms.setdefault((c.la, c.lb) + T.bg_form(c), []).append(c)
    assert set(forms) == {(la, lb, tile, fast) for la in (0, 1) for lb in (0, 1) for tile in (64, 128) for fast in (False, True)}
    for key, mine in forms.items():
        assert {c.K for c in mine} >= set(T.BG_K), key
        assert {c.out_f32 for c in mine} == {False, True} and {c.alpha for c in mine} == {1.0, 0.5} and {c.accumulate for c in mine} == {False, True}, key
        assert {c.c_view for c in mine} == {False, True} and {c.zswap for c in mine} == {False, True}, key
    for tile in (64, 128):
        mine = [c for k, v in forms.items() if k[2] == tile for c in v]
        assert {c.M for c in mine} >= ({65, 127, 128, 129, 130} if tile == 128 else set(T.BG_MN)) and {c.N for c in mine} >= ({65, 127, 128, 129, 130} if tile == 128 else set(T.BG_MN))
        assert T.BG_KBIG in {c.K for c in mine}
        guarded = [c for k, v in forms.items() if k[2] == tile and not k[3] for c in v]
        assert {c.guard for c in guarded} == {"a_off4", "b_off4", "a_ragged", "b_ragged"}
        fast = [c for k, v in forms.items() if k[2] == tile and k[3] for c in v]
        assert {c.pad for c in fast} == {0, 8}
        # branch-free by extents that are multiples of 8 and by padded strides
        assert any((c.K if c.la == 0 else c.M) % 8 == 0 for c in fast) and any((c.K if c.la == 0 else c.M) % 8 for c in fast)
    assert {c.Z1 * c.Z2 for c in T.BG_CASES if T.bg_form(c)[0] == 128} == {64, 256}
    # the k-tile skipping exists in the branch-free instantiation only: every (Tt, cg) must run THERE on the 64 tile; the guarded walk and the 128 tile are extra cases
    assert {(c.Tt, c.cg) for c in T.BAND_CASES if T.band_form(c) == (64, True)} == {(t, g) for t in (31, 32, 33, 64, 65, 97) for g in (1, 2, 3)}
    assert [(c.Tt, c.cg, c.hd, c.H * c.G) for c in T.BAND_CASES if T.band_form(c) == (128, True)] == [(250, 1, 128, 64)]
    assert [(c.Tt, c.cg) for c in T.BAND_CASES if T.band_form(c) == (64, False)] == [(65, 2)] and len(T.BAND_CASES) == 20
    assert {(T.mv_form(c), c.accumulate) for c in T.MV_CASES} == {(64, False), (64, True), (128, False), (128, True)}


# ----------------------------------------------------------------------------------------------------------------- the restated dispatch, value by value
def test_restated_weight_gradient_dispatch_is_pinned_at_its_thresholds():
    assert not T.tn_big(32767, 256, 256) and T.tn_big(32768, 256, 256)
    assert not T.tn_big(32768, 255, 256) and not T.tn_big(32768, 256, 255) and not T.tn_big(32768, 248, 256) and not T.tn_big(32768, 256, 248)
    assert T.tn_splits(256, 8, 8, 0) == 1 and T.tn_splits(257, 8, 8, 0) == 2 and T.tn_splits(513, 264, 264, 0) == 3 and T.tn_splits(1025, 264, 264, 1) == 5
    assert T.tn_splits(8000, 512, 512, 0) == 32 and T.tn_splits(8000, 512, 512, 1) == 24 and T.tn_splits(48000, 512, 2304, 2) == 14          # 512 / 768 / 256 blocks
    assert T.tn_splits(2049, 1024, 1024, 0) == 8 and T.rows_per_split(2049, 8) == 320 and 7 * 320 > 2049                                 # the empty split
    assert T.rows_per_split(257, 2) == 192 and T.rows_per_split(1025, 5) == 256 and T.rows_per_split(64, 1) == 64 and T.rows_per_split(65, 1) == 128
    assert T.tn_splits(32768, 256, 256, 2) == 128 and T.tn_splits(32769, 256, 256, 2) == 129 and T.tn_splits(33553, 256, 256, 2) == 132
    # the 4 GiB bound: M * max(ldy, ldx) * 2 < 2**32 - 4096
    assert T.FAST_LIMIT == 4294963200
    assert T.fast_ok(32763, 8, 65544) and not T.fast_ok(32764, 8, 65544) and not T.fast_ok(32776, 152, 65544) and T.fast_ok(32776, 152, 65512)
    assert T.fast_ok(1, 8, (T.FAST_LIMIT - 2) // 2) and not T.fast_ok(1, T.FAST_LIMIT // 2, 8)
    assert not T.fast_ok(64, 8, 8, conv=True) and not T.fast_ok(64, 8, 8, gathered_big=True)
    # the gathered form takes the big tile only at Cin % 256 == 0
    assert T.tn_plan(32768, 256, 2304, 0, 256, 256, conv_cin=256).form == "big-gather" and T.tn_plan(32768, 256, 1152, 0, 256, 128, conv_cin=128).form == "t128-gather"
    assert T.tn_plan(32768, 256, 1152, 0, 256, 384, conv_cin=384).form == "t128-gather" and T.tn_plan(32767, 256, 2304, 0, 256, 256, conv_cin=256).form == "t128-gather"
    assert T.tn_plan(32768, 256, 256, 1, 256, 256).form == "t128x64-desc"                                                               # variant 1 never takes it
    # the grouped launch's tile
    assert T.group_xw(128, [(1, 8, 8)]) == 128 and T.group_xw(256, [(1, 8, 8)]) == 256
    assert T.group_xw(0, [(65, 264, 520)] * 33) == 128 and T.group_xw(0, [(65, 264, 520)] * 34) == 256                                  # 198 / 204 tiles of 256 x 256
    assert T.group_xw(0, [(65, 256, 256)] * 48) == 128


def test_restated_bgemm_dispatch_is_pinned_at_its_thresholds():
    assert T.bg_blocks128(130, 130, 64) == 256 and T.bg_tile(130, 130, 64) == 128 and T.bg_blocks128(130, 130, 63) == 252 and T.bg_tile(130, 130, 63) == 64
    assert T.bg_blocks128(128, 128, 255) == 255 and T.bg_tile(128, 128, 255) == 64 and T.bg_tile(128, 128, 256) == 128
    assert T.bg_tile(64, 128, 256) == 64 and T.bg_tile(128, 64, 256) == 64 and T.bg_tile(65, 65, 256) == 128
    assert T.bg_tile(512, 128, 64) == 128 and T.bg_tile(512, 64, 64) == 64                                                               # the band product at hd 128 / 64
    f = T.bg_operand_fast
    assert f(0, 8, 8, 96, 1, 70, 90) and not f(0, 8, 8, 90, 1, 70, 90) and f(0, 8, 8, 88, 1, 70, 88) and not f(0, 8, 8, 88, 1, 70, 90)   # k-contiguous: padded / ragged / whole / too short
    assert not f(4, 8, 8, 96, 1, 70, 90) and f(8, 8, 8, 96, 1, 70, 90) and not f(0, 4, 8, 96, 1, 70, 90) and not f(0, 8, 12, 96, 1, 70, 90)
    assert f(0, 8, 8, 1, 72, 70, 90) and not f(0, 8, 8, 1, 70, 70, 90) and f(0, 8, 8, 1, 64, 64, 90) and not f(0, 8, 8, 1, -72, 70, 90)  # row-contiguous: the extent is R


# ----------------------------------------------------------------------------------------------------------------- refusals before any launch
@pytest.fixture(scope="module")
def lib():
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.csrc import build as B
    B.build()
    return _lib.lib()


FAKE = 0x10000                       # 16-B aligned; never dereferenced: every call below is refused before a launch


def _group_args(n, edits, tile_k, overwrite=0):
    m = max(n, 1)
    arr = {"ldy": [136] * m, "ldx": [264] * m, "ldo": [264] * m, "M": [65] * m, "N": [136] * m, "K": [264] * m, "n_store": [131] * m}
    ptr = {"dY": [FAKE] * m, "X": [FAKE] * m, "dW": [FAKE] * m, "db": [None] * m}
    for name, e in edits.items():
        for i, v in e.items():
            (arr if name in arr else ptr)[name][i] = v
    vp, lg, it = (C.c_void_p * m), (C.c_long * m), (C.c_int * m)
    return (n, vp(*ptr["dY"]), lg(*arr["ldy"]), vp(*ptr["X"]), lg(*arr["ldx"]), vp(*ptr["dW"]), lg(*arr["ldo"]), vp(*ptr["db"]),
            it(*arr["M"]), it(*arr["N"]), it(*arr["K"]), it(*arr["n_store"]), tile_k, overwrite, None)


GROUP_MORE = {"a null dW": (3, {"dW": {1: None}}, 128), "dY not 16-B aligned": (3, {"dY": {0: FAKE + 8}}, 128), "ldo = 2**31": (3, {"ldo": {2: 2 ** 31}}, 256),
              "M = 0": (3, {"M": {2: 0}}, 0), "K % 8": (3, {"K": {0: 260}}, 0)}


@pytest.mark.parametrize("what", list(T.GROUP_REFUSALS) + list(GROUP_MORE))
def test_grouped_entry_refuses(lib, what):
    n, edits, tile_k = {**T.GROUP_REFUSALS, **GROUP_MORE}[what]
    for ow in (0, 1):
        assert lib.mi_gemm_tn_group_ow_bf16(*_group_args(n, edits, tile_k, ow)) == T.ARG, what
    a = _group_args(n, edits, tile_k)
    assert lib.mi_gemm_tn_group_bf16(*a[:13], None) == T.ARG, what


TN_BASE = dict(dY=FAKE, ldy=136, X=FAKE, ldx=264, dW=FAKE, ldo=264, db=None, M=65, N=136, K=264, n_store=131, ws=None, ws_bytes=0, variant=0)
TN_REFUSALS = {"M = 0": dict(M=0), "N % 8": dict(N=132, n_store=131), "K % 8": dict(K=260), "ldy % 8": dict(ldy=140), "ldx % 8": dict(ldx=268), "n_store > N": dict(n_store=137),
               "n_store = 0": dict(n_store=0), "variant 2": dict(variant=2), "variant -1": dict(variant=-1), "dY not 16-B aligned": dict(dY=FAKE + 8), "X not 16-B aligned": dict(X=FAKE + 4),
               "two splits without a workspace": dict(M=257), "a workspace one byte short": dict(M=257, ws=FAKE, ws_bytes=2 * 136 * 265 * 4 - 1)}


@pytest.mark.parametrize("what", list(TN_REFUSALS))
def test_weight_gradient_entry_refuses(lib, what):
    a = {**TN_BASE, **TN_REFUSALS[what]}
    assert lib.mi_gemm_tn_bf16(*[a[k] for k in TN_BASE], None) == T.ARG, what
    assert lib.mi_gemm_tn_workspace_bytes(257, 136, 264) == 2 * 136 * 265 * 4 and lib.mi_gemm_tn_workspace_bytes(256, 136, 264) == 0


BG_BASE = dict(A=FAKE, a_z1=0, a_z2=0, a_m=96, a_k=1, B=FAKE, b_z1=0, b_z2=0, b_n=96, b_k=1, C=FAKE, c_z1=0, c_z2=0, c_m=64, out_f32=1, accumulate=0, alpha=1.0,
               Z1=1, Z2=1, M=64, N=64, K=90, band_T=0, band_a=0, band_cg=0, m_valid=None)
BG_REFUSALS = {"Z1 = 0": (dict(Z1=0), T.ARG), "M = 0": (dict(M=0), T.ARG), "K = 0": (dict(K=0), T.ARG), "more than 65535 batch entries": (dict(Z1=256, Z2=256), T.ARG),
               "A with neither stride 1": (dict(a_m=96, a_k=2), T.UNSUPPORTED), "B with neither stride 1": (dict(b_n=2, b_k=96), T.UNSUPPORTED),
               "band_T < 0": (dict(band_T=-1), T.ARG), "a band without utterances": (dict(band_T=90, band_cg=0), T.ARG), "band_cg * band_T != K": (dict(band_T=44, band_cg=2), T.ARG)}


@pytest.mark.parametrize("what", list(BG_REFUSALS))
def test_bgemm_entry_refuses(lib, what):
    edits, code = BG_REFUSALS[what]
    a = {**BG_BASE, **edits}
    assert lib.mi_bgemm_sparse_bf16(*[a[k] for k in BG_BASE], None) == code, what
