"""The references of tests/dwconv_ref.py checked on their own, without a GPU: the closed-form backwards against torch.autograd of the oracle's depthwise conv, the
integer cases' exact representability (the condition that lets tests/test_gpu_dwconv.py demand equality), and the coverage of the case table."""

import pytest
import torch
import torch.nn.functional as F

import dwconv_ref as D
from oracle import ebranchformer_ref as R

F64 = torch.float64
EPS = 1e-5


def _rel(got, want):
    return float((got - want).abs().max()) / max(float(want.abs().max()), 1e-300)


def _geometries():
    """every (K, pad, dilation) of CASES, once"""
    return sorted({(c.K, c.pad, c.dil) for c in D.CASES})


def _oracle_conv(x, w, bias, B, T, K, pad, dil):
    """the oracle's conv on (B*T, C): symmetric, or causal (left pad (K - 1) dil) — the only two geometries the model has, and all that CASES holds"""
    C = x.shape[1]
    if dil == 1 and pad == (K - 1) // 2 and K % 2 == 1:
        y = R.dwconv1d(x.view(B, T, C), w.view(C, 1, K), bias, False, 1)
    else:
        assert pad == (K - 1) * dil, "CASES holds a geometry the oracle cannot express"
        y = R.dwconv1d(x.view(B, T, C), w.view(C, 1, K), bias, True, dil)
    return y.reshape(B * T, C)


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


@pytest.mark.parametrize("K,pad,dil", _geometries())
@pytest.mark.parametrize("T", [1, 7, 40])
def test_closed_forms_agree_with_autograd(K, pad, dil, T):
    B, C = 3, 5
    T = T if dil == 1 else T * 14                                  # the dilated geometries: below one tap step, below the reach, above it (14, 98, 560)
    M = B * T
    u, ds = _rand((M, 2 * C), 1), _rand((M, C), 2)
    gamma, beta, w, bias = 1 + 0.1 * _rand((C,), 3), 0.1 * _rand((C,), 4), _rand((C, K), 5), _rand((C,), 6)
    stats = D.row_stats(u[:, C:], EPS)
    for gated in (True, False):
        ur, gr, ber, wr, br = [t.clone().requires_grad_(True) for t in (u, gamma, beta, w, bias)]
        gn = F.layer_norm(ur[:, C:], (C,), gr, ber, EPS)
        gn.retain_grad()
        cv = _oracle_conv(gn, wr, br, B, T, K, pad, dil)
        out = ur[:, :C] * cv if gated else cv
        out.backward(ds)
        got_f, got_cv = D.csgu_fwd(u, stats, gamma, beta, w, bias, B, T, pad, dil, 0, gated=gated, parts=True)
        got = D.csgu_bwd(u, stats, gamma, beta, w, bias, ds, B, T, pad, dil, gated=gated)
        assert _rel(got_f, out.detach()) < 1e-12 and _rel(got_cv, cv.detach()) < 1e-12 and _rel(got["conv"], cv.detach()) < 1e-12
        assert _rel(got["dgn"], gn.grad) < 1e-12
        assert _rel(got["dw"], wr.grad) < 1e-12 and _rel(got["db"], br.grad) < 1e-12
        if gated:
            assert _rel(got["dr"], ur.grad[:, :C]) < 1e-12
        else:
            assert got["dr"] is None and float(ur.grad[:, :C].abs().max()) == 0.0
    if dil == 1:                                                   # the merge conv is never dilated (mi_dwconv_residual_bf16 has no dilation argument)
        m, dy = _rand((M, C), 7), _rand((M, C), 8)
        mr, wr, br = [t.clone().requires_grad_(True) for t in (m, w, bias)]
        y = mr + _oracle_conv(mr, wr, br, B, T, K, pad, 1)
        y.backward(dy)
        got = D.merge_bwd(m, w, dy, B, T, pad)
        assert _rel(D.merge_fwd(m, w, bias, B, T, pad), y.detach()) < 1e-12
        assert _rel(got["dm"], mr.grad) < 1e-12 and _rel(got["dw"], wr.grad) < 1e-12 and _rel(got["db"], br.grad) < 1e-12


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_activations_agree_with_torch_and_autograd(act):
    tfn = {0: lambda v: v, 1: F.gelu, 2: F.relu, 3: F.silu}[act]
    r, g, ds = _rand((7, 11), 1), 2 * _rand((7, 11), 2), _rand((7, 11), 3)
    rr, gg = r.clone().requires_grad_(True), g.clone().requires_grad_(True)
    s = rr * tfn(gg)
    s.backward(ds)
    assert _rel(D.gate_act_mul(r, g, act), s.detach()) < 1e-12
    dr, dg = D.gate_act_mul_bwd(r, g, ds, act)
    assert _rel(dr, rr.grad) < 1e-12 and _rel(dg, gg.grad) < 1e-12
    # the fused activation of the CSGU forward
    B, T, C, K = 2, 9, 4, 3
    u, w, bias = _rand((B * T, 2 * C), 4), _rand((C, K), 5), _rand((C,), 6)
    gamma, beta = 1 + 0.1 * _rand((C,), 7), 0.1 * _rand((C,), 8)
    want = u[:, :C] * tfn(_oracle_conv(F.layer_norm(u[:, C:], (C,), gamma, beta, EPS), w, bias, B, T, K, 1, 1))
    assert _rel(D.csgu_fwd(u, D.row_stats(u[:, C:], EPS), gamma, beta, w, bias, B, T, 1, 1, act), want) < 1e-12


def test_gelu_fit_is_within_its_documented_error_of_the_erf_form():
    """the forward GELU of the kernels is a fit (csrc/common.hpp gelu_erf); its approximation error, from the formula alone, is what the GPU tests allow act 1 on top
    of the rounding terms"""
    x = torch.linspace(-12.0, 12.0, 2_400_001, dtype=F64)
    err = (D.gelu_fit(x) - D.act_fn(x, 1)).abs()
    assert float(err.max()) <= D.GELU_FIT_ERR
    assert float(err.max()) > 0.5 * D.GELU_FIT_ERR              # and the figure is not slack: the fit does come that close to it


def test_row_stats_agrees_with_torch():
    x = 3 + 2 * _rand((6, 72), 1)
    st = D.row_stats(x, EPS)
    var, mean = torch.var_mean(x, dim=1, unbiased=False)
    assert _rel(st[:, 0], mean) < 1e-12 and _rel(st[:, 1], torch.rsqrt(var + EPS)) < 1e-12
    gamma, beta = _rand((72,), 2), _rand((72,), 3)
    assert _rel(D.ln_given(x, st, gamma, beta), F.layer_norm(x, (72,), gamma, beta, EPS)) < 1e-12


def _is_small_int(t, bound):
    return bool((t == t.round()).all()) and float(t.abs().max()) < bound


@pytest.mark.parametrize("case", D.CASES, ids=lambda c: c.name)
def test_integer_cases_are_exact_in_bf16_and_fp32(case):
    """every output and every intermediate of an integer case is an integer below 256 (bf16 holds it), every tap / bias gradient below 2**24 (fp32 sums it exactly)"""
    inp = D.int_inputs(case)
    for k, v in inp.items():
        assert _is_small_int(v, 3), k
        assert torch.equal(v.to(torch.bfloat16).to(F64), v)
    for act in ((0, 2) if case.op == "csgu" else (0,)):
        fwd = D.reference(case, inp, act=act)["fwd"]
        assert _is_small_int(fwd, 256)
        assert torch.equal(fwd.to(torch.bfloat16).to(F64), fwd)
    bwd = D.reference(case, inp)["bwd"]                             # identity activation: the backward kernels have no other
    for k in ("dr", "dgn", "dm", "conv", "dyc"):
        if bwd.get(k) is not None:
            assert _is_small_int(bwd[k], 256), k
            assert torch.equal(bwd[k].to(torch.bfloat16).to(F64), bwd[k]), k
    for k in ("dw", "db", "S", "Sb"):
        assert _is_small_int(bwd[k], 2 ** 24), k
    # the same reference evaluated in fp32 gives the same integers: nothing in it rounds
    ref32 = D.reference(case, inp, act=0, dtype=torch.float32)
    assert torch.equal(ref32["fwd"].to(F64), D.reference(case, inp, act=0)["fwd"])
    assert torch.equal(ref32["bwd"]["dw"].to(F64), bwd["dw"])
    if case.B > 1:                                                  # utterance isolation can only show if every utterance holds data
        x = inp["m"] if case.op == "merge" else inp["u"]
        assert all(bool(x.view(case.B, case.T, -1)[b].abs().sum() > 0) for b in range(case.B))
    for k in D.dead_taps(case):
        assert float(bwd["dw"][:, k].abs().max()) == 0.0


def test_every_reachable_form_and_op_has_two_cases():
    """the dispatcher reaches: fast x {gated, merge} (its predicate rejects the split form), generic x {gated, split, merge}, dilated x {gated, split}
    (the merge entry points have no dilation: ops.dwconv_residual / ops_train.dwconv_residual_bwd always pass 1)"""
    reachable = {("fast", "csgu"), ("fast", "merge"), ("generic", "csgu"), ("generic", "split"), ("generic", "merge"), ("dilated", "csgu"), ("dilated", "split")}
    cells = {}
    for c in D.CASES:
        fwd, bwd = D.forms(c)
        assert (fwd == "fast") == (bwd == "fast"), c.name          # the two fast predicates agree on the tests' layouts
        assert fwd == "generic" or bwd == "fast"
        cells.setdefault((bwd, c.op), []).append(c.name)            # a case sits in exactly one cell
    assert set(cells) == reachable, sorted(set(cells) ^ reachable)
    for cell, names in cells.items():
        assert len(names) >= 2 and len(set(names)) == len(names), (cell, names)
    assert sum(len(v) for v in cells.values()) == len(D.CASES)


def test_forms_restate_the_dispatch_predicates():
    mk = D._c
    assert D.forms(mk("a", "csgu", 2, 65, 64)) == ("fast", "fast")
    assert D.forms(mk("b", "split", 2, 65, 64)) == ("generic", "generic")                  # no gate operand
    assert D.forms(mk("c", "merge", 2, 65, 64, view="slice64")) == ("fast", "fast")        # ld != C is fine
    assert D.forms(mk("d", "merge", 2, 65, 64, view="off4")) == ("generic", "generic")     # 8-B aligned pointer
    assert D.forms(mk("e", "merge", 2, 65, 72)) == ("generic", "generic")                  # C % 64
    assert D.forms(mk("f", "csgu", 2, 65, 64, K=15)) == ("generic", "generic")
    assert D.forms(mk("g", "merge", 2, 65, 64, pad=30)) == ("generic", "generic")          # K 31 with a causal pad
    assert D.forms(mk("h", "csgu", 2, 65, 64, pad=450, dil=15)) == ("generic", "dilated")
    for c in D.CASES:                                                                       # names say what the case is meant to reach
        want = "fast" if c.name.startswith("fast-") else "dilated" if c.name.startswith("dil") else "generic"
        assert D.forms(c)[1] == want, c.name


def test_every_listed_edge_appears_in_every_form_that_admits_it():
    need = {
        "fast": {"T=1", "T=15", "T=16", "T=31", "T=63", "T=64", "T=65", "T=150", "B=1", "B=2", "B=3", "slice"},
        "generic": {"partial-channel-block", "C%8", "unaligned", "K=1", "K=3", "K=7", "K=15", "K=31", "T=5", "T=64", "T=65", "T=130", "non-centred-pad", "B=1", "slice"},
        "dilated": {"T=20", "T=100", "T=520", "B=1", "B=2", "partial-channel-block", "dead-taps", "K=7", "K=31"},
    }
    have = {}
    for c in D.CASES:
        have.setdefault(D.forms(c)[1], set()).update(D.edges(c))
    for form, tags in need.items():
        assert tags <= have[form], (form, sorted(tags - have[form]))
    # the fast T edges hold for the CSGU and for the merge conv separately, and so do B = 1, the slice and the unaligned view
    for op in ("csgu", "merge"):
        tags = set().union(*[D.edges(c) for c in D.CASES if c.op == op and D.forms(c)[1] == "fast"])
        assert need["fast"] - {"B=3"} <= tags, (op, sorted(need["fast"] - tags))
    for op in ("csgu", "split", "merge"):
        tags = set().union(*[D.edges(c) for c in D.CASES if c.op == op and D.forms(c)[1] == "generic"])
        assert {"unaligned", "partial-channel-block", "non-centred-pad"} <= tags, (op, tags)
    assert {(c.C, c.op) for c in D.CASES if c.C % 8} == {(100, "merge")}                     # the CSGU entry points take C % 8 == 0 only through row_stats
    split31 = [c for c in D.CASES if c.op == "split" and (c.K, c.C, c.T, c.pad, c.dil, c.view) == (31, 64, 65, 15, 1, "contig")]
    assert split31 and D.forms(split31[0]) == ("generic", "generic")
    assert all(c.B * c.T * c.C <= 200_000 for c in D.CASES)


def test_real_case_subset_has_one_case_per_form_and_op():
    cells = [(D.forms(D.CASE_BY_NAME[n])[1], D.CASE_BY_NAME[n].op) for n in D.REAL_CASES]
    assert len(set(cells)) == len(cells) == 7
    assert [D.forms(D.CASE_BY_NAME[n])[0] for n in D.REAL_ACT_CASES] == ["fast", "generic"]
    assert all(D.CASE_BY_NAME[n].op == "csgu" for n in D.REAL_ACT_CASES)
