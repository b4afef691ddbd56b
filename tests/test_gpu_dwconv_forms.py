"""The fast depthwise-conv forward kernels (csrc/conv.hip: dwconv31_kernel, one instance per CSGU activation and one for the merge) against the generic
dwconv_time_kernel, bit for bit, and the properties the fast form's LDS reuse puts at risk.

The fast form passes its fp32 results through rows 0 .. 63 of the block's input tile once every wave holds its window in registers, and the thread that stores
(row, 8-channel chunk) multiplies by the x_r it loaded at the fill.  What can go wrong: a barrier missing around the reused tile (stale or half-written rows), a store
mapping that does not match the fill's (x_r of another row or chunk), rows past T, an activation instance wired to the wrong `act`, a row stride taken for C.

  * fast == generic: the same integer-valued data (dwconv_ref.int_inputs: every intermediate exact) once in a 16-B-aligned buffer and once in one that is only 8-B
    aligned ("off4": the fast-path predicate of dw_launch refuses it, nothing else differs), all four activations and the merge, B x C x T below.  Both forms apply
    the same float operations in the same order to every element, so equality is demanded for GELU and SiLU too; identity, ReLU and the merge are also held to the
    fp64 reference (exact on these inputs).
        T = 1, 15, 16: no interior tile, the halo longer than the utterance;  63, 64, 65: one tile less a row, exactly one, one row into the second;
        94: the tile plus its halo;  250: the flagship's 3 tiles + 58 rows.   C = 64, 128: one and two channel blocks.   B = 1, 2.
  * no stale LDS: outputs pre-filled with NaN, two calls with different inputs in one process, no NaN left and the second result equal to the fp64 reference.
  * row strides: ld_in = ld_mul = 2 C + 128 and ld_out = 2 C, the slack holding a sentinel that must survive.
  * real-valued inputs: the derived bounds of tests/test_gpu_dwconv.py (its helpers, imported) for the four activation instances.
"""
import pytest
import torch

import dwconv_ref as D
from test_gpu_dwconv import (BF, DEV, EPS, F32, G, JUNK, Guarded, _report, assert_equal, device_inputs, ratio_bf16, run_fwd)

pytestmark = pytest.mark.gpu

ACTS = (0, 1, 2, 3)                      # identity, GELU, ReLU, SiLU
EXACT_ACTS = (0, 2)                      # integer inputs stay integers: the fp64 reference is exact
SHAPES = [(B, C, T) for B in (1, 2) for C in (64, 128) for T in (1, 15, 16, 63, 64, 65, 94, 250)]
NAN = float("nan")


def _pair(op, B, T, C):
    """the same case twice: in a buffer the fast form accepts and in one only the generic form takes"""
    fast, gen = D._c(f"forms-{op}", op, B, T, C, view="contig"), D._c(f"forms-{op}", op, B, T, C, view="off4")
    assert D.forms(fast)[0] == "fast" and D.forms(gen)[0] == "generic"
    return fast, gen


def _seeded_int_inputs(case, seed):
    """dwconv_ref.int_inputs with another seed: its generator is keyed by the case's place in the table, and these cases are not in it"""
    orig = D._gen
    D._gen = lambda c, salt: torch.Generator().manual_seed(seed)
    try:
        return D.int_inputs(case)
    finally:
        D._gen = orig


def _nan_output(case):
    out = Guarded(case.B * case.T, case.C, BF)
    out.view.fill_(NAN)
    return out


def _run(case, d, act):
    out = _nan_output(case)
    run_fwd(case, d, out.view, act)
    torch.cuda.synchronize()
    assert out.guards_intact(), f"{case.name} act {act}: wrote outside its (B*T, C) output"
    got = out.view.clone()
    assert not bool(torch.isnan(got).any()), f"{case.name} act {act}: rows < T left unwritten"
    return got


@pytest.mark.parametrize("op", ["csgu", "merge"])
@pytest.mark.parametrize("B,C,T", SHAPES, ids=lambda v: str(v))
def test_fast_form_equals_generic_form_bit_for_bit(op, B, C, T):
    fast, gen = _pair(op, B, T, C)
    inp = D.int_inputs(fast)
    d_fast, d_gen = device_inputs(fast, inp), device_inputs(gen, inp)
    for act in (ACTS if op == "csgu" else (0,)):
        got_fast, got_gen = _run(fast, d_fast, act), _run(gen, d_gen, act)
        assert_equal(got_fast, got_gen, f"{op} B {B} C {C} T {T} act {act}: fast form against generic form", fast)
        if act in EXACT_ACTS:
            assert_equal(got_fast, D.reference(fast, inp, act=act)["fwd"].to(BF), f"{op} B {B} C {C} T {T} act {act}: fast form against the reference", fast)


@pytest.mark.parametrize("op", ["csgu", "merge"])
@pytest.mark.parametrize("B,C,T", [(2, 128, 250), (2, 64, 65), (1, 64, 15)], ids=lambda v: str(v))
def test_second_call_with_other_inputs_leaves_no_stale_result(op, B, C, T):
    case = _pair(op, B, T, C)[0]
    for act in (EXACT_ACTS if op == "csgu" else (0,)):
        out = _nan_output(case)
        for seed in (11, 12):
            inp = _seeded_int_inputs(case, seed)
            d = device_inputs(case, inp)
            out.poison()
            out.view.fill_(NAN)
            run_fwd(case, d, out.view, act)
            torch.cuda.synchronize()
            assert out.guards_intact()
            assert not bool(torch.isnan(out.view).any()), f"{op} act {act} call with seed {seed}: rows < T left unwritten"
        assert_equal(out.view, D.reference(case, inp, act=act)["fwd"].to(BF), f"{op} B {B} C {C} T {T} act {act}: second call against the reference", case)


@pytest.mark.parametrize("op", ["csgu", "merge"])
@pytest.mark.parametrize("B,C,T", [(2, 128, 250), (1, 64, 65)], ids=lambda v: str(v))
def test_row_strides_larger_than_the_channel_count(op, B, C, T):
    case = D._c(f"forms-{op}-strided", op, B, T, C, view="slice64")          # the conv input (and x_r) inside a buffer 128 columns wider: ld_in = ld_mul = W + 128
    assert D.forms(case)[0] == "fast"
    inp = D.int_inputs(case)
    d = device_inputs(case, inp)
    src = d["m" if op == "merge" else "u"]
    assert src.stride(0) == D.layout(case)["ld_in"] > C
    M = B * T
    big = torch.full((G + M + G, 2 * C), 77.0, device=DEV, dtype=BF)          # ld_out = 2 C: the result is the left half of a row, as the encoder's buffers have it
    out = big[G:G + M, :C]
    assert out.data_ptr() % 16 == 0 and out.stride(0) == 2 * C
    for act in (EXACT_ACTS if op == "csgu" else (0,)):
        big.fill_(77.0)
        out.fill_(NAN)
        run_fwd(case, d, out, act)
        torch.cuda.synchronize()
        assert bool((big[:G] == 77.0).all()) and bool((big[G + M:] == 77.0).all()) and bool((big[G:G + M, C:] == 77.0).all()), f"{op} act {act}: the slack of the output rows changed"
        assert_equal(out.clone(), D.reference(case, inp, act=act)["fwd"].to(BF), f"{op} B {B} C {C} T {T} act {act}: strided rows against the reference", case)
    # the input's slack columns and guard rows still hold what place() put there
    whole = src._base if src._base is not None else src
    off, W = D.VIEW_OFF[case.view], D.layout(case)["W"]
    assert bool((whole[:, :off] == JUNK).all()) and bool((whole[:, off + W:] == JUNK).all()) and bool((whole[:G] == JUNK).all()) and bool((whole[G + M:] == JUNK).all())


@pytest.mark.parametrize("act", ACTS)
def test_real_valued_inputs_stay_inside_the_derived_bound_per_activation(act):
    case = D._c("forms-csgu-real", "csgu", 2, 250, 128)
    assert D.forms(case)[0] == "fast"
    inp = D.real_inputs(case, EPS)
    d = device_inputs(case, inp)
    out = Guarded(case.B * case.T, case.C, BF)
    run_fwd(case, d, out.view, act)
    torch.cuda.synchronize()
    assert out.guards_intact()
    r64, r32 = D.reference(case, inp, act=act)["fwd"], D.reference(case, inp, act=act, dtype=F32)["fwd"]
    fit = D.GELU_FIT_ERR * inp["u"][:, :case.C].abs() if act == 1 else None             # out = x_r * gelu(conv): the fit's specified tolerance (tests/test_gpu_dwconv.py)
    _report(f"fast csgu B 2 T 250 C 128 act {act}", {"fwd": ratio_bf16(out.view, r64, r32, fit)})


def test_real_valued_merge_stays_inside_the_derived_bound():
    case = D._c("forms-merge-real", "merge", 2, 250, 128)
    assert D.forms(case)[0] == "fast"
    inp = D.real_inputs(case, EPS)
    d = device_inputs(case, inp)
    out = Guarded(case.B * case.T, case.C, BF)
    run_fwd(case, d, out.view, 0)
    torch.cuda.synchronize()
    assert out.guards_intact()
    r64, r32 = D.reference(case, inp)["fwd"], D.reference(case, inp, dtype=F32)["fwd"]
    _report("fast merge B 2 T 250 C 128", {"fwd": ratio_bf16(out.view, r64, r32)})
