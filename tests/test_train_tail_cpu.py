"""The comparisons of tests/train_tail_ref.py must have teeth: every plausible slip of the cross-entropy gradient kernel and of the embedding-gradient kernels, built here as
a mutated reference, has to be REJECTED by the check the GPU tests (tests/test_gpu_train_tail.py) hold the kernels to, and an honest fp32 evaluation has to pass with room.
Also pins why tests/test_gpu_train_ops.py::test_ce_and_embed_bwd changed its comparison: the old floor-of-the-row-maximum tolerance accepts a gradient without its
label-smoothing term."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import train_tail_ref as R  # noqa: E402

BF = torch.bfloat16
F64 = torch.float64


def _ce_inputs(B, U, V, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, U, V, generator=g) * 2.0
    labels = torch.randint(0, V, (B, U), generator=g)
    labels[1, U - 4:] = -100
    return logits, labels


def _grad(logits, ref, *, p=None, target=None, k=None, smooth=1.0):
    """k (p - smooth * eps / V - (1 - eps) [c == target]) in fp64 on the rows the reference has a gradient for, in the reference's layout"""
    V = ref["V"]
    p = ref["p"] if p is None else p
    target = ref["target"] if target is None else target
    k = ref["k"] if k is None else k
    valid = target >= 0
    onehot = torch.zeros_like(p)
    onehot[valid, target[valid]] = 1.0
    g = k * (p - smooth * ref["eps"] / V - (1.0 - ref["eps"]) * onehot)
    g[~valid] = 0.0
    out = torch.zeros_like(ref["grad"])
    out[:, :V] = g
    return out


CE_SHAPES = [(3, 11, 65), (23, 14, 257)]          # (a few rows, one column past the wave stride) and (more rows than one block of the row sum, one column past the block stride)


@pytest.fixture(scope="module", params=CE_SHAPES, ids=lambda s: "B%d-U%d-V%d" % s)
def ce_case(request):
    B, U, V = request.param
    logits, labels = _ce_inputs(B, U, V, seed=7)
    ref = R.ce_ref(logits, labels, 1, 0.1, 0.6, ldo=V + 7)
    return logits, labels, ref


def test_the_reference_is_torch_cross_entropy(ce_case):
    logits, labels, ref = ce_case
    B, U, V = logits.shape
    lg = logits.double().clone().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(lg[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), label_smoothing=0.1, ignore_index=-100)
    (0.6 * loss).backward()
    assert abs(float(ref["acc"][0] / ref["acc"][1]) - float(loss.detach())) < 1e-12
    assert float((ref["grad"][:, :V] - lg.grad.reshape(B * U, V)).abs().max()) < 1e-15
    assert float(ref["grad"][:, V:].abs().max()) == 0.0
    assert torch.isnan(ref["row_loss"]).sum() == 4 and ref["row_loss"].numel() == B * (U - 1)


def test_the_unmutated_gradient_passes(ce_case):
    logits, labels, ref = ce_case
    assert R.ce_grad_ok(ref["grad"].to(BF), ref)
    assert R.ce_grad_ok(_grad(logits, ref).to(BF), ref)


def test_fp32_evaluation_of_the_kernel_formula_passes_with_a_fourfold_margin(ce_case):
    """rounded to bf16 it passes; before that rounding — which the tolerance's first term is there for — its error is within a quarter of the tolerance, and within a quarter
    of the fp32 term of the tolerance alone (the stronger statement)"""
    logits, labels, ref = ce_case
    V = ref["V"]
    emu = R.ce_grad_emulated_f32(logits, ref)
    assert R.ce_grad_ok(emu.to(BF), ref)
    rep = R.ce_grad_report(emu, ref)
    assert rep["ok"] and rep["worst"] <= 0.25, rep
    valid = ref["target"] >= 0
    onehot = torch.zeros_like(ref["p"])
    onehot[valid, ref["target"][valid]] = 1.0
    fp32_term = 2.0 ** -16 * ref["k"] * (ref["p"] + ref["eps"] / V + onehot)
    err = (emu[:, :V].double() - ref["grad"][:, :V]).abs()
    assert float((err / fp32_term)[valid].max()) <= 0.25


def _mutants(logits, labels, ref):
    B, U, V = logits.shape
    z = logits.double().reshape(B * U, V)
    yield "smoothing term dropped", _grad(logits, ref, smooth=0.0)
    yield "smoothing term doubled", _grad(logits, ref, smooth=2.0)
    Vw = V - V % 64
    e = torch.exp(z - z.max(dim=1, keepdim=True).values)
    yield "softmax normalised over the first V - V % 64 columns", _grad(logits, ref, p=e / e[:, :Vw].sum(dim=1, keepdim=True))
    unshifted = torch.where(ref["target"] >= 0, labels.reshape(-1), ref["target"])          # labels[b, u] on the rows that have a gradient (all of those are >= 0 here)
    yield "target from labels[b, u]", _grad(logits, ref, target=unshifted)
    count = float(ref["acc"][1])
    yield "count one too many", _grad(logits, ref, k=0.6 / (count + 1.0))
    yield "count one too few", _grad(logits, ref, k=0.6 / (count - 1.0))


def test_every_ce_gradient_mutant_is_rejected(ce_case):
    logits, labels, ref = ce_case
    seen = 0
    for name, g in _mutants(logits, labels, ref):
        rep = R.ce_grad_report(g.to(BF), ref)
        assert not rep["ok"] and rep["n_bad"] > 0, f"{name} passes: {rep}"
        seen += 1
    assert seen == 6


def test_poison_pad_columns_and_ignored_rows_are_rejected(ce_case):
    logits, labels, ref = ce_case
    V = ref["V"]
    good = ref["grad"].to(BF)
    for r, c, val in ((0, V, 1e-30), (0, V + 6, float("nan")), (1 * logits.shape[1] + logits.shape[1] - 1, 3, 1e-30), (0, 5, float("nan"))):
        bad = good.clone()
        bad[r, c] = val
        assert not R.ce_grad_ok(bad, ref), (r, c, val)


def test_a_zero_count_reference_is_all_zeros():
    logits, labels = _ce_inputs(3, 5, 65, seed=1)
    labels[:] = -100
    ref = R.ce_ref(logits, labels, 1, 0.1, 0.6, ldo=72)
    assert float(ref["acc"][0]) == 0.0 and float(ref["acc"][1]) == 0.0 and float(ref["grad"].abs().max()) == 0.0 and torch.isnan(ref["row_loss"]).all()
    assert R.ce_grad_ok(torch.zeros(15, 72, dtype=BF), ref)
    bad = torch.zeros(15, 72, dtype=BF)
    bad[7, 7] = 1e-20
    assert not R.ce_grad_ok(bad, ref)


def test_caller_supplied_count_sets_the_scale():
    logits, labels = _ce_inputs(3, 5, 65, seed=2)
    ref = R.ce_ref(logits, labels, 0, 0.0, 0.25, count=1.0)
    own = R.ce_ref(logits, labels, 0, 0.0, 0.25)
    assert ref["k"] == 0.25 and own["k"] == 0.25 / float(own["acc"][1])
    assert torch.allclose(ref["grad"] / float(own["acc"][1]), own["grad"], rtol=1e-14, atol=0)
    assert torch.equal(ref["acc"], own["acc"]) and torch.equal(ref["row_loss"].nan_to_num(-1.0), own["row_loss"].nan_to_num(-1.0))


def test_the_old_floor_tolerance_accepts_a_gradient_without_its_smoothing_term():
    """the inputs and the comparison of test_ce_and_embed_bwd as it stood: 5e-3 of the tensor's largest |value| (a target column) is above most of the k * softmax
    elements, so the eps / V term — dropped or doubled — disappears under it.  `ce_grad_ok` rejects both."""
    B, U, V = 3, 11, 50
    logits = torch.randn(B, U, V, generator=torch.Generator().manual_seed(1)) * 2.0
    labels = torch.randint(0, V, (B, U), generator=torch.Generator().manual_seed(2))
    labels[1, 7:] = -100
    ref = R.ce_ref(logits, labels, 1, 0.1, 0.6)
    want = ref["grad"]
    floor = 5e-3 * float(want.abs().max())
    assert float((want.abs() < floor).double().mean()) > 0.5                    # most elements are below the floor
    for smooth in (0.0, 2.0):
        mutant = _grad(logits, ref, smooth=smooth).to(BF)
        assert R.old_floor_close_ok(mutant, want)
        assert not R.ce_grad_ok(mutant, ref)
    assert R.old_floor_close_ok(want.to(BF), want) and R.ce_grad_ok(want.to(BF), ref)


# ---------------------------------------------------------------------------------------------------------------- embedding gradient
def _embed_case():
    V, d, U = 40, 8, 16
    M = 33 * U                                      # 528 rows: three chunks of 256
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V, (M,), generator=g)
    ids[255], ids[256], ids[257] = 5, 5, 5
    heavy = 39
    ids[torch.rand(M, generator=g) < 0.5] = heavy
    ids[255], ids[256], ids[257] = 5, 5, 5
    dx = R.int_valued((M, d), seed=12)
    dx[255], dx[256] = dx[255].abs() + 0.125, dx[256].abs() + 0.125      # rows whose loss cannot go unnoticed
    return ids.reshape(33, U), dx, V, heavy


def test_int_valued_sums_are_exact_in_fp32_in_any_order():
    x = R.int_valued((16517, 7), seed=3)
    want = x.double().sum(0)
    assert torch.equal(x.sum(0).double(), want)
    assert torch.equal(x.flip(0).cumsum(0)[-1].double(), want)
    perm = torch.randperm(16517, generator=torch.Generator().manual_seed(4))
    acc = torch.zeros(7)
    for chunk in x[perm].split(129):
        acc = acc + chunk.sum(0)
    assert torch.equal(acc.double(), want)
    assert float(x.abs().max()) <= 1.0 and float((x * 8).frac().abs().max()) == 0.0


def test_every_embedding_gradient_mutant_fails_the_exact_comparison():
    ids, dx, V, heavy = _embed_case()
    flat = ids.reshape(-1)
    dwte0 = R.int_valued((V, dx.shape[1]), seed=13)
    want, _ = R.embed_bwd_ref(ids, dx, V, scale=2.0, dwte0=dwte0)
    assert R.exact(want.float(), want)                                          # the honest result, held in fp32, passes

    def run(ids_=ids, dx_=dx):
        return R.embed_bwd_ref(ids_, dx_, V, scale=2.0, dwte0=dwte0)[0].float()

    for m in (255, 256):                                                        # one row dropped at a chunk boundary
        dropped = flat.clone()
        dropped[m] = -1
        assert not R.exact(run(dropped.reshape(ids.shape)), want), m
    twice = torch.cat([flat, flat[256:257]]).reshape(1, -1)                     # one row added twice
    assert not R.exact(run(twice, torch.cat([dx, dx[256:257]])), want)
    again = run()                                                               # the heavy id gathered as well as column-summed
    again[heavy] += 2.0 * dx[flat == heavy].sum(0)
    assert not R.exact(again, want)
    shifted = flat.clone()                                                      # the rows of one id summed into its neighbour
    shifted[flat == 5] = 6
    assert not R.exact(run(shifted.reshape(ids.shape)), want)
    nan = run()
    nan[3, 1] = float("nan")
    assert not R.exact(nan, want)


def test_embedding_references_ignore_and_clamp_out_of_range_ids():
    V, d = 10, 4
    ids = torch.tensor([[0, -100, -1, V, V + 7, 9]])
    dx = R.int_valued((6, d), seed=1)
    dwte, dwpe = R.embed_bwd_ref(ids, dx, V, n_pos=8, pos_offset=2)
    assert torch.equal(dwte[0], dx[0].double()) and torch.equal(dwte[9], dx[5].double()) and float(dwte[1:9].abs().max()) == 0.0
    assert torch.equal(dwpe[2:8], dx.double()) and float(dwpe[:2].abs().max()) == 0.0
    wte, pos = R.int_valued((V, d), seed=2), R.int_valued((8, d), seed=3)
    out = R.embed_fwd_ref(ids, wte, pos, scale=2.0, pos_offset=1, U=3)
    assert torch.equal(out[1], 2.0 * wte[0].double() + pos[2].double())         # -100 -> entry 0, row 1 -> position 1 + 1 % 3
    assert torch.equal(out[4], 2.0 * wte[9].double() + pos[2].double())         # V + 7 -> entry V - 1, row 4 -> position 1 + 4 % 3


# ---------------------------------------------------------------------------------------------------------------- optimizer
def test_adamw_reference_is_torch_adamw():
    n = 257
    g0 = torch.Generator().manual_seed(5)
    p0, m0, v0 = torch.randn(n, generator=g0).double(), torch.zeros(n).double(), torch.zeros(n).double()
    decay = torch.arange(n) % 3 != 0
    pa, pb = p0[decay].clone().requires_grad_(True), p0[~decay].clone().requires_grad_(True)
    opt = torch.optim.AdamW([{"params": [pa], "weight_decay": 0.01}, {"params": [pb], "weight_decay": 0.0}], lr=2e-3, betas=(0.9, 0.98), eps=1e-8)
    p, m, v = p0, m0, v0
    for step in (1, 2, 3):
        g = torch.randn(n, generator=g0).double()
        pa.grad, pb.grad = 0.5 * g[decay], 0.5 * g[~decay]
        opt.step()
        p, m, v = R.adamw_ref(p, g, m, v, decay, lr=2e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01, step=step, coef=0.5)
    want = torch.empty(n, dtype=F64)
    want[decay], want[~decay] = pa.detach(), pb.detach()
    assert float((p - want).abs().max()) < 1e-14
    q, mq, vq = R.adamw_ref(p, g, m, v, decay, lr=2e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01, step=4, skip=True)
    assert torch.equal(q, p) and torch.equal(mq, m) and torch.equal(vq, v)


def test_clip_reference():
    assert R.clip_ref(4.0, 1.0) == [2.0, 1.0 / (2.0 + 1e-6), 0.0]
    assert R.clip_ref(0.25, 1.0) == [0.5, 1.0, 0.0]
    assert R.clip_ref(4.0, 0.0) == [2.0, 1.0, 0.0]
    assert R.clip_ref(4.0, 1.0, skip_above=1.5) == [2.0, 0.0, 1.0]
    n, c, s = R.clip_ref(float("inf"), 1.0)
    assert n == float("inf") and c == 0.0 and s == 1.0
    n, c, s = R.clip_ref(float("nan"), 1.0)
    assert n != n and c == 0.0 and s == 1.0
