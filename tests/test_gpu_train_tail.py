"""GPU: the kernels that close a training step, at the sizes where they loop — the label-smoothed cross entropy and its gradient (ce_smooth_kernel / ce_sum_kernel,
ce_bwd_kernel), the token embedding and its gradient (embed_kernel, embed_bwd_wte_kernel / embed_bwd_heavy_kernel / rows_reduce_kernel / embed_bwd_wpe_kernel) and the
flat-buffer optimizer kernels (sumsq, dot, clip_coef, adamw, axpy, scale, and their device-scalar forms) — against the fp64 references of tests/train_tail_ref.py.

Sums are tested with integer-valued inputs and must EQUAL the reference (see `int_valued`); the CE gradient is held to `ce_grad_ok`, elementwise with no floor taken from
the row maximum (tests/test_train_tail_cpu.py shows which slips that rejects).  Every output starts as poison (NaN; -7 for the row losses, where NaN is itself an answer), every call is made twice and must return the same bits."""
import functools
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import train_tail_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32
NAN = float("nan")


def _o():
    from huggingface_asr_amd import _lib, ops, ops_train
    return ops, ops_train, _lib


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def poison_next(shape, dtype):
    """the wrappers that allocate their own output take it with torch.empty: fill a block of that size with NaN and hand it back to the caching allocator, which gives the
    next request of the same size that block (best effort: the allocator promises nothing, the tests do not depend on it)"""
    t = torch.full(shape, NAN, device=DEV, dtype=dtype)
    torch.cuda.current_stream().synchronize()
    del t


def pad64(n):
    return (n + 63) // 64 * 64


# ================================================================================================================ cross entropy
CE_B, CE_U = 23, 14                   # 322 rows at shift 0, 299 at shift 1: neither a multiple of the 4 rows of a block, both past the 256-row stride of the row sum
CE_VS = [50, 64, 65, 256, 257, 5001, 8192]      # the 64-lane stride of the forward and the 256-thread stride of the backward: below, at and one past; the two recipe sizes


@functools.lru_cache(maxsize=None)
def _ce_inputs(V, shift):
    """(logits buffer (B, U, ld) fp32 with NaN in columns V.., labels (B, U)) on the CPU.  Utterance 1 has a padded tail, utterance 2 is ignored altogether; rows 0..3 of
    utterance 0: +80 in the last column (the target) and -80 in the first; -80 at the target and +80 elsewhere; all values equal; the target holds the smallest logit."""
    B, U = CE_B, CE_U
    g = torch.Generator().manual_seed(1000 + V)
    ld = pad64(V + 1)
    buf = torch.full((B, U, ld), NAN)
    z = torch.randn(B, U, V, generator=g) * 2.0
    labels = torch.randint(0, V, (B, U), generator=g)
    z[0, 0, V - 1], z[0, 0, 0] = 80.0, -80.0
    labels[0, 0 + shift] = V - 1
    z[0, 1, V - 1], z[0, 1, 1] = -80.0, 80.0
    labels[0, 1 + shift] = V - 1
    z[0, 2, :] = 1.5
    labels[0, 3 + shift] = int(z[0, 3].argmin())
    labels[1, U - 4:] = -100
    labels[2, :] = -100
    buf[..., :V] = z
    return buf, labels


def _ce_forward(lib, lg, lab, shift, eps, acc, rows):
    _, _, _lib = _o()
    B, U, V = lg.shape
    _lib.check(lib.mi_ce_label_smoothing(lg.data_ptr(), lg.stride(1), lab.data_ptr(), B, U, shift, V, float(eps), acc.data_ptr(), rows.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "mi_ce_label_smoothing")


def _assert_grad(dl, ref, what):
    rep = R.ce_grad_report(dl, ref)
    assert rep["ok"], f"{what}: {rep}"


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("V", CE_VS)
def test_cross_entropy_and_its_gradient(V, shift, eps):
    ops, T, _lib = _o()
    B, U = CE_B, CE_U
    buf, labels = _ce_inputs(V, shift)
    ldo = (V + 7) // 8 * 8 + 8
    ref = R.ce_ref(buf[..., :V], labels, shift, eps, 0.6, ldo=ldo)
    lg, lab = buf.to(DEV)[..., :V], labels.to(DEV)
    assert lg.stride(1) > V and not lg.is_contiguous()
    n_rows = B * (U - shift)
    # ---- forward: per-row losses, the [sum, count] pair, a second call adds into it
    acc = torch.zeros(2, device=DEV)
    rows = torch.full((n_rows,), -7.0, device=DEV)
    _ce_forward(_lib.lib(), lg, lab, shift, eps, acc, rows)
    rows1, acc1 = rows.clone(), acc.clone()
    rows.fill_(-7.0)
    _ce_forward(_lib.lib(), lg, lab, shift, eps, acc, rows)
    assert same_bits(rows, rows1)
    got = rows1.cpu().double()
    want = ref["row_loss"]
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN marks exactly the ignored rows"
    ok = ~torch.isnan(want)
    err = (got[ok] - want[ok]).abs()
    print(f"ce rows V={V} shift={shift} eps={eps}: max |err| {float(err.max()):.3g}, max loss {float(want[ok].max()):.4g}")
    torch.testing.assert_close(got[ok], want[ok], atol=1e-4, rtol=1e-4)
    a1 = acc1.cpu().double()
    assert float(a1[1]) == float(ref["acc"][1]) == float(ok.sum())
    torch.testing.assert_close(a1[0] / a1[1], ref["acc"][0] / ref["acc"][1], atol=1e-4, rtol=1e-4)
    # the sum is the kernel's own rows added in fp32 by a tree of depth ~10: a row the stride skipped is 1/300 of it
    assert abs(float(a1[0]) - float(got[ok].sum())) <= 16 * 2.0 ** -24 * float(got[ok].abs().sum())
    assert torch.equal(acc.cpu().double(), 2.0 * a1), "the pair accumulates (x + x is exact)"
    assert same_bits(ops.ce_label_smoothing(lg, lab, shift=shift, eps=eps, return_acc=True), acc1)
    # ---- backward
    outs = []
    for _ in range(2):
        poison_next((B * U, ldo), BF)
        outs.append(T.ce_label_smoothing_bwd(lg, lab, acc1, shift=shift, eps=eps, weight=0.6, ldo=ldo))
    assert outs[0].shape == (B * U, ldo) and same_bits(outs[0], outs[1])
    rep = R.ce_grad_report(outs[0], ref)
    print(f"ce grad V={V} shift={shift} eps={eps}: worst err/tol {rep['worst']:.3g} at {rep['first']}")
    assert rep["ok"], rep


def test_cross_entropy_of_a_batch_without_targets():
    """every label ignored: the count is zero, the pair stays [0, 0], every row loss is NaN, the gradient is all zeros"""
    ops, T, _lib = _o()
    B, U, V, shift = CE_B, CE_U, 257, 1
    buf, _ = _ce_inputs(V, shift)
    labels = torch.full((B, U), -100, dtype=torch.long)
    ref = R.ce_ref(buf[..., :V], labels, shift, 0.1, 0.6, ldo=272)
    lg, lab = buf.to(DEV)[..., :V], labels.to(DEV)
    acc = torch.zeros(2, device=DEV)
    rows = torch.full((B * (U - shift),), -7.0, device=DEV)
    _ce_forward(_lib.lib(), lg, lab, shift, 0.1, acc, rows)
    assert torch.isnan(rows).all() and torch.equal(acc.cpu(), torch.zeros(2))
    for _ in range(2):
        poison_next((B * U, 272), BF)
        dl = T.ce_label_smoothing_bwd(lg, lab, acc, shift=shift, eps=0.1, weight=0.6, ldo=272)
        assert bool((dl == 0).all())
        _assert_grad(dl, ref, "no targets")


def test_cross_entropy_gradient_with_a_caller_built_pair():
    """the BEST-RQ trainer's form: shift 0, no smoothing, acc = [anything, 1] and weight = 1 / n — the gradient of the SUM over the rows, scaled"""
    ops, T, _lib = _o()
    B, U, V = CE_B, CE_U, 8192
    buf, labels = _ce_inputs(V, 0)
    ldo = V + 64
    ref = R.ce_ref(buf[..., :V], labels, 0, 0.0, 1.0 / 12.0, count=1.0, ldo=ldo)
    lg, lab = buf.to(DEV)[..., :V], labels.to(DEV)
    pair = torch.tensor([3.25, 1.0], device=DEV)
    outs = []
    for _ in range(2):
        poison_next((B * U, ldo), BF)
        outs.append(T.ce_label_smoothing_bwd(lg, lab, pair, shift=0, eps=0.0, weight=1.0 / 12.0, ldo=ldo))
    assert same_bits(outs[0], outs[1]) and torch.equal(pair.cpu(), torch.tensor([3.25, 1.0]))
    _assert_grad(outs[0], ref, "caller-built pair")


# ================================================================================================================ embedding gradient
EMB_SHAPES = [(3, 11, 64, 50), (1, 257, 256, 5001), (72, 80, 256, 5000), (1, 1031, 1024, 163), (83, 199, 64, 40)]       # (B, U, d, V): M = B * U
E_BOUNDARY, E_FULL, E_WAVES, PAD = 3, 20, 33, 2          # entries with hand-placed rows; the padding token of the heavy cases
HEAVY_MODES = ["none", "pad", "absent", "last", "outside"]


def _embed_ids(B, U, V, heavy_mode, seed):
    """random ids, then the heavy token on ~60 % of the rows, then by hand (M permitting): one entry at rows 255, 256, 257 (both sides of a 256-row chunk boundary); one
    entry on all 256 rows of a chunk (the hit list full); one entry in each of the four waves of a chunk; entries 15 and 16 (the last of one 16-entry block, the first of
    the next); the last entry V - 1 (V is no multiple of 16); and the ids -100, -1, V, V + 7, which add nothing."""
    M = B * U
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, V, (M,), generator=g)
    heavy = {"none": None, "pad": PAD, "absent": 4, "last": V - 1, "outside": V + 3}[heavy_mode]
    if heavy_mode in ("pad", "last"):
        ids[torch.rand(M, generator=g) < 0.6] = heavy
    if heavy_mode == "absent":
        ids[ids == heavy] = 7
    if M >= 768:
        ids[512:768] = E_FULL
    elif M >= 256:
        ids[0:256:2] = E_FULL                         # (every other row, so that the heavy token keeps rows at this M)
    if M >= 512:
        ids[torch.tensor([256 + 3, 256 + 70, 256 + 130, 256 + 200])] = E_WAVES
    elif M >= 256:
        ids[torch.tensor([3, 70, 130, 200])] = E_WAVES
    if M > 257:
        ids[255:258] = E_BOUNDARY
    elif M > 256:
        ids[255:257] = E_BOUNDARY
    ids[5], ids[6], ids[7] = 15, 16, V - 1
    ids[8], ids[9], ids[10], ids[11] = -100, -1, V, V + 7
    return ids.reshape(B, U), heavy


def _embed_bwd_run(T, ids, dx, V, d, heavy, *, scale, pos_offset, n_pos, dwte0, dwpe0):
    dwte = dwte0.to(DEV).clone()
    dwpe = None if dwpe0 is None else dwpe0.to(DEV).clone()
    T.embed_tokens_bwd(ids, dx, dwte, dwpe, scale=scale, pos_offset=pos_offset, heavy_id=heavy)
    return dwte, dwpe


@pytest.mark.parametrize("heavy_mode", HEAVY_MODES)
@pytest.mark.parametrize("shape", EMB_SHAPES, ids=lambda s: "M%d-d%d-V%d" % (s[0] * s[1], s[2], s[3]))
def test_embedding_gradient_is_exact(shape, heavy_mode):
    _, T, _ = _o()
    B, U, d, V = shape
    M = B * U
    assert V % 16 != 0
    ids, heavy = _embed_ids(B, U, V, heavy_mode, seed=31 + M)
    dx = R.int_valued((M, d), seed=32 + M)
    pos_offset, n_pos = 3, U + 5
    dwte0, dwpe0 = R.int_valued((V, d), seed=33), R.int_valued((n_pos, d), seed=34)
    kw = dict(scale=4.0, pos_offset=pos_offset, n_pos=n_pos)
    want_te, want_pe = R.embed_bwd_ref(ids, dx, V, dwte0=dwte0, dwpe0=dwpe0, **kw)
    ids_d, dx_d = ids.to(DEV), dx.to(DEV)
    te1, pe1 = _embed_bwd_run(T, ids_d, dx_d, V, d, heavy, dwte0=dwte0, dwpe0=dwpe0, **kw)
    te2, pe2 = _embed_bwd_run(T, ids_d, dx_d, V, d, heavy, dwte0=dwte0, dwpe0=dwpe0, **kw)
    assert same_bits(te1, te2) and same_bits(pe1, pe2)
    bad = (te1.cpu().double() != want_te).any(dim=1).nonzero()[:, 0].tolist()
    assert not bad, f"dwte entries off: {bad[:20]} (heavy {heavy}; rows per entry {[int((ids == v).sum()) for v in bad[:20]]})"
    assert R.exact(te1, want_te) and R.exact(pe1, want_pe)
    # the heavy entry as a column sum and as a gather: the same bits
    te3, pe3 = _embed_bwd_run(T, ids_d, dx_d, V, d, None, dwte0=dwte0, dwpe0=dwpe0, **kw)
    assert same_bits(te3, te1) and same_bits(pe3, pe1)
    # no position gradient (fixed positions): the token gradient is unchanged
    te4, pe4 = _embed_bwd_run(T, ids_d, dx_d, V, d, heavy, dwte0=dwte0, dwpe0=None, **kw)
    assert pe4 is None and same_bits(te4, te1)


def test_embedding_gradient_small_call_after_a_large_one_sees_a_clean_workspace():
    """the entry-occurs flags and the heavy entry's partial rows live in one shared workspace: what the large call left there must not leak into the small one"""
    _, T, _ = _o()
    for (B, U, d, V) in (EMB_SHAPES[4], EMB_SHAPES[0]):
        M = B * U
        ids, heavy = _embed_ids(B, U, V, "pad", seed=41)
        dx = R.int_valued((M, d), seed=42)
        dwte0 = R.int_valued((V, d), seed=43)
        want, _ = R.embed_bwd_ref(ids, dx, V, scale=0.5, dwte0=dwte0)
        got, _ = _embed_bwd_run(T, ids.to(DEV), dx.to(DEV), V, d, heavy, scale=0.5, pos_offset=0, n_pos=None, dwte0=dwte0, dwpe0=None)
        assert R.exact(got, want), (M, d, V)


def test_embedding_gradient_of_normal_data_at_the_recipe_shape():
    """realism, not sharpness: normal dx, scale sqrt(768), the padding token on 60 % of 5760 rows, against fp64.  Bound per element: 2 n_e 2**-24 sum |scale dx| over the
    entry's n_e rows — what any fp32 sum of n_e terms satisfies (n_e - 1 additions, one product each, one rounding of the scale)."""
    _, T, _ = _o()
    B, U, d, V = EMB_SHAPES[2]
    M = B * U
    ids, heavy = _embed_ids(B, U, V, "pad", seed=51)
    dx = torch.randn(M, d, generator=torch.Generator().manual_seed(52))
    scale = math.sqrt(768.0)
    want, want_pe = R.embed_bwd_ref(ids, dx, V, scale=scale, n_pos=U)
    flat = ids.reshape(-1)
    okid = (flat >= 0) & (flat < V)
    n_e = torch.zeros(V, dtype=torch.float64).index_add_(0, flat[okid], torch.ones(int(okid.sum()), dtype=torch.float64))
    mag = torch.zeros(V, d, dtype=torch.float64).index_add_(0, flat[okid], (scale * dx[okid].double()).abs())
    dwte, dwpe = torch.zeros(V, d, device=DEV), torch.zeros(U, d, device=DEV)
    T.embed_tokens_bwd(ids.to(DEV), dx.to(DEV), dwte, dwpe, scale=scale, heavy_id=heavy)
    err = (dwte.cpu().double() - want).abs()
    tol = 2.0 * n_e[:, None] * 2.0 ** -24 * mag
    print(f"embed bwd normal data: max err/tol {float((err / tol.clamp(min=1e-300)).max()):.3g}, heavy rows {int(n_e[heavy])}")
    assert bool((err <= tol).all())
    pe_err = (dwpe.cpu().double() - want_pe).abs()
    pe_mag = torch.zeros(U, d, dtype=torch.float64).index_add_(0, torch.arange(M) % U, dx.double().abs())
    assert bool((pe_err <= 2.0 * B * 2.0 ** -24 * pe_mag).all())


# ================================================================================================================ embedding forward
def test_embedding_forward_is_exact_past_the_grid_cap():
    ops, _, _ = _o()
    B, U, d, V = 41, 100, 512, 97                     # M * d / 4 = 524 800 float4 > 2048 blocks * 256 threads: the grid strides
    M = B * U
    assert M * d // 4 > 2048 * 256
    g = torch.Generator().manual_seed(61)
    ids = torch.randint(0, V, (B, U), generator=g)
    ids[0, 0], ids[0, 1], ids[40, 99], ids[40, 98] = -1, V, V + 7, -100          # clamped to the ends of the table
    wte, pos = R.int_valued((V, d), seed=62), R.int_valued((U + 9, d), seed=63)
    for U_arg, off in ((None, 0), (None, 9), (25, 4)):                          # the position index wraps at U, which need not be the row length of `ids`
        want = R.embed_fwd_ref(ids, wte, pos, scale=2.0, pos_offset=off, U=U_arg)
        outs = []
        for _ in range(2):
            poison_next((M, d), F32)
            outs.append(ops.embed_tokens(ids.to(DEV), wte.to(DEV), pos.to(DEV), scale=2.0, pos_offset=off, U=U_arg))
        assert same_bits(outs[0], outs[1]) and R.exact(outs[0], want), (U_arg, off)
    with pytest.raises(RuntimeError):                                           # rows are read 16 bytes at a time: d % 4 != 0 is refused
        ops.embed_tokens(ids.to(DEV), wte[:, :510].contiguous().to(DEV), pos[:, :510].contiguous().to(DEV))


# ================================================================================================================ reductions and optimizer
N_BIG = 16384 * 256 * 4 + 4 * 256 * 3 + 3         # the 16384-block cap twice over in 16-byte steps, a vector remainder, a 3-element scalar tail; 16 sweeps of the 1024-block reductions
N_SMALL = 5003
SIZES = [("big", N_BIG, 0), ("small", N_SMALL, 0), ("small-unaligned", N_SMALL, 1), ("big-unaligned", N_BIG, 1)]     # offset 1: a view buf[1:], 4 bytes off: the scalar path


@functools.lru_cache(maxsize=None)
def _ternary(n, seed):
    return (torch.randint(0, 3, (n,), generator=torch.Generator().manual_seed(seed)) - 1).to(F32)


@functools.lru_cache(maxsize=None)
def _normal(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def _view(x_cpu, off, fill=NAN):
    """x on the device as buf[off:] of a buffer whose first `off` elements are poison"""
    buf = torch.full((x_cpu.numel() + off,), fill, device=DEV, dtype=x_cpu.dtype)
    buf[off:] = x_cpu.to(DEV)
    v = buf[off:]
    assert v.data_ptr() % 16 == (4 * off) % 16 or x_cpu.dtype != F32
    return v


@pytest.mark.parametrize("name,n,off", SIZES, ids=[s[0] for s in SIZES])
def test_sumsq_and_dot(name, n, off):
    _, T, _ = _o()
    x, y = _ternary(n, 71), _ternary(n, 72)
    xd, yd = _view(x, off), _view(y, off)
    # {-1, 0, 1}: every partial sum is an integer below 2**24: exact in any order
    for _ in range(2):
        acc = torch.zeros(1, device=DEV)
        T.sumsq_(acc, xd)
        assert float(acc) == float((x != 0).sum()), name
        acc = torch.zeros(1, device=DEV)
        T.dot_(acc, xd, yd)
        assert float(acc) == float((x.double() * y.double()).sum()), name
    acc = torch.full((1,), 5.0, device=DEV)
    T.sumsq_(acc, xd)
    assert float(acc) == 5.0 + float((x != 0).sum())
    acc = torch.full((1,), 5.0, device=DEV)
    T.dot_(acc, xd, yd)
    assert float(acc) == 5.0 + float((x.double() * y.double()).sum())
    # normal data against fp64, 1e-5 of the sum of the magnitudes of the terms
    a, b = _normal(n, 73), _normal(n, 74)
    ad, bd = _view(a, off), _view(b, off)
    s1, s2, d1, d2 = (torch.zeros(1, device=DEV) for _ in range(4))
    T.sumsq_(s1, ad); T.sumsq_(s2, ad); T.dot_(d1, ad, bd); T.dot_(d2, ad, bd)
    assert same_bits(s1, s2) and same_bits(d1, d2)
    want = float((a.double() ** 2).sum())
    assert abs(float(s1) - want) <= 1e-5 * want
    prod = a.double() * b.double()
    assert abs(float(d1) - float(prod.sum())) <= 1e-5 * float(prod.abs().sum())
    # a NaN anywhere is a NaN out: in the vector body, in the last element
    for where in (n // 2, n - 1):
        ad[where] = NAN
        s, dd = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        T.sumsq_(s, ad); T.dot_(dd, bd, ad)
        assert math.isnan(float(s)) and math.isnan(float(dd)), where
        ad[where] = 1.0


@pytest.mark.parametrize("sumsq,max_norm,skip_above", [(4.0, 1.0, 0.0), (0.25, 1.0, 0.0), (4.0, 0.0, 0.0), (4.0, 1.0, 1.5), (4.0, 1.0, 2.0), (4.0, 1.0, 2.5), (1e-14, 1.0, 0.0),
                                                       (float("inf"), 1.0, 0.0), (float("nan"), 1.0, 0.0), (float("inf"), 0.0, 0.0)])
def test_clip_coef(sumsq, max_norm, skip_above):
    _, T, _ = _o()
    out = torch.full((3,), NAN, device=DEV)
    T.clip_coef(torch.tensor([sumsq], device=DEV), max_norm, out, skip_above=skip_above)
    got, want = out.cpu().double(), torch.tensor(R.clip_ref(sumsq, max_norm, skip_above), dtype=torch.float64)
    torch.testing.assert_close(got, want, atol=0.0, rtol=1e-6, equal_nan=True)
    assert float(got[2]) in (0.0, 1.0) and (float(got[2]) == 0.0 or float(got[1]) == 0.0)


HP = dict(lr=2e-3, eps=1e-8, weight_decay=0.01)
#            name                n        betas         steps    decay  mirror norm   views 4 bytes / 1 element off
ADAMW = [("big",                N_BIG,   (0.9, 0.98),  (1, 2),  True,  True,  True,  ()),
         ("small-bare",         N_SMALL, (0.9, 0.98),  (1, 2),  False, False, False, ()),
         ("small-all",          N_SMALL, (0.9, 0.98),  (1, 2),  True,  True,  True,  ()),
         ("step-1000",          N_SMALL, (0.9, 0.999), (1000,), True,  True,  True,  ()),
         ("unaligned-buffers",  N_SMALL, (0.9, 0.98),  (1, 2),  True,  True,  True,  ("p", "g", "m", "v")),
         ("unaligned-p",        N_SMALL, (0.9, 0.98),  (1, 2),  True,  True,  True,  ("p",)),
         ("unaligned-decay",    N_SMALL, (0.9, 0.98),  (1, 2),  True,  True,  True,  ("decay",)),
         ("unaligned-mirror",   N_SMALL, (0.9, 0.98),  (1, 2),  True,  True,  True,  ("mirror",))]


def _adamw_state(n, steps):
    p0 = _normal(n, 73)
    if steps[0] == 1:
        return p0, torch.zeros(n), torch.zeros(n)
    return p0, 0.1 * _normal(n, 74), 0.01 * _normal(n, 75).abs()       # a state a thousand steps in


def _adamw_device_run(T, p0, m0, v0, grads, decay, betas, steps, use_mirror, nc, off):
    o = lambda k: 1 if k in off else 0                                          # noqa: E731
    p, m, v = _view(p0, o("p")), _view(m0, o("m")), _view(v0, o("v"))
    dm = None if decay is None else _view(decay.to(torch.uint8), o("decay"), fill=1)
    mirror = _view(torch.zeros(p0.numel(), dtype=BF), o("mirror")).fill_(NAN) if use_mirror else None
    for step, g in zip(steps, grads):
        T.adamw_step_(p, _view(g, o("g")), m, v, dm, betas=betas, step=step, norm_coef=nc, mirror=mirror, **HP)
    return p, m, v, mirror


@pytest.mark.parametrize("case", ADAMW, ids=[c[0] for c in ADAMW])
def test_adamw_step(case):
    """p against torch's AdamW formula in fp64 at atol 1e-6 / rtol 1e-5; m and v at rtol 1e-5 against the same formula with the betas the fp32 interface can carry
    (1 - fp32(0.999) is 1.3e-5 away from 0.001: the interface, not the kernel).  The bias corrections are computed in fp32 by the launcher: step 1000 checks that."""
    _, T, _ = _o()
    name, n, betas, steps, use_decay, use_mirror, use_norm, off = case
    p0, m0, v0 = _adamw_state(n, steps)
    grads = [_normal(n, 74) * 3.0, _normal(n, 75) * 0.1][:len(steps)]
    decay = (torch.arange(n) % 3 != 0) if use_decay else None
    coef = 0.5 if use_norm else 1.0
    nc = torch.tensor([2.0, coef, 0.0], device=DEV) if use_norm else None
    runs = [_adamw_device_run(T, p0, m0, v0, grads, decay, betas, steps, use_mirror, nc, off) for _ in range(2)]
    for a, b in zip(*runs):
        assert (a is None and b is None) or same_bits(a, b)
    p, m, v, mirror = runs[0]
    b32 = tuple(float(torch.tensor(b, dtype=F32)) for b in betas)
    wp, wm, wv = p0, m0, v0
    xp, xm, xv = p0, m0, v0
    for step, g in zip(steps, grads):
        wp, wm, wv = R.adamw_ref(wp, g, wm, wv, decay, betas=betas, step=step, coef=coef, **HP)
        xp, xm, xv = R.adamw_ref(xp, g, xm, xv, decay, betas=b32, step=step, coef=coef, **HP)
    err = (p.cpu().double() - wp).abs()
    print(f"adamw {name}: max |dp| {float(err.max()):.3g}, max |dp| / (1e-6 + 1e-5 |p|) {float((err / (1e-6 + 1e-5 * wp.abs())).max()):.3g}")
    torch.testing.assert_close(p.cpu().double(), wp, atol=1e-6, rtol=1e-5)
    torch.testing.assert_close(m.cpu().double(), xm, atol=1e-6, rtol=1e-5)       # m is a difference of terms of magnitude ~1: a few fp32 roundings of those
    torch.testing.assert_close(v.cpu().double(), xv, atol=1e-12, rtol=1e-5)
    if use_mirror:
        assert torch.equal(mirror.cpu(), p.cpu().to(BF))


@pytest.mark.parametrize("name,n,off", SIZES[:3], ids=[s[0] for s in SIZES[:3]])
def test_adamw_skipped_step_leaves_everything_untouched(name, n, off):
    """the skip flag, or a norm that is not finite: p, m and v keep their bits; the bf16 mirror is still refreshed from p"""
    _, T, _ = _o()
    p0, m0, v0 = _adamw_state(n, (1000,))
    g = _normal(n, 74) * 1e4
    decay = (torch.arange(n) % 3 != 0).to(torch.uint8).to(DEV)
    for nc in ([1e4, 0.0, 1.0], [float("inf"), 1.0, 0.0], [NAN, 1.0, 0.0]):
        p, m, v, gd = _view(p0, off), _view(m0, off), _view(v0, off), _view(g, off)
        mirror = torch.full((n,), NAN, device=DEV, dtype=BF)
        T.adamw_step_(p, gd, m, v, decay, betas=(0.9, 0.98), step=9, norm_coef=torch.tensor(nc, device=DEV), mirror=mirror, **HP)
        assert same_bits(p.cpu(), p0) and same_bits(m.cpu(), m0) and same_bits(v.cpu(), v0), nc
        assert torch.equal(mirror.cpu(), p0.to(BF))


@pytest.mark.parametrize("name,n,off", SIZES, ids=[s[0] for s in SIZES])
def test_axpy_and_scale_are_exact_with_power_of_two_coefficients(name, n, off):
    """a product by a power of two is exact, so each op has ONE rounding (the add) or none: the device result must equal torch's on the CPU"""
    _, T, _ = _o()
    a, b = _normal(n, 73), _normal(n, 74)

    def twice(fn, want):
        outs = []
        for _ in range(2):
            ad = _view(a, off)
            fn(ad)
            outs.append(ad)
        assert same_bits(outs[0], outs[1]) and same_bits(outs[0].cpu(), want)

    bd = _view(b, off)
    twice(lambda ad: T.axpy_(ad, bd, 0.5), a + 0.5 * b)
    twice(lambda ad: T.axpy_(ad, bd), a + b)
    twice(lambda ad: T.scale_(ad, 0.25), a * 0.25)
    two = torch.tensor([7.0, 2.0], device=DEV)[1:]
    twice(lambda ad: T.axpy_dev_(ad, bd, two), a + 2.0 * b)
    twice(lambda ad: T.axpy_dev_(ad, bd, two, overwrite=True), 2.0 * b)
    nan_start = _view(torch.full((n,), NAN), off)                                # overwrite must not read what it replaces
    T.axpy_dev_(nan_start, bd, two, overwrite=True)
    assert same_bits(nan_start.cpu(), 2.0 * b)
    half, one = torch.tensor([0.5], device=DEV), torch.tensor([1.0], device=DEV)
    if off == 0:
        twice(lambda ad: T.scale_by_device_scalar_(ad, half), a * 0.5)
        twice(lambda ad: T.scale_by_device_scalar_(ad, one), a)
        odd = _view(torch.full((n,), NAN), 0)                                    # alpha == 1 touches nothing: not even a NaN's payload
        odd[1::2] = -0.0
        before = odd.clone()
        T.scale_by_device_scalar_(odd, one)
        assert same_bits(odd, before)
    else:
        with pytest.raises(RuntimeError):                                        # 16-byte steps only: a misaligned buffer is refused, not mis-scaled
            T.scale_by_device_scalar_(_view(a, off), half)


def test_scale_by_device_scalar_shorter_than_one_vector():
    _, T, _ = _o()
    for n in (1, 3, 4, 7):
        a = _normal(n, 93)
        ad = _view(a, 0)
        T.scale_by_device_scalar_(ad, torch.tensor([0.5], device=DEV))
        assert same_bits(ad.cpu(), a * 0.5), n
