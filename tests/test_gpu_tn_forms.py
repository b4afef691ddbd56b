"""Every form of the two GEMM families of the backward pass — the weight-gradient GEMM (huggingface_asr_amd/csrc/gemm_tn.hip) and the strided batched GEMM of the
materialising attention backward (huggingface_asr_amd/csrc/bgemm.hip) — at the smallest sizes at which its stage loop, its ring, its M splits and its tile masks can
go wrong, compared bit for bit.  The cases, the references and the reasoning that makes zero tolerance legitimate live in tests/tn_cases.py;
tests/test_tn_cases_cpu.py checks them without a GPU.  Every comparison is `torch.equal` against the float64-derived expectation.

  a. mi_gemm_tn_bf16: the 128 x 128 and 128 x 64 tiles at 1 ... 4 stages, every class of ragged last stage, 1 / 2 / 3 / 5 splits and a split without rows; the
     256 x 256 tile split over M (M >= 32768) and, one row below it, the 128 tile on the same operands; the per-lane pointer loader behind the 4 GiB bound on both
     tiles.  Every launch ADDS: the target starts from integers, the call is made twice (the second adds again), and a tile written twice would show.
  b. mi_conv2d_wgrad_cl_bf16: the gathered loader on the 128 tile and on the 256 x 256 tile against float64 F.conv2d autograd.
  c. mi_gemm_tn_group_ow_bf16 through ctypes (ops_train.TnBatch runs small grids one by one): both output tiles, 1 ... 5 stages against ring depths 3 and 2, block
     counts that are no multiple of 8 (the XCD permutation), 1 ... 48 problems (the tile0 search), overwrite on NaN targets and add on integer targets; refusals.
  d. mi_bgemm_sparse_bf16: four operand layouts x {64, 128 tile} x {branch-free, guarded loads}, K at every tile-count edge, the band and m_valid on both tiles.

Operands are views inside NaN-filled buffers, outputs views inside NaN-filled buffers with guard rows: what a kernel must not use or write is NaN before the launch
and must be NaN after it.  WHICH kernel a case reaches is not observable (no profiling slot): it rests on the restated dispatch of tests/tn_cases.py.
Every launch is repeated into the re-poisoned output and must give the same bits.
"""
import ctypes as C

import pytest
import torch

import tn_cases as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32
GUARD = 8                    # rows below an output that no launch may touch
NAN = float("nan")


def _mods():
    from huggingface_asr_amd import _lib, ops_train
    from huggingface_asr_amd.ops import _stream
    return _lib, ops_train, _stream


def nanbuf(shape, dtype):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def place(x, cols, off, guard=GUARD):
    """x (R, W) float64 as the bf16 device view buf[:R, off:off+W] of a NaN-filled (R + guard, cols) buffer"""
    R, W = x.shape
    v = nanbuf((R + guard, cols), BF)[:R, off:off + W]
    v.copy_(x.to(BF))
    return v


def assert_same(got, want, what):
    want = want.to(got.device)
    bad = got != want                                   # (NaN left in an output cell compares unequal too)
    if bool(bad.any()):
        first = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.numel()} wrong, first at {list(first)}: got {float(got[first])}, want {float(want[first])}")
    assert torch.equal(got, want), what


class Target:
    """dW as the view buf[:n_store, off:off+K] of a NaN-filled (N + GUARD, ldo) buffer — the rows from n_store on, the columns beside the view and the guard rows must
    stay NaN — and db as the head of a NaN-filled (N + GUARD) vector"""

    def __init__(self, N, K, n_store, lo, db):
        self.big = nanbuf((N + GUARD, lo.ldo), F32)
        self.view = self.big[:n_store, lo.w_off:lo.w_off + K]
        self.own = torch.zeros_like(self.big, dtype=torch.bool)
        self.own[:n_store, lo.w_off:lo.w_off + K] = True
        self.db_big = nanbuf((N + GUARD,), F32) if db else None
        self.db = self.db_big[:n_store] if db else None
        self.n_store = n_store

    def reset(self, bw=None, bb=None):
        """NaN everywhere; then the integers an adding launch starts from (None: an overwriting launch starts from NaN)"""
        self.big.fill_(NAN)
        if bw is not None:
            self.view.copy_(bw)
        if self.db is not None:
            self.db_big.fill_(NAN)
            if bb is not None:
                self.db.copy_(bb)

    def check(self, want_w, want_b, what):
        assert_same(self.view, want_w.float(), f"{what}: dW")
        touched = ~torch.isnan(self.big) & ~self.own
        assert not bool(touched.any()), f"{what}: {int(touched.sum())} cells outside dW were written, first at {touched.nonzero()[0].tolist()}"
        if self.db is not None:
            assert_same(self.db, want_b.float(), f"{what}: db")
            assert bool(torch.isnan(self.db_big[self.n_store:]).all()), f"{what}: db written past n_store"

    def bits(self):
        return self.big.clone(), (self.db_big.clone() if self.db is not None else None)

    def assert_bits(self, bits, what):
        assert torch.equal(self.big.view(torch.int32), bits[0].view(torch.int32)), f"{what}: dW not the same bits launch to launch"
        if self.db is not None:
            assert torch.equal(self.db_big.view(torch.int32), bits[1].view(torch.int32)), f"{what}: db not the same bits launch to launch"


def add_twice_then_repeat(launch, tgt, bw, bb, ref, what):
    """the adding launches' protocol: integers + one call, + a second call, then one call into the re-poisoned target with the first call's bits"""
    tgt.reset(bw, bb)
    launch()
    tgt.check(*ref(1), what)
    first = tgt.bits()
    launch()
    tgt.check(*ref(2), f"{what} (second adding call)")
    tgt.reset(bw, bb)
    launch()
    tgt.assert_bits(first, what)


# ----------------------------------------------------------------------------------------------------------------- a
def huge_view(x, ld, off):
    """x (M, K) as a column view of an UNINITIALISED (M, ld) bf16 buffer of which only the view and the 8 columns on either side (NaN) are filled"""
    M, K = x.shape
    buf = torch.empty((M, ld), device=DEV, dtype=BF)
    buf[:, off - 8:off + K + 8] = NAN
    v = buf[:, off:off + K]
    v.copy_(x.to(BF))
    return v


@pytest.mark.parametrize("c", T.TN_CASES, ids=lambda c: f"{T.tn_case_plan(c).form}-{c.id}")
def test_weight_gradient_exact(c):
    _, ops_train, _ = _mods()
    lo = T.tn_layout(c)
    if c.xwide:
        free, _total = torch.cuda.mem_get_info()
        if free < 8 * 2 ** 30:
            pytest.skip(f"the 4 GiB operand needs 8 GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    dy, x, bw, bb = T.tn_inputs(c)
    dyd = place(dy, lo.ldy, lo.y_off)
    xd = huge_view(x, lo.ldx, lo.x_off) if c.xwide else place(x, lo.ldx, lo.x_off)
    assert dyd.stride(0) == lo.ldy and xd.stride(0) == lo.ldx and dyd.data_ptr() % 16 == 0 and xd.data_ptr() % 16 == 0
    assert T.fast_ok(c.M, dyd.stride(0), xd.stride(0)) == (not c.xwide)
    tgt = Target(c.N, c.K, c.n_store, lo, c.db)
    assert tgt.view.stride(0) == lo.ldo

    def launch():
        ops_train.gemm_tn_(tgt.view, dyd, xd, n_store=c.n_store, db=tgt.db, variant=c.variant)

    add_twice_then_repeat(launch, tgt, bw, bb, lambda n: T.tn_reference(c, n), c.id)
    if c.xwide:
        del xd
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("c", T.CONV_CASES, ids=lambda c: f"{T.conv_plan(c).form}-{c.id}")
def test_conv_weight_gradient_exact(c):
    _lib, _, _stream = _mods()
    L = _lib.lib()
    M, N, K = T.conv_mnk(c)
    Tin, Fin = T.conv_dims(c)
    x, dy, bw, bb = T.conv_inputs(c)
    flat = nanbuf((x.numel() + 2 * c.Cin,), BF)                     # one pixel of NaN before and after the activation
    xd = flat[c.Cin:c.Cin + x.numel()].view(x.shape)
    xd.copy_(x.to(BF))
    dyd = place(dy, T.conv_ldy(c), 8 if c.views else 0)
    lo = T.TnLayout(0, 0, 0, 0, 4, K + 12) if c.views else T.TnLayout(0, 0, 0, 0, 0, K)
    tgt = Target(N, K, c.n_store, lo, c.db)
    nbytes = L.mi_gemm_tn_workspace_bytes(M, N, K)
    ws = torch.empty(max(nbytes, 16), device=DEV, dtype=torch.uint8)
    assert xd.data_ptr() % 16 == 0 and dyd.data_ptr() % 16 == 0

    def launch():
        _lib.check(L.mi_conv2d_wgrad_cl_bf16(dyd.data_ptr(), dyd.stride(0), xd.data_ptr(), tgt.view.data_ptr(), lo.ldo, tgt.db.data_ptr() if c.db else None,
                                             c.B, Tin, Fin, c.Cin, c.KH, c.KW, c.stride, c.pad_t, c.pad_f, c.Tout, c.Fout, N, c.n_store,
                                             ws.data_ptr() if nbytes else None, nbytes, _stream()), "mi_conv2d_wgrad_cl_bf16")

    add_twice_then_repeat(launch, tgt, bw, bb, lambda n: T.conv_reference(c, n), c.id)


# ----------------------------------------------------------------------------------------------------------------- c
class GroupCall:
    """the operands, targets and host arrays of one grouped launch"""

    def __init__(self, problems, inputs):
        self.problems, self.inputs = problems, inputs
        self.dy, self.x, self.tg = [], [], []
        for p, (dy, x, *_rest) in zip(problems, inputs):
            lo = T.prob_layout(p)
            self.dy.append(place(dy, lo.ldy, lo.y_off))
            self.x.append(place(x, lo.ldx, lo.x_off))
            self.tg.append(Target(p.N, p.K, p.n_store, lo, p.db))
        self.arrays = {"ldy": [t.stride(0) for t in self.dy], "ldx": [t.stride(0) for t in self.x], "ldo": [T.prob_layout(p).ldo for p in problems],
                       "M": [p.M for p in problems], "N": [p.N for p in problems], "K": [p.K for p in problems], "n_store": [p.n_store for p in problems]}

    def reset(self, add):
        for t, (_, _, bw, bb, _, _) in zip(self.tg, self.inputs):
            t.reset(bw if add else None, bb if add else None)

    def launch(self, L, stream, tile_k, overwrite, n=None, edits=None):
        m = len(self.problems)
        a = {k: list(v) for k, v in self.arrays.items()}
        for name, e in (edits or {}).items():
            for i, v in e.items():
                a[name][i] = v
        vp, lg, it = (C.c_void_p * m), (C.c_long * m), (C.c_int * m)
        return L.mi_gemm_tn_group_ow_bf16(m if n is None else n, vp(*[t.data_ptr() for t in self.dy]), lg(*a["ldy"]), vp(*[t.data_ptr() for t in self.x]), lg(*a["ldx"]),
                                          vp(*[t.view.data_ptr() for t in self.tg]), lg(*a["ldo"]), vp(*[(t.db.data_ptr() if t.db is not None else None) for t in self.tg]),
                                          it(*a["M"]), it(*a["N"]), it(*a["K"]), it(*a["n_store"]), int(tile_k), int(overwrite), stream)

    def check(self, calls, add, what):
        for i, (t, (_, _, bw, bb, prod, col)) in enumerate(zip(self.tg, self.inputs)):
            t.check((bw if add else 0) + calls * prod, (bb if add else 0) + calls * col, f"{what}, problem {i} {tuple(self.problems[i])}")


@pytest.mark.parametrize("c", T.GROUP_CASES, ids=lambda c: f"g{T.group_plan(c)[0]}-{c.id}")
def test_grouped_weight_gradients_exact(c):
    _lib, _, _stream = _mods()
    L = _lib.lib()
    g = GroupCall(c.problems, [T.prob_inputs(p, i) for i, p in enumerate(c.problems)])
    add = not c.overwrite
    g.reset(add)
    assert g.launch(L, _stream(), c.tile_k, c.overwrite) == 0
    g.check(1, add, c.id)
    first = [t.bits() for t in g.tg]
    if add:
        assert g.launch(L, _stream(), c.tile_k, 0) == 0
        g.check(2, True, f"{c.id} (second adding call)")
    else:                                                             # an overwriting launch into targets that hold something else: stored, not added
        for t in g.tg:
            t.view.fill_(5.0)
            if t.db is not None:
                t.db.fill_(-7.0)
        assert g.launch(L, _stream(), c.tile_k, 1) == 0
        g.check(1, False, f"{c.id} (overwriting launch into filled targets)")
    g.reset(add)
    assert g.launch(L, _stream(), c.tile_k, c.overwrite) == 0
    for t, b in zip(g.tg, first):
        t.assert_bits(b, c.id)


@pytest.mark.parametrize("what", list(T.GROUP_REFUSALS))
def test_grouped_entry_refusals_leave_the_targets_untouched(what):
    _lib, _, _stream = _mods()
    L = _lib.lib()
    n, edits, tile_k = T.GROUP_REFUSALS[what]
    problems = (T.Prob(65, 136, 264, 131, True, True),) * 3
    g = GroupCall(problems, [T.prob_inputs(p, i) for i, p in enumerate(problems)])
    for ow in (0, 1):
        g.reset(False)
        assert g.launch(L, _stream(), tile_k, ow, n=n, edits=edits) == _lib.ERR_ARG, what
        torch.cuda.synchronize()
        for t in g.tg:
            assert bool(torch.isnan(t.big).all()) and bool(torch.isnan(t.db_big).all()), what


# ----------------------------------------------------------------------------------------------------------------- d
def bg_operand(x, lay):
    """x (Z1, Z2, R, K) float64 as the as_strided bf16 view of a flat NaN buffer laid out by tn_cases.operand_layout"""
    flat = nanbuf((lay.size,), BF)
    v = flat.as_strided(lay.shape, lay.strides, lay.off)
    v.copy_(x.to(BF))
    assert (v.data_ptr() % 16 == 0) == (lay.off % 8 == 0)
    return v


class BgOut:
    """C (Z1, Z2, M, N) as a strided view of a flat NaN buffer (tn_cases.c_layout): a guard row between batch entries, columns beside the view"""

    def __init__(self, Z1, Z2, M, N, out_f32, view):
        self.lay = lay = T.c_layout(Z1, Z2, M, N, view)
        self.flat = nanbuf((lay.size,), F32 if out_f32 else BF)
        self.shape, self.strides = (Z1, Z2, M, N), (lay.z1, lay.z2, lay.ldc, 1)
        self.view = self.flat.as_strided(self.shape, self.strides, lay.off)
        self.own = torch.zeros(lay.size, device=DEV, dtype=torch.bool)
        self.own.as_strided(self.shape, self.strides, lay.off).fill_(True)
        self.c_str = (lay.z1, lay.z2, lay.ldc)

    def reset(self, base=None):
        self.flat.fill_(NAN)
        if base is not None:
            self.view.copy_(base)

    def check(self, want, what):
        assert_same(self.view, want, what)
        touched = ~torch.isnan(self.flat) & ~self.own
        assert not bool(touched.any()), f"{what}: {int(touched.sum())} cells outside C were written, first at {touched.nonzero()[0].tolist()}"

    def run_check_repeat(self, launch, base, want, what):
        self.reset(base)
        launch()
        self.check(want, what)
        first = self.flat.clone()
        self.reset(base)
        launch()
        assert torch.equal(self.flat.view(torch.int16 if self.flat.dtype == BF else torch.int32), first.view(torch.int16 if first.dtype == BF else torch.int32)), \
            f"{what}: not the same bits launch to launch"


def _bg_id(c):
    tile, fast = T.bg_form(c)
    return f"t{tile}-" + ("fast" if fast else "guarded") + f"-{c.id}"


@pytest.mark.parametrize("c", T.BG_CASES, ids=_bg_id)
def test_bgemm_exact(c):
    _, ops_train, _ = _mods()
    a, b, base = T.bg_inputs(c)
    la, lb = T.bg_layouts(c)
    ad, bd = bg_operand(a, la), bg_operand(b, lb)
    out = BgOut(c.Z1, c.Z2, c.M, c.N, c.out_f32, c.c_view)
    want = T.bg_expected(T.bg_reference(c), c.out_f32)

    def launch():
        ops_train.bgemm(ad, la.strides, bd, lb.strides, out.view, out.c_str, c.Z1, c.Z2, c.M, c.N, c.K, alpha=c.alpha, accumulate=c.accumulate)

    out.run_check_repeat(launch, base, want, c.id)


@pytest.mark.parametrize("c", T.BAND_CASES, ids=lambda c: f"t{T.band_form(c)[0]}-" + ("fast" if T.band_form(c)[1] else "guarded") + f"-{c.id}")
def test_bgemm_band_exact(c):
    """the d(positions) product on the real band geometry, with and without the band argument, against the float64 einsum"""
    _, ops_train, _ = _mods()
    dbd, qv = T.band_inputs(c)
    off, Kp = T.band_geometry(c.Tt)
    assert (off, Kp) == ops_train.band_geometry(c.Tt)
    B, d = c.G * c.cg, c.H * c.hd
    dbd_d = dbd.to(DEV, BF)
    qoff = 4 if c.guard == "b_off4" else 0
    qv_d = nanbuf((qv.numel() + 16,), BF)[qoff:qoff + qv.numel()].view(qv.shape)
    qv_d.copy_(qv.to(BF))
    assert (qv_d.data_ptr() % 16 == 0) == (qoff == 0)
    want = T.band_reference(c).float()
    dpp = nanbuf((c.G + 1, Kp * d), F32)                              # one guard row
    first = None
    for band in ((c.Tt, c.Tt - 1 + off, c.cg), None, (c.Tt, c.Tt - 1 + off, c.cg)):
        dpp.fill_(NAN)
        ops_train.bgemm(dbd_d, (B * c.Tt * Kp, c.cg * c.Tt * Kp, 1, Kp), qv_d, (c.hd, c.cg * c.Tt * d, 1, d), dpp, (c.hd, Kp * d, d), c.H, c.G, Kp, c.hd, c.cg * c.Tt, band=band)
        assert_same(dpp[:c.G], want, f"{c.id} band={band}")
        assert bool(torch.isnan(dpp[c.G:]).all())
        if first is None:
            first = dpp.clone()
        else:                                                         # the walk over all of K, and the repeated banded launch: the first launch's bits
            assert torch.equal(dpp.view(torch.int32), first.view(torch.int32)), f"{c.id} band={band}: not the same bits as the first launch"


@pytest.mark.parametrize("c", T.MV_CASES, ids=lambda c: c.id)
def test_bgemm_dead_row_tiles_exact(c):
    """m_valid: live tiles multiply true zeros past the count, dead tiles (NaN in A: a multiplied one would show) are stored as zeros — or left alone when accumulating"""
    _, ops_train, _ = _mods()
    Z2 = len(c.lens)
    a, b, base = T.mv_inputs(c)
    a = a.clone()
    for z in range(Z2):
        a[:, z, T.mv_dead_rows(c, z):] = NAN
    la = T.operand_layout(c.la, c.Z1, Z2, c.M, c.K, "fast", 0, False)
    lb = T.operand_layout(1 - c.la, c.Z1, Z2, c.N, c.K, "fast", 8, True)
    ad, bd = bg_operand(a, la), bg_operand(b, lb)
    lens = torch.tensor(c.lens, dtype=torch.int32, device=DEV)
    out = BgOut(c.Z1, Z2, c.M, c.N, c.out_f32, True)
    want = T.bg_expected(T.mv_reference(c), c.out_f32)

    def launch():
        ops_train.bgemm(ad, la.strides, bd, lb.strides, out.view, out.c_str, c.Z1, Z2, c.M, c.N, c.K, accumulate=c.accumulate, m_valid=lens)

    out.run_check_repeat(launch, base if c.accumulate else None, want, c.id)
