"""The attention forward kernels (huggingface_asr_amd/csrc/attention.hip) at mask, shift and cache edges, bit for bit: every selector case of tests/attention_cases.py
expects the gather V[b, winner] with zero tolerance, every family D case (ramps that drive the lazy rescale) stays inside the constant derived on the CPU
(tests/test_attention_cases_cpu.py proves both legitimate).  Every buffer is allocated at full capacity, outputs are poisoned with NaN and must come back fully
written, and every kernel runs twice with bit-identical results."""
import math

import pytest
import torch

import attention_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
NAN = float("nan")

# rows checked exactly / worst family D error (units of 2^-8 (|want| + mean|want|)) per kernel form: printed when the module is done (run with -s)
STATS = {"rows": {}, "d_worst": {}, "lse_worst": 0.0}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nexact-checked rows per kernel form:", dict(sorted(STATS["rows"].items())))
    print("family D worst normalised error per kernel form (bound %.1f):" % AC.D_C, {k: round(v, 3) for k, v in sorted(STATS["d_worst"].items())})
    print("worst |lse| error (log2 domain, bound %.0e): %.3e" % (AC.LSE_TOL, STATS["lse_worst"]))


def _ops():
    from huggingface_asr_amd import ops
    return ops


def _dev(x):
    return x.to(DEV, BF16)


def _poison_next(shape, dtype=BF16):
    """NaN-fill a block of the size an entry is about to allocate for its result and free it: the caching allocator hands the same block back, so an element
    the kernel does not write shows up as NaN (for entries that take no `out`)."""
    t = torch.full(shape, NAN, device=DEV, dtype=dtype)
    del t


def _bits(x):
    return x.contiguous().view(torch.int16) if x.dtype == BF16 else x.contiguous().view(torch.int32)


def _row_mask(case, exact):
    return exact.permute(0, 2, 1).unsqueeze(-1).expand(case.B, case.Tq, case.H, case.hd).reshape(case.B, case.Tq, -1)


_REF = {}


def _reference(case):
    if case.name not in _REF:
        _REF.clear()                                   # cases arrive grouped: one reference alive at a time, shared by a case's variants and entries
        want, lse2, s = AC.reference(case, AC.build(case))
        _REF[case.name] = (want, lse2, s)
    return _REF[case.name]


def _check_ctx(case, form, out, what):
    B, Tq, d = case.B, case.Tq, case.H * case.hd
    got = out.float().cpu().view(B, Tq, d)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written / not finite"
    inp = AC.build(case)
    if case.family == "D":
        want, _, _ = _reference(case)
        e = AC.d_normalised_error(got, want)
        worst = float(e.max())
        print(f"{what}: family D worst normalised error {worst:.3f} (bound {AC.D_C})")
        STATS["d_worst"][form] = max(STATS["d_worst"].get(form, 0.0), worst)
        assert worst <= AC.D_C, f"{what}: {int((e > AC.D_C).sum())} / {e.numel()} elements outside, worst {worst:.3f}"
        return
    want, exact = AC.expected_rows(case, inp)
    m = _row_mask(case, exact)
    bad = got[m] != want[m]
    nbad = int(bad.sum())
    if nbad:
        rows = (got != want) & m
        where = rows.view(B, Tq, case.H, case.hd).any(-1).nonzero()[:6].tolist()
        raise AssertionError(f"{what}: {nbad} / {int(m.sum())} exact-checked elements differ; first (batch, query, head): {where}")
    STATS["rows"][form] = STATS["rows"].get(form, 0) + int(exact.sum())
    if not bool(exact.all()):                          # family C's tied rows
        ref, _, _ = _reference(case)
        e = AC.d_normalised_error(got, ref)[~m]
        assert float(e.max()) <= AC.D_C, f"{what}: tied rows, worst {float(e.max()):.3f}"


def _check_lse(case, lse, what):
    got = lse.float().cpu().double()
    assert bool(torch.isfinite(got).all()), what
    _, lse2, s = _reference(case)
    err = float((got - lse2).abs().max())
    print(f"{what}: worst |lse| error {err:.3e}")
    STATS["lse_worst"] = max(STATS["lse_worst"], err)
    assert err <= AC.LSE_TOL, (what, err)
    if case.family in ("A", "A1"):                     # the winner's score itself
        top = torch.gather(s, 3, AC.build(case)["winner"].unsqueeze(-1)).squeeze(-1) * AC.LOG2E
        assert float((got - top).abs().max()) <= AC.LSE_TOL, what


def _lengths(case):
    return None if case.lengths is None else torch.tensor(case.lengths, dtype=torch.int32, device=DEV)


def _rel_operands(case, inp):
    if not case.rel:
        return dict()
    d = case.H * case.hd
    return dict(pos=_dev(inp["pos"].reshape(-1, d)), bias_u=inp["bias_u"].to(DEV), bias_v=inp["bias_v"].to(DEV))


def _twice(run, what):
    a = run()
    b = run()
    torch.cuda.synchronize()
    outs_a, outs_b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    for x, y in zip(outs_a, outs_b):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: two runs differ"
    return a


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _run_square(case):
    ops = _ops()
    inp = AC.build(case)
    B, T, H, hd = case.B, case.Tq, case.H, case.hd
    d = H * hd
    q, k, v = inp["q"].reshape(B * T, d), inp["k"].reshape(B * T, d), inp["v"].reshape(B * T, d)
    kw = dict(lengths=_lengths(case), causal=case.causal, **_rel_operands(case, inp))
    if case.entry == "reg":
        Tp = (T + 31) // 32 * 32
        qk = _dev(torch.cat([q, k], 1))
        vt = torch.zeros((d, B * Tp), dtype=BF16, device=DEV)
        vt.view(d, B, Tp)[:, :, :T] = _dev(v.t().reshape(d, B, T))

        def run():
            _poison_next((B * T, d))
            return ops.attention(qk[:, :d], qk[:, d:], vt, Tp, B, T, H, **kw)
        _check_ctx(case, "reg", _twice(run, case.name), case.name)
        return
    qkv = _dev(torch.cat([q, k, v], 1))
    if case.entry == "qkv_lse":
        form = AC.forms_of(case)[0]

        def run():
            lse = torch.full((B, H, T), NAN, device=DEV, dtype=torch.float32)
            _poison_next((B * T, d))
            return ops.attention_qkv(qkv, B, T, H, lse=lse, **kw), lse
        out, lse = _twice(run, case.name)
        _check_ctx(case, form, out, case.name)
        if case.family in ("A", "A1", "D"):
            _check_lse(case, lse, case.name)
        return
    for variant, form in zip(case.variants, AC.forms_of(case)):
        def run():
            _poison_next((B * T, d))
            return ops.attention_qkv(qkv, B, T, H, variant=variant, **kw)
        what = f"{case.name} variant {variant} ({form})"
        _check_ctx(case, form, _twice(run, what), what)


@pytest.mark.parametrize("case", [c for c in AC.SQUARE if c.entry == "reg"], ids=lambda c: c.name)
def test_register_kernel_square(case):
    _run_square(case)


@pytest.mark.parametrize("case", [c for c in AC.SQUARE if c.entry == "qkv"], ids=lambda c: c.name)
def test_lds_forms_square(case):
    _run_square(case)


@pytest.mark.parametrize("case", [c for c in AC.SQUARE if c.entry == "qkv_lse"], ids=lambda c: c.name)
def test_lds_lse_square(case):
    _run_square(case)


@pytest.mark.parametrize("case", AC.BLOCKID, ids=lambda c: c.name)
def test_eight_wave_block_ids_at_the_limit(case):
    _run_square(case)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _general_operands(case, inp):
    """q as a column view of a (B*Tq, 3d) buffer; k, v as the (B*Lmax, d) caches or as views of a (B*Tk, 2d) buffer, as decoder.py passes them."""
    B, H, hd, Tq, Tk = case.B, case.H, case.hd, case.Tq, case.Tk
    d = H * hd
    qbuf = torch.zeros((B * Tq, 3 * d), dtype=BF16, device=DEV)
    qbuf[:, :d] = _dev(inp["q"].reshape(B * Tq, d))
    if case.Lmax:
        k, v = _dev(inp["k"].reshape(B * case.Lmax, d)), _dev(inp["v"].reshape(B * case.Lmax, d))
        return qbuf[:, :d], k, v, case.Lmax * d
    kv = _dev(torch.cat([inp["k"].reshape(B * Tk, d), inp["v"].reshape(B * Tk, d)], 1))
    return qbuf[:, :d], kv[:, :d], kv[:, d:], 0


def _run_general(case, strided_out=False):
    ops = _ops()
    inp = AC.build(case)
    B, H, Tq, Tk = case.B, case.H, case.Tq, case.Tk
    d = H * case.hd
    q, k, v, bstride = _general_operands(case, inp)
    for variant, form in zip(case.variants, AC.forms_of(case)):
        what = f"{case.name} variant {variant} ({form})"

        def run():
            obuf = torch.full((B * Tq, 2 * d if strided_out else d), NAN, device=DEV, dtype=BF16)
            out = obuf[:, d:] if strided_out else obuf
            ops.attention_general(q, k, v, B, Tq, Tk, H, lengths=_lengths(case), causal=case.causal, out=out, kv_bstride=bstride, variant=variant)
            if strided_out:
                assert bool(torch.isnan(obuf[:, :d]).all()), f"{what}: wrote outside the strided output view"
            return out.contiguous()
        _check_ctx(case, form, _twice(run, what), what)


@pytest.mark.parametrize("case", [c for c in AC.CACHE if c.group == "step"], ids=lambda c: c.name)
def test_general_kv_cache_step(case):
    _run_general(case)


@pytest.mark.parametrize("case", [c for c in AC.CACHE if c.group == "chunk"], ids=lambda c: c.name)
def test_general_chunked_append(case):
    _run_general(case)


_CROSS_GENERAL = [c for c in AC.CROSS if c.entry == "general"]


@pytest.mark.parametrize("case", _CROSS_GENERAL, ids=lambda c: c.name)
def test_general_cross_attention(case):
    _run_general(case, strided_out=_CROSS_GENERAL.index(case) % 3 == 1)


@pytest.mark.parametrize("case", [c for c in AC.CROSS if c.entry == "xlse"], ids=lambda c: c.name)
def test_training_forward_x_lse(case):
    from huggingface_asr_amd import ops_train as OT
    inp = AC.build(case)
    B, H, Tq, Tk = case.B, case.H, case.Tq, case.Tk
    d = H * case.hd
    q, k, v, _ = _general_operands(case, inp)
    form = AC.forms_of(case)[0]

    def run():
        _poison_next((B, H, Tq), torch.float32)
        _poison_next((B * Tq, d))
        return OT.attention_x_lse(q, k, v, B, Tq, Tk, H, lengths=_lengths(case), causal=case.causal)
    out, lse = _twice(run, case.name)
    _check_ctx(case, form, out, case.name)
    if case.family in ("A", "D"):
        _check_lse(case, lse, case.name)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
def _refused_operands(Tq=40, Tk=33, H=2, hd=64, B=2):
    d = H * hd
    gen = torch.Generator().manual_seed(3)
    q = torch.randn(B * Tq, d, generator=gen).to(DEV, BF16)
    kv = torch.randn(B * Tk, 2 * d, generator=gen).to(DEV, BF16)
    return B, Tq, Tk, H, d, q, kv[:, :d], kv[:, d:]


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_causal_with_fewer_keys_than_queries_is_refused_general(variant):
    """causal with 0 < Tk < Tq: the first queries see no key (l = 0, the row is 0 * inf).  mi_attention_qkv_bf16 / mi_attention_qkv_bf16_v refuse it and launch nothing."""
    ops = _ops()
    B, Tq, Tk, H, d, q, k, v = _refused_operands()
    out = torch.full((B * Tq, d), NAN, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError, match="mi_attention_qkv_bf16"):
        ops.attention_general(q, k, v, B, Tq, Tk, H, causal=True, out=out, variant=variant)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    ops.attention_general(q, k, v, B, Tq, Tk, H, causal=False, out=out, variant=variant)          # the same call without the mask is fine
    assert bool(torch.isfinite(out.float()).all())


def test_causal_with_fewer_keys_than_queries_is_refused_x_lse():
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd import ops_train as OT
    B, Tq, Tk, H, d, q, k, v = _refused_operands()
    out = torch.full((B * Tq, d), NAN, device=DEV, dtype=BF16)
    lse = torch.full((B, H, Tq), NAN, device=DEV, dtype=torch.float32)
    rc = _lib.lib().mi_attention_x_lse_bf16(q.data_ptr(), q.stride(0), k.data_ptr(), k.stride(0), v.data_ptr(), v.stride(0), 0, out.data_ptr(), out.stride(0),
                                            lse.data_ptr(), B, Tq, Tk, H, d // H, 1.0 / math.sqrt(d // H), 1, 0.0, 0, 0, OT._stream())
    with pytest.raises(RuntimeError, match="mi_attention_x_lse_bf16"):
        _lib.check(rc, "mi_attention_x_lse_bf16")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(lse).all())
    with pytest.raises(RuntimeError, match="mi_attention_x_lse_bf16"):
        OT.attention_x_lse(q, k, v, B, Tq, Tk, H, causal=True)


def test_causal_with_fewer_keys_than_queries_is_refused_x_bwd_probs():
    from huggingface_asr_amd import ops_train as OT
    B, Tq, Tk, H, d, q, k, v = _refused_operands()
    ctx, lse = OT.attention_x_lse(q, k, v, B, Tq, Tk, H)
    dq = torch.full((B * Tq, d), NAN, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError, match="mi_attention_x_bwd_probs"):
        OT.attn_x_bwd_probs(q, k, v, B, Tq, Tk, H, ctx, ctx, lse, dq, causal=True)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dq).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusal_table_bases_are_valid_calls():
    """The six base calls of tests/attention_arg_cases.py on real tensors of their dimensions and strides: each returns 0 and writes finite values everywhere, so the
    one defect of each mutation (tests/test_attention_args_cpu.py) is what refuses it.  The backward bases read the context and log-sum-exp their forward bases leave."""
    import attention_arg_cases as A
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd import ops_train as OT
    gen = torch.Generator().manual_seed(11)
    dims = A.BASES["mi_attention_qkv_bwd_probs"]
    B, T, H, hd, Tk = dims["B"], dims["T"], dims["H"], dims["hd"], A.BASES["mi_attention_x_bwd_probs"]["Tk"]
    d = H * hd

    def rnd(*shape, dtype=BF16):
        return (0.5 * torch.randn(*shape, generator=gen)).to(DEV, dtype)

    def poison(*shape, dtype=BF16):
        return torch.full(shape, NAN, device=DEV, dtype=dtype)

    qkv, xq, xkv = rnd(B * T, 3 * d), rnd(B * T, d), rnd(B * Tk, 2 * d).chunk(2, dim=1)
    shared = dict(pos=rnd(2 * T - 1, d), bias_u=rnd(H, hd, dtype=torch.float32), bias_v=rnd(H, hd, dtype=torch.float32), dctx=rnd(B * T, d))
    operands = {"qkv": dict(shared, q=qkv[:, :d], k=qkv[:, d:2 * d], v=qkv[:, 2 * d:], lengths=torch.tensor([T, 25], dtype=torch.int32, device=DEV)),
                "x": dict(shared, q=xq, k=xkv[0].contiguous(), v=xkv[1].contiguous(), lengths=torch.tensor([Tk, 20], dtype=torch.int32, device=DEV))}
    nw = 4 * ((T + 127) // 128)
    for entry in ("mi_attention_qkv_bf16", "mi_attention_qkv_bf16_v", "mi_attention_qkv_lse_bf16", "mi_attention_qkv_bwd_probs", "mi_attention_x_lse_bf16", "mi_attention_x_bwd_probs"):
        base, ops_ = A.BASES[entry], operands["x" if "_x_" in entry else "qkv"]
        fwd = "bwd" not in entry
        outs = dict(out=poison(B * T, d), lse=poison(B, H, T, dtype=torch.float32)) if fwd else \
            dict(prob=poison(H, B, T, base["ldsr"]), ds=poison(H, B, T, base["ldsr"]), dq=poison(B * T, d), dbd=poison(H, B, T, base.get("ldbd", 32)),
                 dsum_u=poison(B, nw, d, dtype=torch.float32), dsum_v=poison(B, nw, d, dtype=torch.float32), qu_out=poison(B * T, d), qv_out=poison(B * T, d))
        outs = {n: t for n, t in outs.items() if base.get(n)}
        tensors = dict(ops_, **outs)
        for n, ld in (("q", "ldq"), ("k", "ldk"), ("v", "ldv"), ("pos", "ldp"), ("out", "ldo"), ("ctx", "ldo"), ("dctx", "ldd"), ("dq", "lddq"), ("qu_out", "ldqb")):
            if base.get(n):
                assert tensors[n].stride(0) == base[ld], (entry, n)
        args = [tensors[n].data_ptr() if n in A.POINTERS and base[n] else base[n] for n in A.PARAMS[entry]]
        rc = getattr(_lib.lib(), entry)(*args, OT._stream())
        torch.cuda.synchronize()
        assert rc == 0, entry
        for n, t in outs.items():
            assert bool(torch.isfinite(t.float()).all()), (entry, n)
        if entry.endswith("_lse_bf16"):
            operands["x" if "_x_" in entry else "qkv"].update(ctx=outs["out"], lse=outs["lse"])
