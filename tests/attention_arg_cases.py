"""The refusal table of the LDS-staged attention entries (csrc/attention.hip): for each of the six C entries one VALID base call at the smallest shape its argument
checks can tell apart, and single-defect mutations of it with the return code the entry must give.  No GPU code here: tests/test_attention_args_cpu.py calls every
mutation with the fake addresses below (each is refused before anything is launched or dereferenced), tests/test_gpu_attention_probes.py runs the six bases on real
tensors of the same dimensions and strides (each returns 0: a mutation's one defect is therefore what refuses it).

The expected codes are literals RECORDED from the library as it stood before the entries' checks were merged into shared functions (the backward-probs entry: from its then
`_f` form), not derived from the code under test: -1 = MI_ERR_ARG, -3 = MI_ERR_UNSUPPORTED.  A case overrides only the fields of its defect; where the defect needs a call
without relative positions (the `pos` rules would be a second defect), NO_POS drops that operand group, which is itself a valid call — the two `x` bases run without it.

Shape: B = 2, T = 40 (two 32-query waves, the second ragged), H = 2, hd = 64; fused (B*T, 384) projection for the qkv entries, (., 128) operands with Tq = 40, Tk = 33 for
the x entries; positions (79, 128); backward: ldsr = 64 (T rounded up to 32), pad = 24 ((T - 32 + pad) % 32 == 0), ldbd = 128 (>= pad + 2T - 1 = 103)."""
ARG, UNSUPPORTED = -1, -3
BIG = 1 << 30          # the kernels keep row strides as 32-bit byte counts: strides of 2^30 elements and more are refused

_FWD = "q ldq k ldk v ldv pos ldp bias_u bias_v lengths out ldo"
_BWD = "q ldq k ldk v ldv pos ldp bias_u bias_v lengths ctx ldo dctx ldd lse prob ds ldsr dbd ldbd pad dq lddq dsum_u dsum_v qu_out qv_out ldqb"
_DROP = "drop_p seed stream_id"
# argument order of each entry (include/hfasr_hip.h), without the trailing stream
PARAMS = {
    "mi_attention_qkv_bf16": f"{_FWD} B T Tk kv_bstride H hd scale causal".split(),
    "mi_attention_qkv_bf16_v": f"{_FWD} B T Tk kv_bstride H hd scale causal variant".split(),
    "mi_attention_qkv_lse_bf16": f"{_FWD} lse B T H hd scale causal {_DROP}".split(),
    "mi_attention_qkv_bwd_probs": f"{_BWD} B T H hd scale causal {_DROP} flags".split(),
    "mi_attention_x_lse_bf16": f"q ldq k ldk v ldv lengths out ldo lse B T Tk H hd scale causal {_DROP}".split(),
    "mi_attention_x_bwd_probs": f"q ldq k ldk v ldv lengths ctx ldo dctx ldd lse prob ds ldsr dq lddq B T Tk H hd scale causal {_DROP}".split(),
}
# the fields that are addresses: the CPU test passes the fake (256-byte aligned, never dereferenced) values below, the GPU test real tensors
POINTERS = ("q", "k", "v", "pos", "bias_u", "bias_v", "lengths", "out", "lse", "ctx", "dctx", "prob", "ds", "dbd", "dq", "dsum_u", "dsum_v", "qu_out", "qv_out")
_FAKE = {name: 0x100000 * (i + 1) for i, name in enumerate(POINTERS)}

_DIMS = dict(B=2, T=40, H=2, hd=64, scale=0.125, causal=0)
_QKV = dict(_DIMS, ldq=384, ldk=384, ldv=384, ldp=128, ldo=128, **{n: _FAKE[n] for n in ("q", "k", "v", "pos", "bias_u", "bias_v", "lengths", "out")})
_X = dict(_DIMS, Tk=33, ldq=128, ldk=128, ldv=128, ldo=128, lengths=_FAKE["lengths"], q=_FAKE["q"], k=_FAKE["k"], v=_FAKE["v"])
_NO_DROP = dict(drop_p=0.0, seed=0, stream_id=0)
_BW = dict(ldd=128, ldsr=64, lddq=128, **{n: _FAKE[n] for n in ("ctx", "dctx", "lse", "prob", "ds", "dq")})
BASES = {
    "mi_attention_qkv_bf16": dict(_QKV, Tk=0, kv_bstride=0),
    "mi_attention_qkv_bf16_v": dict(_QKV, Tk=0, kv_bstride=0, variant=0),
    "mi_attention_qkv_lse_bf16": dict(_QKV, lse=_FAKE["lse"], **_NO_DROP),
    "mi_attention_qkv_bwd_probs": dict({k: v for k, v in _QKV.items() if k != "out"}, **_BW, **_NO_DROP, ldbd=128, pad=24, ldqb=128, flags=0,
                                       **{n: _FAKE[n] for n in ("dbd", "dsum_u", "dsum_v", "qu_out", "qv_out")}),
    "mi_attention_x_lse_bf16": dict(_X, out=_FAKE["out"], lse=_FAKE["lse"], **_NO_DROP),
    "mi_attention_x_bwd_probs": dict(_X, **_BW, **_NO_DROP),
}
NO_POS = dict(pos=0, ldp=0, bias_u=0, bias_v=0)
assert all(set(BASES[e]) == set(PARAMS[e]) for e in PARAMS)


def _each(fields, change, what, code):
    return [(f"{f} {what}", {f: change(f)}, code) for f in fields]


def _off4(entry, fields):          # a row stride that is no multiple of 8 elements (16 bytes)
    return _each(fields, lambda f: BASES[entry][f] + 4, "+ 4", ARG)


def _off8(entry, fields):          # an address 8 bytes off its 16-byte alignment
    return _each(fields, lambda f: BASES[entry][f] + 8, "+ 8 bytes", ARG)


def _forward(entry):
    """What every LDS-staged entry refuses, forward or backward (the x entries have no pos)."""
    qkv = "pos" in BASES[entry]
    return (_each(("B", "T", "H"), lambda f: 0, "= 0", ARG) + _off4(entry, ("ldq", "ldk", "ldv", "ldo")) + _off8(entry, ("q", "k", "v"))
            + _each(("ldq", "ldk", "ldv"), lambda f: BIG, "= 2^30", ARG) + _each(("ldk", "ldv"), lambda f: 0, "= 0", ARG)
            + [("hd = 48", dict(hd=48), UNSUPPORTED), ("hd = 48 and ldq + 4: the argument error comes first", dict(hd=48, ldq=BASES[entry]["ldq"] + 4), ARG),
               ("hd = 48 and ldo + 4: the argument error comes first", dict(hd=48, ldo=132), ARG)]
            + (_off4(entry, ("ldp",)) + _off8(entry, ("pos",)) + _each(("ldp",), lambda f: BIG, "= 2^30", ARG) + _each(("bias_u", "bias_v"), lambda f: 0, "null with pos", ARG)
               if qkv else []))


def _general(entry):
    """mi_attention_qkv_bf16 / _v: keys per batch and the KV-cache batch stride."""
    return (_off8(entry, ("out",))
            + [("Tk = -1", dict(NO_POS, Tk=-1), ARG), ("pos with Tk = 33: the relative term needs a square score matrix", dict(Tk=33), ARG),
               ("pos with Tk = 41", dict(Tk=41), ARG), ("causal with Tk = 33 < T", dict(NO_POS, causal=1, Tk=33), ARG), ("kv_bstride + 4", dict(kv_bstride=40 * 384 + 4), ARG)])


def _training():
    return [("lse null", dict(lse=0), ARG), ("drop_p = -0.1", dict(drop_p=-0.1), ARG), ("drop_p = 1.0", dict(drop_p=1.0), ARG)]


def _x():
    return [("Tk = 0", dict(Tk=0), ARG), ("Tk = -1", dict(Tk=-1), ARG), ("causal with Tk = 33 < Tq", dict(causal=1), ARG)]


def _backward(entry):
    """What both backward entries refuse beyond the forward's checks."""
    return (_each(("ctx", "dctx", "prob", "ds", "dq"), lambda f: 0, "null", ARG) + _off8(entry, ("ctx", "dctx", "prob", "ds", "dq")) + _off4(entry, ("ldd", "lddq"))
            + _each(("ldo", "ldd", "lddq"), lambda f: BIG, "= 2^30", ARG)
            + [("ldsr = 48: no multiple of 32", dict(ldsr=48), ARG), ("ldsr = 32 < the keys rounded up to 32", dict(ldsr=32), ARG)])


_BAND = [("dbd + 8 bytes", dict(dbd=_FAKE["dbd"] + 8), ARG), ("dbd null with pos", dict(dbd=0), ARG), ("dsum_u null with pos", dict(dsum_u=0), ARG),
         ("dsum_v null with pos", dict(dsum_v=0), ARG),
         ("pad = 32", dict(pad=32), ARG), ("pad = 23", dict(pad=23), ARG), ("pad = -8 (band aligned)", dict(pad=-8), ARG), ("pad = 56 (band aligned, ldbd = 160 holds it)", dict(pad=56, ldbd=160), ARG),
         ("ldbd = 96 < pad + 2T - 1", dict(ldbd=96), ARG), ("ldbd = 112: no multiple of 32", dict(ldbd=112), ARG), ("ldbd = 2^30", dict(ldbd=BIG), ARG),
         ("T = 0 (pad = 0 keeps the band aligned)", dict(T=0, pad=0), ARG),
         ("qu_out without qv_out", dict(qv_out=0), ARG), ("qv_out without qu_out", dict(qu_out=0), ARG), ("qu_out without pos", dict(NO_POS), ARG),
         ("qu_out + 8 bytes", dict(qu_out=_FAKE["qu_out"] + 8), ARG), ("qv_out + 8 bytes", dict(qv_out=_FAKE["qv_out"] + 8), ARG),
         ("ldqb = 120 < H hd", dict(ldqb=120), ARG), ("ldqb = 132: no multiple of 8", dict(ldqb=132), ARG), ("flags = 2", dict(flags=2), ARG)]

MUTATIONS = {
    "mi_attention_qkv_bf16": _forward("mi_attention_qkv_bf16") + _general("mi_attention_qkv_bf16"),
    "mi_attention_qkv_bf16_v": _forward("mi_attention_qkv_bf16_v") + _general("mi_attention_qkv_bf16_v")
                               + [("variant = -1", dict(variant=-1), ARG), ("variant = 3", dict(variant=3), ARG)],
    "mi_attention_qkv_lse_bf16": _forward("mi_attention_qkv_lse_bf16") + _off8("mi_attention_qkv_lse_bf16", ("out",)) + _training(),
    "mi_attention_qkv_bwd_probs": [c for c in _forward("mi_attention_qkv_bwd_probs") if c[0] != "T = 0"] + _backward("mi_attention_qkv_bwd_probs") + _training() + _BAND,
    "mi_attention_x_lse_bf16": _forward("mi_attention_x_lse_bf16") + _off8("mi_attention_x_lse_bf16", ("out",)) + _training() + _x(),
    "mi_attention_x_bwd_probs": _forward("mi_attention_x_bwd_probs") + _backward("mi_attention_x_bwd_probs") + _training() + _x(),
}
# (entry, description, the full argument dict, recorded code)
CASES = [(e, what, dict(BASES[e], **over), code) for e, ms in MUTATIONS.items() for what, over, code in ms]
