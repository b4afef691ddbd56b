"""CPU: what two-pass joint decoding (decoder.rescore / decoder.score, csrc/rescore.hip) decides away from the device — the float32 ranking against a float64 brute
force, its tie and -inf rules, the rule by which a hypothesis exists, every host-side refusal, the HFASR_JOINT_RESCORE routing of model.generate on a stub engine, the
new kernels' scratch-free build — and that the inputs of tests/test_gpu_rescore.py's end-to-end case are what that case needs (judged with the CPU oracle alone)."""
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import rescore_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS, PAD, START = 1, 50, 2


def random_case(seed, B, N, U, Tt=None, V=51):
    """an n-best with its nll: lengths 0..U (a quarter of the rows missing), tokens, frames, CTC scores, per-position nll in [0, 12)"""
    g = np.random.default_rng(seed)
    Tt = U if Tt is None else Tt
    ln = g.integers(1, U + 1, size=(B, N)).astype(np.int32)
    ln[g.random((B, N)) < 0.25] = 0
    ln = np.minimum(ln, Tt + 1)
    tokens = g.integers(3, V - 1, size=(B, N, Tt)).astype(np.int64)
    frames = np.sort(g.integers(0, 4 * Tt, size=(B, N, Tt)), axis=-1).astype(np.int32)
    ctc = (-g.random((B, N)) * 40).astype(np.float32)
    nll = (g.random((B, N, U)) * 12).astype(np.float32)
    return dict(ln=ln, tokens=tokens, frames=frames, ctc=ctc, nll=nll)


# ------------------------------------------------------------------------------------------------ select32 against select64
@pytest.mark.parametrize("lp", [0.0, 0.6, 1.0])
@pytest.mark.parametrize("w", [0.0, 0.3, 1.0])
def test_select32_orders_like_select64_beyond_the_float32_error_bound(lp, w):
    """float32 error of a total, derived: the ascending sum of l <= U terms is off by at most (l - 1) u S (S = the sum of the |nll|, u = 2^-24); the two weights and the
    denominator are float32 roundings of their float64 values (relative u each), the two products, the add and the divide round once each (relative u each): at most
    (l - 1) + 6 roundings of relative size u act on terms bounded by T = (w |ctc| + (1 - w) S) / denom.  E = (U + 8) u T covers it, second-order terms included.
    Wherever two float64 totals differ by more than E_i + E_j, float32 must order the pair the same way."""
    u = 2.0 ** -24
    checked = 0
    for seed, (B, N, U) in enumerate([(4, 64, 65), (6, 17, 130), (8, 5, 9)]):
        c = random_case(100 + seed, B, N, U)
        denom = RR.length_denoms(U, lp)
        s32 = RR.select32(c["nll"], c["ln"], c["ctc"], denom, np.float32(w), np.float32(1 - w), N, c["tokens"], c["frames"], EOS, PAD)
        t64, _ = RR.select64(c["nll"], c["ln"], c["ctc"], lp, w, N)
        S = np.array([[np.abs(c["nll"][b, n, :c["ln"][b, n]]).astype(np.float64).sum() for n in range(N)] for b in range(B)])
        with np.errstate(divide="ignore", invalid="ignore"):
            E = (U + 8) * u * (w * np.abs(c["ctc"].astype(np.float64)) + (1 - w) * S) / np.maximum(c["ln"], 1).astype(np.float64) ** lp
        for b in range(B):
            o = s32["order"][b]
            exists = c["ln"][b] > 0
            assert sorted(o.tolist()) == list(range(N))
            assert all(exists[o[k]] or not exists[o[k + 1]] for k in range(N - 1)), "a hypothesis that does not exist ranked in front of one that does"
            for k in range(N - 1):
                i, j = int(o[k]), int(o[k + 1])
                if exists[i] and exists[j]:
                    assert abs(float(s32["total"][b, k]) - t64[b, i]) <= E[b, i], (b, k)
                    if abs(t64[b, i] - t64[b, j]) > E[b, i] + E[b, j]:
                        assert t64[b, i] > t64[b, j], (b, k, t64[b, i], t64[b, j])
                        checked += 1
    assert checked > 100


def test_select32_tie_and_minus_inf_rules():
    B, N, U = 1, 8, 4
    c = random_case(7, B, N, U)
    c["ln"][0] = [3, 3, 0, 3, 2, 3, 0, 3]
    for n in (3, 5):                                        # rows 1, 3, 5: the same numbers -> the same total -> by lower n
        c["nll"][0, n], c["ctc"][0, n] = c["nll"][0, 1], c["ctc"][0, 1]
    c["ctc"][0, 7] = -np.inf                                # exists for the select (len > 0) but its total is -inf ...
    s = RR.select32(c["nll"], c["ln"], c["ctc"], RR.length_denoms(U, 1.0), np.float32(0.3), np.float32(0.7), N, c["tokens"], c["frames"], EOS, PAD)
    o = s["order"][0].tolist()
    assert [n for n in o if n in (1, 3, 5)] == [1, 3, 5] and o.index(3) == o.index(1) + 1 and o.index(5) == o.index(3) + 1
    assert o[-3:] == [2, 6, 7] and np.isneginf(s["total"][0, -3:]).all()          # ... and -inf rows go by lower n, the missing ones among them
    assert s["n_tokens"][0, -3:].tolist() == [0, 0, 2] and s["tokens"][0, -3, 0] == EOS and (s["tokens"][0, -3, 1:] == PAD).all() and (s["token_lp"][0, -3] == 0).all()
    z = RR.select32(c["nll"], c["ln"], c["ctc"], RR.length_denoms(U, 1.0), np.float32(0.0), np.float32(1.0), N, c["tokens"], c["frames"], EOS, PAD)
    assert z["order"][0, -1] == 7 and np.isneginf(z["total"][0, -1])              # 0 * -inf = NaN counts as -inf
    k1 = RR.select32(c["nll"], c["ln"], c["ctc"], RR.length_denoms(U, 1.0), np.float32(0.3), np.float32(0.7), 1, c["tokens"], c["frames"], EOS, PAD)
    assert k1["order"].shape == (1, 1) and k1["order"][0, 0] == o[0] and k1["total"][0, 0] == s["total"][0, 0]
    none = RR.select32(c["nll"], np.zeros((1, N), np.int32), c["ctc"], RR.length_denoms(U, 1.0), np.float32(0.3), np.float32(0.7), N, c["tokens"], None, EOS, PAD)
    assert none["order"][0].tolist() == list(range(N)) and np.isneginf(none["total"]).all() and "frames" not in none
    # the gathered rows: the tokens, the closing eos, then pad; -nll then 0; frames then -1
    k, n = 0, o[0]
    l = int(c["ln"][0, n])
    assert s["tokens"][0, k, :l - 1].tolist() == c["tokens"][0, n, :l - 1].tolist() and s["tokens"][0, k, l - 1] == EOS and (s["tokens"][0, k, l:] == PAD).all()
    assert np.array_equal(s["token_lp"][0, k, :l], -c["nll"][0, n, :l]) and (s["token_lp"][0, k, l:] == 0).all()
    assert s["frames"][0, k, :l - 1].tolist() == c["frames"][0, n, :l - 1].tolist() and (s["frames"][0, k, l - 1:] == -1).all()


# ------------------------------------------------------------------------------------------------ pack
def pack_edge_case(dtype=np.int64):
    """(tokens (2, 3, 7), n_tokens, ctc), V, U: the empty hypothesis, k = U - 1, k = U (too long), a token >= V, a non-finite score, a plain row"""
    V, U, Tt = 51, 5, 7
    tokens = np.full((2, 3, Tt), PAD, dtype=dtype)
    n = np.array([[0, 4, 5], [3, 2, 2]], dtype=np.int32)
    ctc = np.array([[-1.5, -2.5, -3.5], [-4.5, -np.inf, -6.5]], dtype=np.float32)
    tokens[0, 1, :4] = [7, 8, 9, 10]
    tokens[0, 2, :5] = [11, 12, 13, 14, 15]
    tokens[1, 0, :3] = [16, V, 17]
    tokens[1, 1, :2] = [18, 19]
    tokens[1, 2, :2] = [20, 0]
    return tokens, n, ctc, V, U


def test_pack_edge_cases():
    tokens, n, ctc, V, U = pack_edge_case()
    ids, labels, ln = RR.pack(tokens, n, ctc, V, U, START, EOS, PAD)
    assert ln.tolist() == [1, 5, 0, 0, 0, 3]
    assert ids[0].tolist() == [START, PAD, PAD, PAD, PAD] and labels[0].tolist() == [EOS, -100, -100, -100, -100]              # the empty hypothesis exists
    assert ids[1].tolist() == [START, 7, 8, 9, 10] and labels[1].tolist() == [7, 8, 9, 10, EOS]                                 # k = U - 1 fits exactly
    for r in (2, 3, 4):                                                                                                          # k = U; a token >= V; a score of -inf
        assert ids[r].tolist() == [START, PAD, PAD, PAD, PAD] and (labels[r] == -100).all()
    assert ids[5].tolist() == [START, 20, 0, PAD, PAD] and labels[5].tolist() == [20, 0, EOS, -100, -100]
    for bad in (np.nan, np.inf):
        c2 = ctc.copy()
        c2[0, 0] = bad
        assert RR.pack(tokens, n, c2, V, U, START, EOS, PAD)[2][0] == 0
    t2 = tokens.copy()
    t2[1, 2, 1] = -1                                                                                                             # a negative token
    assert RR.pack(t2, n, ctc, V, U, START, EOS, PAD)[2][5] == 0
    i1, l1, n1 = RR.pack(np.full((1, 1, 1), PAD), np.zeros((1, 1), np.int32), np.zeros((1, 1), np.float32), V, 1, START, EOS, PAD)
    assert i1.tolist() == [[START]] and l1.tolist() == [[EOS]] and n1.tolist() == [1]


# ------------------------------------------------------------------------------------------------ refusals
class _OnDevice(torch.Tensor):
    """stands in for a device tensor on a machine without one: `generate` only asks for `.is_cuda` before it hands the request to the (stubbed) engine functions"""
    @property
    def is_cuda(self):
        return True


def _stub_joint(V=51):
    return types.SimpleNamespace(dec=types.SimpleNamespace(w=dict(lm_head=torch.zeros(V, 4))), enc=types.SimpleNamespace(cfg=dict(vocab_size=V - 1)),
                                 jcfg=dict(pad_token_id=PAD, decoder_start_token_id=START), device=torch.device("cpu"))


def test_every_host_side_refusal():
    from huggingface_asr_amd import decoder as D
    joint, x = _stub_joint(), torch.zeros(1, 40, 80)
    ok = dict(num_beams=5, eos_token_id=EOS)
    for bad in (dict(nbest=0), dict(nbest=6), dict(num_beams=0), dict(num_beams=65), dict(ctc_weight=-0.1), dict(ctc_weight=1.5), dict(ctc_weight=float("nan")),
                dict(max_length=1), dict(num_return=6), dict(nbest=3, num_return=4), dict(num_return=0)):
        with pytest.raises(ValueError):
            D.rescore(joint, x, None, **dict(ok, **bad))
    with pytest.raises(RuntimeError, match="GPU"):
        D.rescore(joint, x, None, **ok)                                         # CPU tensors: no fallback
    other = _stub_joint()
    other.enc.cfg["vocab_size"] = 48                                            # a CTC head of 49 classes beside a decoder of 51
    with pytest.raises(ValueError, match="one vocabulary"):
        D._check_rescore_args(other, torch.Tensor._make_subclass(_OnDevice, x), num_beams=5, nbest=None, ctc_weight=0.3, max_length=14, num_return=None, who="rescore")
    hyps = torch.zeros(1, 3, 4, dtype=torch.long)
    for bad in (dict(ctc_weight=2.0), dict(max_length=1)):
        with pytest.raises(ValueError):
            D.score(joint, x, None, hyps, eos_token_id=EOS, **bad)
    for bad_h in (hyps.int(), hyps[0], torch.zeros(2, 3, 4, dtype=torch.long), torch.zeros(1, 65, 4, dtype=torch.long)):
        with pytest.raises(ValueError):
            D.score(joint, x, None, bad_h, eos_token_id=EOS)
    with pytest.raises(RuntimeError, match="GPU"):
        D.score(joint, x, None, hyps, eos_token_id=EOS)
    from test_surface_cpu import _joint_model
    m = _joint_model(False).eval()
    with pytest.raises(RuntimeError, match="GPU"):
        m.rescore(input_values=x, num_beams=5, max_length=14)
    with pytest.raises(RuntimeError, match="GPU"):
        m.score(input_values=x, sequences=torch.tensor([[START, 5, EOS]]), max_length=14)
    from huggingface_asr_amd import ops
    with pytest.raises(RuntimeError):
        ops.rescore_pack(torch.zeros(1, 1, 1, dtype=torch.long), torch.zeros(1, 1, dtype=torch.int32), torch.zeros(1, 1), vocab=51, U=1, start_id=START, eos_id=EOS, pad_id=PAD)
    with pytest.raises(RuntimeError):
        ops.rows_nll(torch.zeros(2, 5), torch.zeros(2), torch.zeros(2, dtype=torch.long))


def test_denominators_are_generates():
    """denom[l] is `_step_denoms`' closing denominator of the step that closes a hypothesis of l generated tokens (cur_len = l prefix tokens incl. the start token)"""
    from huggingface_asr_amd import decoder as D
    for lp in (0.0, 0.6, 1.0, 1.6):
        tab = D._length_denoms(40, lp)
        assert np.array_equal(np.array(tab, dtype=np.float32), RR.length_denoms(40, lp))
        for l in range(1, 41):
            assert tab[l] == D._step_denoms(l, 64, lp, False)[0]


# ------------------------------------------------------------------------------------------------ routing of model.generate
def _routed(monkeypatch, env, **kw):
    from test_surface_cpu import _joint_model
    from huggingface_asr_amd import modeling_joint as MJ
    from huggingface_asr_amd.decoding import GenerationConfigCustom
    m = _joint_model(False).eval()
    m.generation_config = GenerationConfigCustom(pad_token_id=PAD, eos_token_id=EOS, decoder_start_token_id=START, num_beams=kw.pop("num_beams", 5), max_length=14, ctc_weight=0.3,
                                                 space_token_id=-1, apply_eos_space_trick=bool(kw.pop("trick", False)), eos_space_trick_weight=1.0)
    calls = []
    hyp = [dict(tokens=[START, 7, EOS], score=-1.0, hypotheses=[(-1.0 - k, [START, 7 + k, EOS]) for k in range(5)])]

    def fake(name):
        def f(eng, inputs, fl, **k):
            calls.append((name, k))
            return hyp
        return f
    monkeypatch.setattr(MJ, "_generate", fake("generate"))
    monkeypatch.setattr(MJ, "_rescore", fake("rescore"))
    monkeypatch.setattr(m, "_get_engine", lambda device: object())
    if env is None:
        monkeypatch.delenv("HFASR_JOINT_RESCORE", raising=False)
    else:
        monkeypatch.setenv("HFASR_JOINT_RESCORE", env)
    x = torch.Tensor._make_subclass(_OnDevice, torch.zeros(1, 40, 80))
    out = m.generate(input_values=x, **kw)
    return calls, out


def test_generate_routing_by_the_environment_variable(monkeypatch):
    calls, out = _routed(monkeypatch, None)
    assert [c[0] for c in calls] == ["generate"] and out.tolist() == [[START, 7, EOS]]          # unset -> _generate is called
    calls, _ = _routed(monkeypatch, "0")
    assert [c[0] for c in calls] == ["generate"]
    calls, out = _routed(monkeypatch, "1", num_return_sequences=2)
    assert [c[0] for c in calls] == ["rescore"] and out.tolist() == [[START, 7, EOS], [START, 8, EOS]]
    k = calls[0][1]
    assert k["num_beams"] == 5 and k["num_return"] == 2 and k["ctc_weight"] == 0.3 and k["max_length"] == 14 and k["length_penalty"] == 1.0
    assert (k["eos_token_id"], k["pad_token_id"], k["start_token_id"]) == (EOS, PAD, START)
    for es in (True, "never"):                                                                   # early_stopping is anything
        calls, _ = _routed(monkeypatch, "1", early_stopping=es)
        assert [c[0] for c in calls] == ["rescore"]
    calls, _ = _routed(monkeypatch, "1", num_beams=1)                                            # greedy keeps today's route ...
    assert [c[0] for c in calls] == ["generate"]
    calls, _ = _routed(monkeypatch, "1", trick=True)                                             # ... and so does the eos / space trick
    assert [c[0] for c in calls] == ["generate"] and calls[0][1]["apply_eos_space_trick"] is True


# ------------------------------------------------------------------------------------------------ the build
def test_rescore_entries_are_declared_bound_and_built_without_scratch():
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.csrc import build as B
    assert "rescore.hip" in B.SOURCES
    header = open(os.path.join(ROOT, "include", "hfasr_hip.h")).read()
    for name in ("mi_rescore_pack", "mi_rows_nll_f32", "mi_rescore_select"):
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    so = os.path.join(ROOT, "huggingface_asr_amd", "libhfasr_hip.so")
    llvm = "/opt/rocm/lib/llvm/bin"
    found = {}
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "lib.fatbin"), os.path.join(td, "lib.co")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fb], check=True)
        blob = open(fb, "rb").read()                                   # one bundle per translation unit, back to back
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        for lo, hi in zip(starts, starts[1:] + [len(blob)]):
            if b"rescore_select_kernel" not in blob[lo:hi]:
                continue
            with open(fb, "wb") as f:
                f.write(blob[lo:hi])
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
                            f"--output={co}"], check=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S*(?:rescore_pack_kernel|rows_nll_kernel|rescore_select_kernel)\S*)", block)
                if name:
                    num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                    found[name.group(1)] = (num("private_segment_fixed_size"), num("group_segment_fixed_size"), num("vgpr_count"))
    assert len(found) == 5, sorted(found)                              # pack and select for int32 / int64 tokens, the nll gather
    for name, (scratch, lds, vgprs) in found.items():
        assert scratch == 0 and lds <= 1024 and vgprs <= 64, (name, scratch, lds, vgprs)


# ------------------------------------------------------------------------------------------------ the end-to-end case of tests/test_gpu_rescore.py
def test_the_end_to_end_inputs_are_what_the_gpu_case_needs():
    """with the CPU oracle alone: every utterance of the end-to-end case has at least three existing hypotheses of two or more tokens, and at most one utterance has a
    gap between ranks 1 and 2 under the 5e-3 the GPU test needs to hold the top-1 to the oracle's"""
    import rescore_cases as RC
    torch.set_num_threads(8)
    c = RC.end_to_end_case()
    assert len(c["oracle"]) == c["x"].shape[0] == 2
    for rows in c["oracle"]:
        assert sum(len(h["labels"]) >= 2 for h in rows) >= 3, [len(h["labels"]) for h in rows]
        assert all(a["total"] >= b["total"] for a, b in zip(rows, rows[1:]))
        assert all(h["ctc"] <= h["ctc_exact"] + 1e-9 for h in rows)                # the beam search's score is the mass it kept: at most the exact probability
    gaps = [rows[0]["total"] - rows[1]["total"] for rows in c["oracle"]]
    assert sum(g <= RC.TOP1_GAP for g in gaps) <= 1, gaps
    short = RC.end_to_end_case(max_length=RC.SHORT_MAX_LENGTH)                     # the same n-best under a max_length that drops its longest hypotheses
    assert any(len(s) < len(f) for s, f in zip(short["oracle"], c["oracle"])) and all(len(s) >= 1 for s in short["oracle"])
