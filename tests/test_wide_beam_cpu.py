"""CPU: what wide-beam decoding decides on the host — which loop serves a request (`decoder.beam_loop_route`), whether the hypotheses share their utterance's cross K/V
(`decoder.cross_kv_layout`) — the new entries' declarations, the new kernels' scratch-free build, and that the cases of tests/test_gpu_wide_beam.py exercise what they
are there for (judged from the oracle's trace alone, before anything runs on a GPU)."""
import os
import re
import subprocess
import tempfile

import pytest
import torch

import wide_beam_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_beam_loop_route_table():
    from huggingface_asr_amd.decoder import beam_loop_route
    assert beam_loop_route(5, 5001, 64) == "device"                   # config 5
    assert beam_loop_route(10, 5001, 512) == "device"                 # the ebranchformer_english recipe: 10 * 1025 * 8 B of ids fit mi_beam_step's LDS
    assert beam_loop_route(60, 5001, 512) == "device_wide"            # the librispeech_aed recipe
    assert beam_loop_route(16, 5001, 1024) == "device_wide"           # 16 beams, but 16 * 2049 * 8 B > 96 KiB
    assert beam_loop_route(17, 51, 12) == "device_wide" and beam_loop_route(64, 5001, 512) == "device_wide"
    for V, ml in ((51, 12), (5001, 512)):
        assert beam_loop_route(65, V, ml) == "host"
    for W, V, ml in ((1, 51, 12), (5, 5001, 64), (60, 5001, 512), (65, 51, 12)):
        assert beam_loop_route(W, V, ml, True) == "host"              # the eos / space trick lives in the processor the host loop calls
    assert beam_loop_route(64, (1 << 24) // 64, 64) == "host" and beam_loop_route(64, (1 << 24) // 64 - 1, 64) == "device_wide"       # W * V >= 2^24
    assert beam_loop_route(4, 1 << 22, 64) == "host" and beam_loop_route(4, (1 << 22) - 1, 64) == "device"
    # the boundary of the LDS rule is mi_beam_step's own: W * (cur_len + Lmax) * 8 <= 96 KiB with cur_len < max_length, Lmax = max_length + 1
    assert beam_loop_route(16, 51, 383) == "device" and beam_loop_route(16, 51, 384) == "device_wide"


def test_new_entries_are_declared_bound_and_built():
    from huggingface_asr_amd import _lib
    S = _lib.SIGNATURES
    assert S["mi_beam_step_wide"] == S["mi_beam_step_lm"]
    assert len(S["mi_decoder_step_beams"]) == len(S["mi_decoder_step"]) + 1
    header = open(os.path.join(ROOT, "include", "hfasr_hip.h")).read()
    for name in ("mi_beam_step_wide", "mi_decoder_step_beams"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(_lib.lib(), name), name
    flat = lambda name: re.sub(r"\s+", " ", re.search(r"\bint " + name + r"\((.*?)\);", header, re.S).group(1))
    assert flat("mi_beam_step_wide") == flat("mi_beam_step_lm")       # the same arguments, word for word


def test_new_kernels_use_no_scratch():
    """the gfx950 code object of the built library: the kernels of csrc/beam_step_wide.hip have no private segment (no spills, no per-thread arrays in memory) and stay
    within the LDS their header states"""
    from huggingface_asr_amd import _lib
    _lib.lib()
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
            if b"beam_merge_kernel" not in blob[lo:hi]:
                continue
            with open(fb, "wb") as f:
                f.write(blob[lo:hi])
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
                            f"--output={co}"], check=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S*(?:beam_row_select_kernel|beam_merge_kernel)\S*)", block)
                if name:
                    num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                    found[name.group(1)] = (num("private_segment_fixed_size"), num("group_segment_fixed_size"), num("vgpr_count"))
    assert len(found) == 3, sorted(found)                              # row select with and without the LM term, the merge
    for name, (scratch, lds, vgprs) in found.items():
        assert scratch == 0, (name, scratch)
        assert lds <= (40 if "merge" in name else 34) * 1024 and vgprs <= 128, (name, lds, vgprs)


def test_cross_kv_layout_replicates_up_to_eight_rows_and_shares_beyond():
    from huggingface_asr_amd.decoder import cross_kv_layout
    for B, W in ((1, 5), (1, 8), (2, 4), (8, 1)):
        lay = cross_kv_layout(B, W, 250, 512, 8)
        assert lay["beams"] == 1 and lay["kv_rows"] == B * W * 250, (B, W, lay)          # config 5 keeps its kernels and its bits
    for B, W in ((1, 9), (2, 5), (16, 10), (16, 60), (2, 64)):
        lay = cross_kv_layout(B, W, 250, 512, 8)
        assert lay["beams"] == W and lay["kv_rows"] == B * 250, (B, W, lay)
    assert cross_kv_layout(16, 1, 250, 512, 8)["beams"] == 1           # greedy: one row per utterance either way
    # DeCRED_base size at the librispeech recipe's settings: 960 x 500 x 1024 x 2 B x 8 layers replicated, 16 x ... shared
    rep, sh = cross_kv_layout(16, 60, 500, 512, 8, share=False), cross_kv_layout(16, 60, 500, 512, 8)
    assert rep["bytes"] == 960 * 500 * 1024 * 2 * 8 == 7_864_320_000 and rep["beams"] == 1
    assert sh["bytes"] == 16 * 500 * 1024 * 2 * 8 == 131_072_000 and sh["beams"] == 60
    assert cross_kv_layout(1, 5, 250, 512, 8, share=True)["beams"] == 5


def test_wide_requests_on_cpu_tensors_still_raise():
    """no fallback: a 60-beam request on CPU inputs ends at the "inputs must be on the GPU" error, as every request does"""
    from test_surface_cpu import _joint_model
    from huggingface_asr_amd.decoding import GenerationConfigCustom
    m = _joint_model(False).eval()
    m.generation_config = GenerationConfigCustom(pad_token_id=50, eos_token_id=1, decoder_start_token_id=2, num_beams=60, max_length=140, ctc_weight=0.3)
    with pytest.raises(RuntimeError, match="GPU"):
        m.generate(input_values=torch.zeros(1, 200, 80))
    with pytest.raises(RuntimeError, match="GPU"):
        m.generate(input_values=torch.zeros(1, 200, 80), num_beams=20, max_length=12, ctc_weight=0)


SMALL_FOLLOW = [c for c in C.FOLLOW if c[2] <= 500]


def test_the_gpu_cases_exercise_what_they_are_there_for():
    """from the oracle's trace alone: every case closes hypotheses on the end-of-sequence token before max_length and runs at least three steps; the `ties` cases have
    equal values inside the top 2W, the `minus_inf` cases open utterances with fewer than 2W finite candidates; the long case re-orders beams and closes hypotheses while
    W * (cur_len + Lmax) * 8 is past 96 KiB.  (The V = 5001 cases of the plain sweep assert the same in the GPU test, where they are built anyway.)"""
    torch.set_num_threads(8)
    for c in SMALL_FOLLOW:
        r = C.build(*c)
        assert r["eos_closed"] > 0 and r["calls"] >= 3, (c, r["eos_closed"], r["calls"])
    for c in C.TIES:
        r = C.build(*c, 1.0, False, "ties")
        assert r["tied"] > 0 and r["eos_closed"] > 0 and r["calls"] >= 3, (c, r["tied"], r["eos_closed"], r["calls"])
    for c in C.MINUS_INF:
        r = C.build(*c, 1.0, False, "minus_inf")
        assert r["few"] > 0 and r["eos_closed"] > 0 and r["calls"] >= 3, (c, r["few"], r["eos_closed"], r["calls"])
    L = C.LONG
    r = C.build(L["B"], L["W"], L["V"], True, False, 1.0, False, "", L["max_length"], L["late"])
    past = [c for c in range(1, L["max_length"]) if L["W"] * (c + L["max_length"] + 1) * 8 > C.OLD_LDS]
    assert past[0] == 64 and r["calls"] > L["late"] and sum(r["reorder"][past[0]:]) > 20
    seq = r["oracle"][0]
    late_eos = [(row == C.EOS).any() and int((row == C.EOS).argmax()) >= L["late"] for row in seq]
    assert sum(late_eos) > 0
