"""CPU: the contract of the whole-encoder drivers (csrc/encoder.hip, csrc/encoder_f32.hip), written once in csrc/ebf_layout.hpp: the weight-table slot order against
engine.py's G / LS, and both workspace queries pinned to the bytes they returned before the drivers shared one geometry.  Nothing here launches a kernel."""
import ctypes as C
import os
import re

import pytest

from huggingface_asr_amd import shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "huggingface_asr_amd", "csrc")


def _strip_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _enum(src, name):
    """the enumerators of `enum <name> { ... }`, in order (none of them carries a value: the index is the position)"""
    body = re.search(r"\benum\s+" + name + r"\s*\{([^}]*)\}", src).group(1)
    names = [n.strip() for n in body.split(",") if n.strip()]
    assert all(re.fullmatch(r"\w+", n) for n in names), names
    return {n: i for i, n in enumerate(names)}


def test_slot_table_has_one_c_definition_and_engine_matches_it():
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.engine import G, LS
    layout = _strip_comments(open(os.path.join(CSRC, "ebf_layout.hpp")).read())
    c_g = {n[2:]: i for n, i in _enum(layout, "G").items() if n.startswith("G_")}
    c_ls = _enum(layout, "LS")
    assert len(c_g) == len(_enum(layout, "G"))            # every global enumerator is G_<engine name>
    assert c_g == G and c_ls == LS                        # same names, same indices, nothing on one side only
    header = open(os.path.join(ROOT, "include", "hfasr_hip.h")).read()
    n_g, n_ls = map(int, re.search(r"MI_EBF_GLOBAL_SLOTS\s*=\s*(\d+)\s*,\s*MI_EBF_LAYER_SLOTS\s*=\s*(\d+)", header).groups())
    assert (n_g, n_ls) == (_lib.GLOBAL_SLOTS, _lib.LAYER_SLOTS)
    assert max(c_g.values()) < n_g and max(c_ls.values()) < n_ls
    assert "static_assert" in layout and "MI_EBF_GLOBAL_SLOTS" in layout and "MI_EBF_LAYER_SLOTS" in layout
    for driver in ("encoder.hip", "encoder_f32.hip"):
        src = _strip_comments(open(os.path.join(CSRC, driver)).read())
        assert '#include "ebf_layout.hpp"' in src, driver
        assert not re.search(r"\benum\b", src), f"{driver} defines an enum of its own"


@pytest.fixture(scope="module")
def lib():
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.csrc import build as B
    B.build()
    return _lib.lib()


def _cs(cfg, batch, frames, precision="bf16", **fields):
    """the config struct engine.py hands the C call for `cfg` at (batch, frames, 80), with `fields` overwritten"""
    from huggingface_asr_amd.engine import EBranchformerEngine
    cs = EBranchformerEngine(dict(cfg), "cpu", precision=precision)._config_struct(batch, frames, 80)
    for k, v in fields.items():
        setattr(cs, k, v)
    return cs


TINY, SMALL, BASE = shapes.TINY, shapes.SMALL, shapes.BASE
GATED = dict(TINY, context_awareness_type="gated")
# name -> (config struct, bytes the library returned before this file existed)
BF16 = {
    "base_plain": (lambda: _cs(BASE, 32, 1000, ln_fold=0), 606468864),
    "base_fold": (lambda: _cs(BASE, 32, 1000, ln_fold=1), 607492864),
    "small": (lambda: _cs(SMALL, 2, 1000), 31754496),
    "tiny": (lambda: _cs(TINY, 2, 200), 913664),
    "tiny_gated_blk32": (lambda: _cs(dict(GATED, conv_dim=[32, 64]), 2, 200), 1553664),
    "tiny_gated_blk_c2": (lambda: _cs(dict(GATED, conv_dim=[32, 48]), 2, 200), 1361664),
    "tiny_gated_conv1_unfused": (lambda: _cs(dict(GATED, conv_dim=[30, 32]), 2, 200), 2097664),      # C1 % 4 != 0
    "tiny_gated_shared": (lambda: _cs(dict(TINY, context_awareness_type="gated_shared"), 2, 200), 1720064),
    "tiny_csgu_linear": (lambda: _cs(dict(TINY, csgu_use_linear_after_conv=True), 2, 200), 939264),
    "tiny_mixing": (lambda: _cs(dict(TINY, finetune_with_layer_mixing=True), 2, 200), 965120),
    "tiny_extra": (lambda: _cs(dict(TINY, finetune_with_additional_layer=True), 2, 200), 939264),
    "tiny_mixing_extra": (lambda: _cs(dict(TINY, finetune_with_layer_mixing=True, finetune_with_additional_layer=True), 2, 200), 965120),
    "tiny_causal": (lambda: _cs(dict(TINY, is_causal=True), 2, 200), 913664),
    "tiny_odd_T": (lambda: _cs(TINY, 3, 333), 2289408),
}
FP32 = {
    "tiny_relative": (lambda: _cs(TINY, 2, 200, "fp32"), 2061056),
    "tiny_rotary": (lambda: _cs(dict(TINY, position_embeddings_type="rotary"), 2, 200, "fp32"), 1849856),
    "tiny_csgu_linear": (lambda: _cs(dict(TINY, csgu_use_linear_after_conv=True), 2, 200, "fp32"), 2112256),
    "tiny_rotary_csgu_linear": (lambda: _cs(dict(TINY, position_embeddings_type="rotary", csgu_use_linear_after_conv=True), 2, 200, "fp32"), 1901056),
    "base_relative": (lambda: _cs(BASE, 32, 1000, "fp32"), 1263141120),
    "base_rotary": (lambda: _cs(dict(BASE, position_embeddings_type="rotary"), 32, 1000, "fp32"), 1228288256),
}


def test_the_cases_are_the_branches_they_name():
    cs = BF16["tiny_gated_blk32"][0]()
    assert (cs.context_mode, cs.gate_blk, cs.C2) == (1, 32, 64)
    cs = BF16["tiny_gated_blk_c2"][0]()
    assert (cs.context_mode, cs.gate_blk, cs.C2) == (1, 48, 48)
    cs = BF16["tiny_gated_conv1_unfused"][0]()
    assert cs.context_mode == 1 and cs.C1 % 4 != 0
    assert BF16["tiny_gated_shared"][0]().context_mode == 2 and BF16["tiny_csgu_linear"][0]().csgu_linear == 1
    assert BF16["small"][0]().ln_fold == 0 and BF16["tiny_causal"][0]().is_causal == 1
    cs = BF16["tiny_mixing_extra"][0]()
    assert cs.layer_mixing == 1 and cs.extra_layers == 1
    assert FP32["tiny_relative"][0]().pos_type == 1 and FP32["base_rotary"][0]().pos_type == 2


@pytest.mark.parametrize("name", list(BF16))
def test_bf16_workspace_bytes_are_what_they_were(lib, name):
    make, want = BF16[name]
    assert int(lib.mi_ebf_workspace_bytes(C.byref(make()))) == want


@pytest.mark.parametrize("name", list(FP32))
def test_fp32_workspace_bytes_are_what_they_were(lib, name):
    make, want = FP32[name]
    assert int(lib.mi_ebf_f32_workspace_bytes(C.byref(make()))) == want


def test_degenerate_configs_are_refused_not_divided_by(lib):
    """a null config, no heads, no batch or an input the convs reduce to nothing: both queries return 0 and the forward MI_ERR_ARG, before anything is launched
    (no pointer below is ever dereferenced)"""
    from huggingface_asr_amd import _lib
    for query in (lib.mi_ebf_workspace_bytes, lib.mi_ebf_f32_workspace_bytes):
        assert int(query(None)) == 0
        for fields in (dict(H=0), dict(H=-1), dict(B=0), dict(T=2, pad=0)):          # the last: T2 = 0
            assert int(query(C.byref(_cs(TINY, 2, 200, **fields)))) == 0, fields
    cs = _cs(TINY, 2, 200, H=0)
    assert lib.mi_ebf_forward(None, 8, 8, None, None, None, 0, 8, 1 << 40, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.mi_ebf_forward(C.byref(cs), 8, 8, None, None, None, 0, 8, 1 << 40, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.mi_ebf_forward_lse(C.byref(cs), 8, 8, None, None, None, 0, 8, 1 << 40, None, None, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.mi_ebf_forward_hs(C.byref(cs), 8, 8, None, None, None, 0, 8, 1 << 40, None, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.mi_ebf_forward_greedy(C.byref(cs), 8, 8, None, None, None, 0, 8, 1 << 40, None, 8, None, 8, None, None, None) == _lib.ERR_ARG
    assert lib.mi_ebf_forward_f32(None, 8, 8, None, None, None, 0, 8, 1 << 40, None, None, None, None, None) == _lib.ERR_ARG
    assert lib.mi_ebf_forward_f32(C.byref(cs), 8, 8, None, None, None, 0, 8, 1 << 40, None, None, None, None, None) == _lib.ERR_ARG

