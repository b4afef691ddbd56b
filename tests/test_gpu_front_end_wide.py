"""Throughput mode covers the front end: with `mi_ebf_config.wide_tiles` the conv sub-sampling's output Linear (K = F2 * C2 = 5120) and the feature projection run on
the 256 x 256 tile like the layers' N = d GEMMs; without it they keep the product's kernels.

The small config's front end (two layers behind it keep the run short) at B = 3: T = 1000 gives M = 750 rows = two full 256-row tiles and a partial one, with ragged
lengths so that padded frames meet the mask; T = 1024 gives T2 = 256, M = 768 = three full tiles.  A wide engine against an engine with the same forced `ln_fold` and
the product tiles: the tolerance is the one tests/test_gpu_encoder.py test_layernorm_fold_path_vs_reference applies between its "wide" and "fold" engines (the two tiles
differ by summation order only)."""
import ctypes as C

import pytest
import torch

import gemm_cases as G
from huggingface_asr_amd import shapes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDE_VS_FOLD_MAX, WIDE_VS_FOLD_MEAN = 0.02, 0.002          # tests/test_gpu_encoder.py: `dw.max() < 0.02 and dw.mean() < 0.002`


def _cfg(layers):
    return dict(shapes.SMALL, num_hidden_layers=layers, ctc_zero_infinity=True, ctc_loss_reduction="mean")


@pytest.fixture(scope="module")
def engines():
    """(wide, fold) on the same seeded weights"""
    from huggingface_asr_amd import synth
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg = _cfg(2)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 7).items()}
    out = []
    for wide in (True, False):
        eng = EBranchformerEngine(cfg, DEV)
        eng.ln_fold = True
        eng.wide_tiles = wide
        eng.load_state_dict(sd)
        out.append(eng)
    return out


@pytest.mark.parametrize("T,lens", [(1000, (1000, 777, 130)), (1024, (1024, 600, 257))], ids=["M750_partial_tile", "M768_whole_tiles"])
def test_wide_front_end_matches_the_product_tiles(engines, T, lens):
    from huggingface_asr_amd import synth
    wide, fold = engines
    feats = torch.from_numpy(synth.normal(21, "feats", (3, T, 80), 1.0)).to(DEV)
    fl = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for eng, w in ((wide, 1), (fold, 0)):
        cs = eng._config_struct(3, T, 80)
        assert cs.ln_fold == 1 and cs.wide_tiles == w
    a = wide.forward(feats, fl)
    la, ha = a["logits"].clone(), a["last_hidden"].clone()
    b = fold.forward(feats, fl)
    lb = b["logits"].clone()
    assert la.shape == lb.shape and la.shape[1] == T // 4
    assert bool(torch.isfinite(la.float()).all())
    dw = (la.float() - lb.float()).abs()
    print(f"wide vs fold: max {float(dw.max()):.5f} mean {float(dw.mean()):.6f}")
    assert float(dw.max()) < WIDE_VS_FOLD_MAX and float(dw.mean()) < WIDE_VS_FOLD_MEAN, (float(dw.max()), float(dw.mean()))
    again = wide.forward(feats, fl)
    assert torch.equal(again["logits"], la) and torch.equal(again["last_hidden"], ha)            # fixed summation order: the same bits run after run


def _family_flops(L):
    torch.cuda.synchronize()
    out = {}
    ms, fl, n = C.c_double(), C.c_double(), C.c_int()
    for fam in range(G.PF_COUNT):
        assert L.mi_profile_summary_family(fam, C.byref(ms), C.byref(fl), C.byref(n)) == 0
        out[fam] = (n.value, fl.value)
    return out


def test_which_tile_the_front_end_runs_on():
    """At a size where the product's dispatch gives an N = d GEMM to the 128 x 128 phase kernel (M = 36 * 250 = 9000 rows, N = 256: 142 tiles): without wide_tiles the
    front end's output Linear still runs there — it is 2 M d 5120 FLOP, more than every N = d GEMM of the one layer behind it together (K = 1024 + 256 + 512 + 512 + 1024),
    so that family's FLOP total cannot reach it otherwise — and with wide_tiles nothing does."""
    from huggingface_asr_amd import _lib, synth
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg = _cfg(1)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), 7).items()}
    Bz, T = 36, 1000
    feats = torch.from_numpy(synth.normal(22, "feats", (Bz, T, 80), 1.0)).to(DEV)
    L = _lib.lib()
    rc = L.mi_profile_create(64)
    assert rc in (0, _lib.ERR_ARG), rc
    fe_flops = 2.0 * Bz * (T // 4) * cfg["hidden_size"] * (20 * cfg["conv_dim"][1])
    try:
        got = {}
        for wide in (False, True):
            eng = EBranchformerEngine(cfg, DEV)
            eng.ln_fold = True
            eng.wide_tiles = wide
            eng.load_state_dict(sd)
            eng.forward(feats, None)                      # buffers, position table: outside the recorded run
            torch.cuda.synchronize()
            L.mi_profile_reset()
            L.mi_profile_enable(1)
            eng.forward(feats, None)
            got[wide] = _family_flops(L)
            L.mi_profile_enable(0)
        n128, f128 = got[False][G.PF_8P128]
        assert f128 >= fe_flops, (got[False], fe_flops)
        assert got[True][G.PF_8P128] == (0, 0.0), got[True]
        # the fp32-out 256 x 256 family now holds it beside the CTC head (the family's other members — feature projection, FFN-out, merge — are 0.35 of it together)
        head_flops = 2.0 * Bz * (T // 4) * (cfg["vocab_size"] + 1) * cfg["hidden_size"]
        assert got[True][G.PF_8P_OUT32][1] >= fe_flops + head_flops, got[True]
    finally:
        L.mi_profile_enable(0)
        L.mi_profile_reset()
