"""CPU: the decoder's position table against the length of a decode.  The token step reads row `past + u` of the table without a bound (csrc/decoder_step.hip
mi_embed_tokens, csrc/decoder_fused.hip's embedding row), so the host must make the rows exist before any launch: fixed sinusoidal positions are defined for every
position in the reference (src/models/embeddings.py:65-90) and the table grows to the cache; a learned wpe has n_positions rows and a longer decode is refused."""
import types

import pytest
import torch

from helpers import TINY_DEC
from oracle import aed_ref as A


def _decoder(fixed):
    from test_surface_cpu import _joint_model
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    sd = _joint_model(fixed).state_dict()
    cfg = dict(TINY_DEC, pos_emb_fixed=fixed)
    eng = GPT2DecoderEngine(cfg, "cpu")
    eng.load_state_dict(sd, "decoder.")
    return eng, sd, cfg


def test_fixed_positions_grow_to_the_cache():
    eng, sd, cfg = _decoder(True)
    n = cfg["n_positions"]
    assert eng.w["pos"].shape[0] == n
    before = eng.w["pos"].clone()
    cache = eng.init_cache(2, 3 * n + 5)
    pos = eng.w["pos"]
    assert pos.shape[0] >= cache["Lmax"] and eng._wtable[1] == pos.data_ptr()           # the C step's pointer table follows the new tensor
    assert torch.equal(pos[:n], before)                                                  # the rows that existed are unchanged, bit for bit
    ids = torch.zeros(1, cache["Lmax"], dtype=torch.long)
    d = cfg["n_embd"]
    want = A.embed(sd, "decoder.", cfg, ids)[0] - sd["decoder.transformer.wte.emb_layers.0.weight"][0] * d ** 0.5     # the oracle's sinusoid at every position
    torch.testing.assert_close(pos[: cache["Lmax"]], want, atol=2e-5, rtol=0)
    eng.ensure_positions(10)                                                             # a shorter request keeps the table
    assert eng.w["pos"] is pos


def test_learned_positions_refuse_a_decode_past_the_table():
    from huggingface_asr_amd.decoder import generate, generate_stepwise
    eng, sd, cfg = _decoder(False)
    n = cfg["n_positions"]
    cache = eng.init_cache(1, n + 8)                                                     # a cache longer than the table is fine ...
    assert eng.w["pos"].shape[0] == n
    cache["past"] = n - 1
    for U in (2, 3):                                                                     # ... a step that would read row n is not
        with pytest.raises(ValueError, match="n_positions"):
            eng.step(torch.zeros(1, U, dtype=torch.long), cache, None, 0, None)
        with pytest.raises(ValueError, match="n_positions"):
            eng.step_py(torch.zeros(1, U, dtype=torch.long), cache, None, 0, None)
    assert cache["past"] == n - 1
    eng.ensure_positions(n)
    joint = types.SimpleNamespace(dec=eng)                                               # refused up front, before the encoder runs
    for fn in (generate, generate_stepwise):
        with pytest.raises(ValueError, match="n_positions"):
            fn(joint, torch.zeros(1, 100, 80), None, num_beams=3, max_length=n + 2)
