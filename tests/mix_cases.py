"""Seeded token-step cases of the tiny GPT-2 decoder (d = 128, 3 layers, V = 51) for the multi-tap head tests: the decoder of `aed_tiny` with as many additional heads
as a case asks for, encoder frames from `synth`, ids from a fixed pattern — no encoder, so a case costs a few launches.  `step_case` drives two steps the way decoding
does (a prompt at past = 0, then one token on the cache); tests/golden/step_plain_bits.npz holds what `plain_bits` returned on the commit before the multi-tap head
existed (the plain decoder through mi_gpt2_step / mi_decoder_step_beams in every form), which the plain path must keep bit for bit."""
import numpy as np
import torch

from helpers import TINY_DEC, aed_case_inputs, load_golden
from huggingface_asr_amd import synth

T_ENC, SEED = 20, 5
# (rows, beams): both sides of the 8-row (fused / GEMV forms) and 64-row (streaming form) limits, and 2 utterances x 40 hypotheses on shared cross K/V
ROWS = [(1, 1), (8, 1), (9, 1), (64, 1), (65, 1), (80, 40)]


def decoder_sd(head_locations=(1,)):
    """`decoder.*` of the aed_tiny state dict with one additional head per location (head 0 is the fixture's, further ones are seeded here)"""
    sd, _, _, _ = aed_case_inputs(load_golden("aed_tiny"))
    sd = {k: v for k, v in sd.items() if k.startswith("decoder.")}
    V, d = TINY_DEC["vocab_size"], TINY_DEC["n_embd"]
    for k in range(len(head_locations)):
        name = f"decoder.additional_lm_heads.{k}.weight"
        if name not in sd:
            sd[name] = torch.from_numpy(synth.normal(SEED, name, (V, d), 0.08))
    for k in [k for k in sd if k.startswith("decoder.additional_lm_heads.") and int(k.split(".")[2]) >= len(head_locations)]:
        del sd[k]
    return sd


def step_inputs(M, beams, dev):
    """(prompt ids (M, U), next ids (M, 1), encoder frames bf16, key lengths) — beams > 1: one new token per row, frames of M / beams utterances"""
    U = 1 if beams > 1 else 3
    m, u = np.meshgrid(np.arange(M), np.arange(U + 1), indexing="ij")
    ids = torch.from_numpy(3 + (7 * m + 3 * u) % 40).to(dev)
    nkv = M // beams
    enc = torch.from_numpy(synth.normal(SEED, f"mix/enc{nkv}", (nkv * T_ENC, TINY_DEC["n_embd"]), 1.0)).to(dev).to(torch.bfloat16)
    lens = torch.tensor([T_ENC - (3 * b) % 7 for b in range(nkv)], dtype=torch.int32, device=dev)
    return ids[:, :U].contiguous(), ids[:, U:].contiguous(), enc, lens


def step_case(eng, M, beams, form=0, python=False):
    """[logits of the prompt step (past = 0), logits of the next token (past > 0)] of the decoder engine `eng`; `python`: through `step_py`"""
    dev = eng.device
    prompt, nxt, enc, lens = step_inputs(M, beams, dev)
    kvs = eng.cross_kv(enc)
    cache = eng.init_cache(M, 8)
    eng._gcfg.step_form = form
    out = []
    try:
        for ids in (prompt, nxt):
            if python:
                kv = [t.view(M // beams, 1, T_ENC, -1).expand(-1, beams, -1, -1).reshape(M * T_ENC, -1) for t in kvs] if beams > 1 else kvs
                out.append(eng.step_py(ids, cache, kv, T_ENC, lens.repeat_interleave(beams) if beams > 1 else lens).clone())
            else:
                out.append(eng.step(ids, cache, kvs, T_ENC, lens, beams=beams).clone())
    finally:
        eng._gcfg.step_form = 0
    return out


def plain_forms(M, beams):
    """the step forms a plain decoder can be asked for at this shape (mi_gpt2_config.step_form)"""
    return [0, 1, 2] if beams == 1 else [0]


def plain_bits(dev="cuda:0"):
    """name -> fp32 logits of the plain tiny decoder (head_locations [1], lm_head only at decode time) for every shape of ROWS in every form"""
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    eng = GPT2DecoderEngine(dict(TINY_DEC), dev)
    eng.load_state_dict(decoder_sd())
    out = {}
    for M, beams in ROWS:
        for form in plain_forms(M, beams):
            a, b = step_case(eng, M, beams, form)
            out[f"M{M}_W{beams}_f{form}/prompt"], out[f"M{M}_W{beams}_f{form}/next"] = a.cpu().numpy(), b.cpu().numpy()
    return out
