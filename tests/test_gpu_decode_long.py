"""GPU parity of the token step at the lengths the reference's evaluation recipes decode with (`num_beams=10`, `max_length` up to 512): the DeCRED_base-size decoder of
tests/config5_model.py (8 x 512, 8 heads, V = 5001, fixed positions, n_positions = 256) over 300 token steps, so that the KV cache passes 256 keys and the positions pass
the configured table, against the oracle's teacher-forced decoder (oracle/aed_ref.py) with the kernels' bf16 storage model.  The encoder is not run: bf16-rounded random
"encoder states" of 500 frames (past 256 cross-attention keys) feed both sides, for one utterance and for two ragged ones (500 and 180 valid frames, the lengths repeated
per beam as generate() does).

Code paths (csrc/decoder_step.hip mi_gpt2_step):
  * fused   (B * W <= 8 rows, one new token per row): csrc/decoder_fused.hip, `attn_rows` loading keys in batches of 256, `fused_cross_kernel` with per-row enc_len;
  * skinny  (the same rows, mi_gpt2_config.step_form = 1): GEMV-style linears and `decode_attn_kernel`, striding over keys the same way;
  * general (B * W > 8 rows): mi_gemm_bf16 and mi_attention_qkv_bf16 with one query row against past + 1 cached keys (causal offset Tk - T)."""
import functools

import numpy as np
import pytest
import torch

import config5_model as M
from oracle import aed_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS, LMAX = 300, 301
REORDERS = (150, 270)                              # the caches are re-ordered before these steps
CHECKS = (0, 1, 254, 255, 256, 257, 299)
FUSED_MAXM = 8                                      # FD_MAXM / SK_MAXM: the fused and skinny forms take at most 8 rows
ENC_SIDES = {"one_500": (500,), "ragged_500_180": (500, 180)}


@functools.lru_cache(maxsize=1)
def _model():
    sd = M.state_dict(0, structured=False)
    return {k: v for k, v in sd.items() if k.startswith("decoder.")}


@functools.lru_cache(maxsize=2)
def _encoder_states(side):
    lens = ENC_SIDES[side]
    B, T2 = len(lens), max(lens)
    g = torch.Generator().manual_seed(500 + B)
    return A.E.bf16_round(torch.randn(B, T2, M.D, generator=g)), torch.tensor(lens, dtype=torch.int32)


def _token(u, r):
    """the token row r feeds at step u (W different prefixes; step 0 feeds the start token)"""
    return 2 if u == 0 else 7 + (u * (37 + 11 * r) + 101 * r) % 4990


def _selection(k, B, W):
    """beam_idx of the k-th re-ordering: within every utterance's W rows, as beam search selects (a rotation, then one that repeats a row)"""
    rows = []
    for b in range(B):
        sel = [(r + 1) % W for r in range(W)] if k == 0 else [0] + [r - 1 for r in range(1, W)]
        if k == 1 and W > 2:
            sel[2] = 0
        rows += [b * W + s for s in sel]
    return torch.tensor(rows)


def _run_engine(side, W, step_form):
    """300 token steps through GPT2DecoderEngine.step -> (logits at CHECKS (rows, len(CHECKS), V), the rows' token histories at CHECKS)"""
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    enc, lens = _encoder_states(side)
    B, T2 = enc.shape[:2]
    n = B * W
    eng = GPT2DecoderEngine(M.DEC_CFG, DEV)
    eng.load_state_dict(_model(), "decoder.")
    eng._gcfg.step_form = step_form
    kvs = eng.cross_kv(enc.repeat_interleave(W, 0).reshape(n * T2, M.D).to(DEV, torch.bfloat16))
    key_rep = lens.repeat_interleave(W).to(DEV)
    assert eng.w["pos"].shape[0] == M.DEC_CFG["n_positions"] == 256
    cache = eng.init_cache(n, LMAX)
    assert eng.w["pos"].shape[0] >= LMAX                   # the fixed table grew to the cache (position 299 > n_positions)
    hist = torch.zeros(n, 0, dtype=torch.long)
    got, hists = [], []
    for u in range(STEPS):
        if u in REORDERS:
            sel = _selection(REORDERS.index(u), B, W)
            if W > 1:
                assert (sel != torch.arange(n)).any()      # rows move
            past = cache["past"]
            before = [[t.index_select(0, sel.to(DEV))[:, :past].clone() for t in cache[kv]] for kv in ("k", "v")]
            eng.reorder_cache(cache, sel)
            for kv, want in zip(("k", "v"), before):
                for l in range(len(want)):
                    assert torch.equal(cache[kv][l][:, :past], want[l]), (u, kv, l)        # every cached row, beyond key 256 at the second re-ordering
            hist = hist.index_select(0, sel)
        tok = torch.tensor([[_token(u, r)] for r in range(n)])
        hist = torch.cat([hist, tok], 1)
        logits = eng.step(tok.to(DEV), cache, kvs, T2, key_rep)
        if u in CHECKS:
            got.append(logits.float().cpu())
            hists.append(hist.clone())
    assert cache["past"] == STEPS
    return torch.stack(got, 1), hists


def _oracle(side, W, hists):
    """the oracle's teacher-forced logits of every row's history at CHECKS: one decoder pass per span between re-orderings (a row's history within a span is a prefix of
    its history at the span's last check)"""
    enc, lens = _encoder_states(side)
    B, T2 = enc.shape[:2]
    enc_rep = enc.repeat_interleave(W, 0)
    mask = (torch.arange(T2)[None] < lens[:, None].long()).repeat_interleave(W, 0)
    span = lambda u: sum(u >= r for r in REORDERS)
    out = [None] * len(CHECKS)
    for s in sorted({span(u) for u in CHECKS}):
        idx = [i for i, u in enumerate(CHECKS) if span(u) == s]
        last = hists[idx[-1]]
        for i in idx:
            assert torch.equal(hists[i], last[:, : CHECKS[i] + 1])
        with torch.no_grad():
            _, logits = A.decoder_forward(_model(), "decoder.", M.DEC_CFG, last, enc_rep, mask, None, A.E.bf16_round)
        for i in idx:
            out[i] = logits[:, CHECKS[i]].float()
    return torch.stack(out, 1)


def _compare(got, want, rows):
    std = float(want.std())
    err = (got - want).abs()
    assert float(err.max()) < 0.06 * max(std, 1.0) + 0.03 and float(err.mean()) < 0.01 * max(std, 1.0), (float(err.max()), float(err.mean()), std)
    top2 = want.topk(2, -1).values
    clear = (top2[..., 0] - top2[..., 1]) > 0.1
    assert bool((got.argmax(-1)[clear] == want.argmax(-1)[clear]).all()) and int(clear.sum()) >= rows, int(clear.sum())
    return float(err.max())


@pytest.mark.parametrize("side,W", [("one_500", 1), ("one_500", 5), ("one_500", 8), ("ragged_500_180", 1), ("ragged_500_180", 4)])
def test_fused_and_skinny_token_steps_over_300_positions(side, W):
    """Fused and skinny forms (B * W <= 8 rows) over 300 steps: the self-attention's second 256-key batch from step 256 on, the cross-attention's second batch over
    500 frames (and the ragged utterance's 180), positions past n_positions = 256 — against the oracle at steps 0, 1, 254-257 and 299, with two re-orderings."""
    torch.set_num_threads(8)
    B = len(ENC_SIDES[side])
    assert B * W <= FUSED_MAXM
    want = None
    for form in (0, 1):                                    # 0: fused (csrc/decoder_fused.hip), 1: skinny
        got, hists = _run_engine(side, W, form)
        if want is None:
            want = _oracle(side, W, hists)
        worst = _compare(got, want, B * W)
        print(f"{side} W = {W} form {form}: max |dlogit| {worst:.3f}")


@pytest.mark.parametrize("side,W", [("one_500", 10), ("ragged_500_180", 5), ("ragged_500_180", 10)])
def test_general_token_step_over_300_positions(side, W):
    """The general path (B * W > 8 rows: the recipes' 10 beams): MFMA GEMMs and mi_attention_qkv_bf16 with one query row against past + 1 cached keys, over 300 steps
    (past 256 keys and n_positions) and 500 encoder frames, against the oracle at steps 0, 1, 254-257 and 299, with two re-orderings."""
    torch.set_num_threads(8)
    B = len(ENC_SIDES[side])
    assert B * W > FUSED_MAXM
    got, hists = _run_engine(side, W, 0)
    worst = _compare(got, _oracle(side, W, hists), B * W)
    print(f"{side} W = {W} general path: max |dlogit| {worst:.3f}")


def test_learned_positions_are_refused_past_the_table_on_the_device_engine():
    """A learned wpe with n_positions = 16: the step that would read row 16 raises on the host, before any launch (the cache stays as it was)."""
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    cfg = dict(M.DEC_CFG, pos_emb_fixed=False, n_positions=16)
    sd = dict(_model())
    sd["decoder.transformer.wte.weight"] = sd.pop("decoder.transformer.wte.emb_layers.0.weight")
    sd["decoder.transformer.wpe.weight"] = torch.randn(16, M.D, generator=torch.Generator().manual_seed(16)) * 0.02
    eng = GPT2DecoderEngine(cfg, DEV)
    eng.load_state_dict(sd, "decoder.")
    enc, lens = _encoder_states("one_500")
    kvs = eng.cross_kv(enc.reshape(-1, M.D).to(DEV, torch.bfloat16))
    cache = eng.init_cache(1, 24)
    for u in range(16):
        assert torch.isfinite(eng.step(torch.tensor([[_token(u, 0)]], device=DEV), cache, kvs, enc.shape[1], lens.to(DEV))).all()
    torch.cuda.synchronize()
    k0 = cache["k"][0].clone()
    with pytest.raises(ValueError, match="n_positions"):
        eng.step(torch.tensor([[5]], device=DEV), cache, kvs, enc.shape[1], lens.to(DEV))
    torch.cuda.synchronize()
    assert cache["past"] == 16 and torch.equal(cache["k"][0], k0)
