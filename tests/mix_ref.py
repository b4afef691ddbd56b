"""CPU restatement of the DeCRED head mixing for the tests (reference src/models/decoders/multi_head_gpt2_mixing.py:101-131 and the `average_logits` branch of
multi_head_gpt2.py:129-136) on the oracle decoder of oracle/aed_ref.py, plus the structured model the decoding tests run.

`decoder_forward` has the signature of `oracle.aed_ref.decoder_forward`; `patched()` puts it in that place for the duration of a `with` block, so the oracle's joint score
function (oracle/generate_ref.py `joint_score_fn`, which `tests/test_gpu_generate.py::certified_decode` builds its reference trajectory from) scores with the mixed head.
Two arithmetic models, chosen by the storage hook `q` as everywhere in the oracle:
  q = identity   the reference's own arithmetic: H head products, mixed in fp32 (fp64 with `dtype=torch.float64`);
  q = bf16 round the HIP path's storage model: ONE product of the bf16-rounded row [hidden[loc_0] | ... | ln_f(x)] with the bf16-rounded folded matrix (+ fp32 bias).
The loss is the plain shifted cross-entropy of the mixed logits over every non-ignored position of the batch (the reference's formula, which the reference
itself only evaluates correctly at B = 1)."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

import gen_model as GM
from huggingface_asr_amd import synth
from huggingface_asr_amd.packing import head_fold, head_taps
from oracle import aed_ref as A

MODES = ("scalar", "linear", "full")


def _rounds(q) -> bool:
    return float(q(torch.tensor([1.00390625]))[0]) != 1.00390625          # 1 + 2^-8 is not a bf16 number


def mix_params(sd, pre, cfg):
    mode = cfg.get("mixing_mode")
    if mode in ("scalar", "linear"):
        return {"mix": sd[pre + "lm_mixing"]}
    if mode == "full":
        return {"mix_w": sd[pre + "lm_mixing.weight"], "mix_b": sd[pre + "lm_mixing.bias"]}
    return {}


def head_matrices(sd, pre, cfg):
    return [sd[f"{pre}additional_lm_heads.{k}.weight"] for k in range(len(cfg.get("head_locations") or []))] + [sd[pre + "lm_head.weight"]]


def mix_logits(per_head, cfg, mix):
    """the reference's expression for the logits from the H per-head logit tensors (..., V), in their dtype"""
    mode = cfg.get("mixing_mode")
    dt = per_head[0].dtype
    if mode == "full":
        return F.linear(torch.cat(per_head, -1), mix["mix_w"].to(dt), mix["mix_b"].to(dt))
    if mode in ("scalar", "linear"):
        return (torch.stack(per_head, -1) * mix["mix"].to(dt).t()).sum(-1)
    if mode is not None:
        raise NotImplementedError(mode)
    hw = list(cfg.get("head_weights") or [1.0])                              # average_logits with labels absent
    out = per_head[-1] * hw[-1]
    for lg, w in zip(per_head[:-1], hw[:-1]):
        out = out + w * lg
    return out


def mixed_from_hidden(hs, sd, pre, cfg, q=A._id, dtype=torch.float32):
    """logits of the mixed head from the hidden-state list of `oracle.aed_ref.decoder_hidden_states`"""
    heads, mix = head_matrices(sd, pre, cfg), mix_params(sd, pre, cfg)
    taps = head_taps(cfg)
    if _rounds(q):
        fold, bias = head_fold(cfg, [h.float() for h in heads], {k: v.float() for k, v in mix.items()})
        out = F.linear(q(torch.cat([hs[t].float() for t in taps], -1)), q(fold))
        return out + bias if bias is not None else out          # (`head_fold` is the code under test: this storage model is not an independent reference for the fold —
                                                                # `mix_logits` below is, and tests/test_mix_cpu.py ties the fold to it in fp64)
    return mix_logits([F.linear(hs[t].to(dtype), h.to(dtype)) for t, h in zip(taps, heads)], cfg, mix)


def plain_ce(logits, labels):
    """mean unsmoothed, shifted cross-entropy over the non-ignored positions of the whole batch"""
    lg, tg = logits[:, :-1].reshape(-1, logits.shape[-1]), labels[:, 1:].reshape(-1)
    return F.cross_entropy(lg, tg, ignore_index=-100)


def decoder_forward(sd, pre, cfg, ids, enc, enc_mask, labels=None, q=A._id, dm=None):
    """`oracle.aed_ref.decoder_forward` for a decoder whose configuration mixes heads (`mixing_mode`, or `average_logits` with labels absent); any other configuration goes
    to the oracle's own function"""
    mixing = cfg.get("mixing_mode") is not None
    if not mixing and not (labels is None and cfg.get("average_logits") and cfg.get("head_locations")):
        return _ORIGINAL(sd, pre, cfg, ids, enc, enc_mask, labels, q, dm)
    hs = A.decoder_hidden_states(sd, pre, cfg, ids, enc, enc_mask, q, dm)
    if labels is None:
        return None, mixed_from_hidden(hs, sd, pre, cfg, q)
    # the loss path mixes the per-head logits in fp32 also under the storage model (the engine does not use the folded bf16 matrix there)
    heads, mix = head_matrices(sd, pre, cfg), mix_params(sd, pre, cfg)
    logits = mix_logits([F.linear(q(hs[t]).to(LOSS_DTYPE), q(h).to(LOSS_DTYPE)) for t, h in zip(head_taps(cfg), heads)], cfg, mix)
    return plain_ce(logits, labels), logits


_ORIGINAL = A.decoder_forward
LOSS_DTYPE = torch.float32          # the head products, the mix and the cross-entropy of the loss path (the body of the oracle decoder stays fp32)


@contextlib.contextmanager
def patched(loss_dtype=torch.float32):
    global LOSS_DTYPE
    A.decoder_forward, LOSS_DTYPE = decoder_forward, loss_dtype
    try:
        yield
    finally:
        A.decoder_forward, LOSS_DTYPE = _ORIGINAL, torch.float32


# ---------------------------------------------------------------------------------------------------------------- the structured mixing model
SEED_MIX = 23
GAMMA2 = 13.0          # weaker than the main head's 22: with equal scales the two heads' favourites tie under a uniform mix; of 8 / 13 / 22 the value whose decodes close
                       # on the end-of-sequence token at several depths and differ from the plain decoder's in most rows


def successors2(t: int):
    """the additional head's successor table: other successors than tests/gen_model.py `successors`, end-of-sequence at other places"""
    s = [GM.ACTIVE + (5 * (t % GM.NACT) + 13 * k + 1) % GM.NACT for k in range(GM.NSUCC)]
    if t % 5 == 2:
        s[1] = GM.EOS
    return s


def overrides(seed: int, mode, fixed_pos: bool = False) -> dict:
    """state-dict entries on top of `gen_model.overrides`: the additional head (location 1 of `helpers.TINY_DEC`: the raw stream after one block, whose component along a
    token's embedding direction is ~ |emb|^2 = D) built like the main head from its own successor table, and seeded, non-uniform mixing parameters of `mode`
    (None: no mixing parameters — the `average_logits` case)."""
    ov = GM.overrides(seed, fixed_pos)
    emb = ov["decoder.transformer.wte.emb_layers.0.weight"] * (GM.D ** 0.5) if fixed_pos else ov["decoder.transformer.wte.weight"]
    u = torch.from_numpy(synth.uniform(seed, "mix/u", (GM.V,), 0.0, 1.0))
    head = torch.zeros(GM.V, GM.D)
    for t in list(range(GM.ACTIVE, GM.ACTIVE + GM.NACT)) + [GM.START]:
        for k, v in enumerate(successors2(t)):
            head[v] += GAMMA2 * (1.0 - GM.STEP * k * (1.0 + GM.SPREAD * float(u[t]))) / GM.D * emb[t]
    out = {"decoder.additional_lm_heads.0.weight": head}
    H, V = 2, GM.V
    if mode == "scalar":
        out["decoder.lm_mixing"] = torch.tensor([0.62, 0.47])
    elif mode == "linear":
        out["decoder.lm_mixing"] = 0.5 + torch.from_numpy(synth.uniform(SEED_MIX, "mix/linear", (H, V), -0.2, 0.2))
    elif mode == "full":
        out["decoder.lm_mixing.weight"] = torch.eye(V).repeat(1, H) * 0.5 + torch.from_numpy(synth.normal(SEED_MIX, "mix/full_w", (V, H * V), 0.01))
        out["decoder.lm_mixing.bias"] = torch.from_numpy(synth.normal(SEED_MIX, "mix/full_b", (V,), 0.1))
    return out


def mix_case_inputs(mode, average_logits=False):
    """(state dict, feats, attention mask, decoder configuration) of the `gen_tiny` model with the structured additional head and the mixing parameters of `mode`"""
    from helpers import gen_case_inputs
    _, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    seed, fixed, _ = GM.CASES["gen_tiny"]
    sd = dict(sd)
    sd.update(overrides(seed, mode, fixed))
    return sd, x, am, dict(dec_cfg, mixing_mode=mode, average_logits=average_logits)


def fold_case(H, locs, mode, seed=3, V=51, d=16, L=3, rows=7):
    """random heads / hidden states / mixing parameters (fp64) for the fold check: -> (cfg, heads, mix, hidden list indexed by location)"""
    g = torch.Generator().manual_seed(seed * 100 + H)
    rnd = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)
    cfg = dict(n_layer=L, head_locations=list(locs), head_weights=[0.3, 0.2, 0.5][:H] if H == 3 else [0.4, 0.6], mixing_mode=mode, average_logits=mode is None)
    heads = [rnd(V, d) * 0.3 for _ in range(H)]
    mix = {"scalar": {"mix": 0.5 + 0.2 * rnd(H)}, "linear": {"mix": 0.5 + 0.2 * rnd(H, V)},
           "full": {"mix_w": torch.eye(V, dtype=torch.float64).repeat(1, H) * 0.5 + 0.05 * rnd(V, H * V), "mix_b": 0.1 * rnd(V)}, None: {}}[mode]
    hidden = [rnd(rows, d) for _ in range(L + 1)]
    return cfg, heads, mix, hidden


def np_pad(a, L, pad):
    return np.pad(a, ((0, 0), (0, L - a.shape[1])), constant_values=pad)
