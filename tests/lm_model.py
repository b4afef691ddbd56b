"""GPT-2 language models for the shallow-fusion tests (reference src/decoding/shallow_fussion.py: `scores + lm_weight * log_softmax(lm_model(input_ids).logits[:, -1])`).

`tiny_lm()` is the LM of the fixture tests/golden/gen_tiny_lm.npz: transformers' `GPT2LMHeadModel` over the vocabulary of tests/gen_model.py with a STRUCTURED head, built
the way gen_model.py builds its decoder — orthogonal token directions in the embedding, a head that reads the last token's direction — but ranking the designated
successors differently from the decoder: where the decoder's best successor of a token is `successors(t)[0]`, this LM's is `successors(t)[1]` (unless the best one is the
end-of-sequence token, which it keeps), far enough ahead (GAMMA) that half its log-probability gap outweighs the decoder's.  So with `lm_weight = 0.5` greedy and beam search
leave the paths of `gen_tiny.npz`, which is what makes the fixture a test of the LM term.  Everything else keeps seeded random weights: the blocks, the positions and the KV
cache shape the values.  Only constants and huggingface_asr_amd.synth are used: the generator (which hands the module to the REFERENCE's generate()) and the tests (which
hand it to the HIP path and to the oracle) build the same numbers, and no weights are stored.

`random_lm(...)` is a seeded random GPT-2 of any size for the token-step tests."""
import torch

import gen_model as GM
from huggingface_asr_amd import synth

D, LAYERS, HEADS, NPOS = 128, 2, 2, 64
SEED = 23
GAMMA = 40.0
LM_WEIGHT = 0.5
# generation settings of the fixture: (num_beams, length_penalty, early_stopping, max_length, ctc_weight)
SETTINGS = [(1, 1.0, False, 14, 0.3), (3, 1.0, False, 14, 0.3), (5, 1.0, False, 14, 0.3), (5, 1.6, "never", 14, 0.3), (5, 1.0, True, 14, 0.3),
            (1, 1.0, False, 14, 0.0), (5, 1.0, False, 14, 0.0)]


def setting_key(W, lp, es, ml, cw):
    return f"W{W}_lp{lp}_es{es}_ml{ml}_ctc{cw}"


def _config(d, layers, heads, vocab, npos, tie):
    from transformers import GPT2Config
    return GPT2Config(vocab_size=vocab, n_embd=d, n_layer=layers, n_head=heads, n_positions=npos, activation_function="gelu_new", resid_pdrop=0.0, embd_pdrop=0.0,
                      attn_pdrop=0.0, tie_word_embeddings=tie, bos_token_id=GM.START, eos_token_id=GM.EOS)


def _seeded(model, seed):
    sd = {k: torch.from_numpy(synth.init_param(seed, "lm." + k, tuple(v.shape))) for k, v in model.named_parameters()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(("attn.bias" in m or "masked_bias" in m or m == "lm_head.weight") for m in missing), (missing, unexpected)
    return model


def random_lm(seed, d, layers, heads, vocab, npos=64, tie=True):
    from transformers import GPT2LMHeadModel
    return _seeded(GPT2LMHeadModel(_config(d, layers, heads, vocab, npos, tie)), seed).eval()


def lm_successors(t: int):
    s = GM.successors(t)
    if s[0] != GM.EOS:
        s[0], s[1] = s[1], s[0]
    return s


def overrides(seed: int = SEED) -> dict:
    fixed = torch.ones(1, D)
    rnd = torch.from_numpy(synth.normal(seed, "lm/emb", (GM.NACT + 1, D), 1.0))
    qm, _ = torch.linalg.qr(torch.cat([fixed, rnd], 0).double().t())
    dirs = (qm[:, 1:1 + GM.NACT + 1].t() * (D ** 0.5)).float()
    emb = torch.from_numpy(synth.normal(seed, "lm/emb_rest", (GM.V, D), 1.0))
    toks = list(range(GM.ACTIVE, GM.ACTIVE + GM.NACT)) + [GM.START]
    emb[toks] = dirs
    head = torch.zeros(GM.V, D)
    for t in toks:
        for k, v in enumerate(lm_successors(t)):
            head[v] += GAMMA * (1.0 if k == 0 else 0.5 - 0.1 * k) / D * emb[t]
    return {"transformer.wte.weight": emb, "lm_head.weight": head, "transformer.ln_f.weight": torch.ones(D), "transformer.ln_f.bias": torch.zeros(D)}


def tiny_lm(seed: int = SEED):
    """d 128, 2 layers, 2 heads (head size 64), V = gen_model.V, 64 positions, gelu_new, a separate (structured) head"""
    from transformers import GPT2LMHeadModel
    m = _seeded(GPT2LMHeadModel(_config(D, LAYERS, HEADS, GM.V, NPOS, False)), seed)
    missing, unexpected = m.load_state_dict(overrides(seed), strict=False)
    assert not unexpected
    return m.eval()


def lm_log_probs(lm, ids, q=None):
    """fp32 log_softmax of the LM's last-position logits for the prefixes `ids` (numpy (rows, len) int64) -> numpy (rows, V): LMRescorerLogitsProcessor's `lm_scores`.
    `q` (e.g. oracle.aed_ref.E.bf16_round) rounds the LM's matrices for the bf16 storage model."""
    if q is not None:
        import copy
        key = "_rounded_" + q.__name__
        if key not in lm.__dict__:
            r = copy.deepcopy(lm)
            with torch.no_grad():
                for n, p in r.named_parameters():
                    if p.dim() == 2 and "wpe" not in n and "wte" not in n:
                        p.copy_(q(p))
                if r.lm_head.weight.data_ptr() == r.transformer.wte.weight.data_ptr():
                    r.lm_head.weight = torch.nn.Parameter(q(r.transformer.wte.weight.detach().clone()))
            lm.__dict__[key] = r
        lm = lm.__dict__[key]
    with torch.no_grad():
        out = lm(torch.from_numpy(ids)).logits[:, -1].float()
    return torch.log_softmax(out, -1).numpy()


def with_lm(fn, lm, weight, q=None):
    """the reference's processor chain with the LM appended: fn(ids) + float32(weight) * log_softmax(LM(ids))[:, -1]"""
    import numpy as np

    def wrapped(ids):
        return (np.asarray(fn(ids), np.float32) + np.float32(weight) * lm_log_probs(lm, ids, q)).astype(np.float32)
    return wrapped
