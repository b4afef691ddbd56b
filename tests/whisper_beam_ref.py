"""A plain-torch restatement of transformers' `GenerationMixin._beam_search` for one call with a prompt of P tokens, shared by tests/test_whisper_beam_cpu.py (where it is
held to transformers' own loop) and tests/test_gpu_whisper_beam.py (where it is the reference of `whisper.beam_decode`).

Per step: logits (B W, V) from `step_fn`; candidate values = `logprob_fn(logits)` with the `processors` (transformers' own SuppressTokens* / WhisperTimeStampLogitsProcessor
objects, or callables of the same signature) applied in order, + the running beam score (fp32).  The top 2W of an utterance's W V candidates are ordered by value, then by
lower index — a stable sort, not `topk`, whose order among equal values is not defined.  The closing, early-stop and done rules are those of
`huggingface_asr_amd.decoder.generate_stepwise` with the prompt length in place of 1: a candidate stops at EOS or at max_length; the first W that did not stop run on (at
max_length the stopped ones, lowered by 1e9); stopped candidates among the first W ranks join the kept hypotheses with score / (generated tokens) ** length_penalty, an
equal score behind the older one; an utterance is done when the best running beam cannot beat the worst of W kept hypotheses, or — early_stopping True — as soon as W are
kept, or at max_length.  A done utterance is frozen (its rows keep stepping, as in transformers, and are not read)."""
import numpy as np
import torch

NEG = np.float32(-1.0e9)


def beam_search_ref(step_fn, logprob_fn, processors, prompt, *, num_beams, max_length, eos_token_id, pad_token_id, length_penalty=1.0, early_stopping=False):
    """step_fn(new_tokens (B W, U) int64 on the CPU, beam_idx (B W) or None at the first call) -> logits (B W, V) fp32 on the CPU: the decoder step AFTER its cache
    followed `beam_idx`.  prompt (B, P) int64.  -> dict(kept = per utterance [(score np.float32, tokens incl. the prompt)], best first, at most W;
    sequences = (B, P + n) in `_beam_search`'s layout for num_return_sequences = 1, filled with `pad_token_id`; scores (B) = the best hypotheses' scores; steps)."""
    B, P = prompt.shape
    W = num_beams
    ids = prompt.repeat_interleave(W, 0).clone()
    beam_scores = torch.zeros((B, W), dtype=torch.float32)
    beam_scores[:, 1:] = -1e9
    beam_scores = beam_scores.view(-1)
    kept = [[] for _ in range(B)]
    done = [False] * B
    new_tok, beam_idx, steps = ids, None, 0
    while ids.shape[1] < max_length and not all(done):
        logits = step_fn(new_tok, beam_idx)
        V = logits.shape[1]
        scores = logprob_fn(logits)
        for p in processors:
            scores = p(ids, scores)
        cand = (scores.float() + beam_scores[:, None]).view(B, W * V)
        order = torch.sort(cand, dim=1, descending=True, stable=True).indices[:, :2 * W]
        top_s, top_i = torch.gather(cand, 1, order).numpy(), order.numpy()
        cur_len = ids.shape[1]
        at_max = cur_len + 1 >= max_length
        gen = cur_len + 1 - P
        hyp = (max_length - P) if (early_stopping == "never" and length_penalty > 0.0) else gen
        denom, heur = np.float32(gen ** length_penalty), np.float32(hyp ** length_penalty)
        nb_scores = torch.zeros((B, W)); nb_tok = torch.zeros((B, W), dtype=torch.long); nb_idx = torch.zeros((B, W), dtype=torch.long)
        for b in range(B):
            if done[b]:
                nb_tok[b] = pad_token_id; nb_idx[b] = b * W
                continue
            rows = [(np.float32(top_s[b, r]), int(top_i[b, r]) // V, int(top_i[b, r]) % V) for r in range(2 * W)]
            hit = [tok == eos_token_id or at_max for _, _, tok in rows]
            nxt = [(s, beam, tok) for (s, beam, tok), h in zip(rows, hit) if not h][:W]
            nxt += [(np.float32(s + NEG), beam, tok) for (s, beam, tok), h in zip(rows, hit) if h][:W - len(nxt)]
            for k, (s, beam, tok) in enumerate(nxt):
                nb_scores[b, k], nb_tok[b, k], nb_idx[b, k] = float(s), tok, b * W + beam
            for r in range(W):
                if hit[r]:
                    s, beam, tok = rows[r]
                    sc = np.float32(s / denom)
                    pos = len(kept[b])
                    while pos > 0 and sc > kept[b][pos - 1][0]:
                        pos -= 1
                    if pos < W:
                        kept[b].insert(pos, (sc, ids[b * W + beam].tolist() + [tok]))
                        del kept[b][W:]
            best = np.float32(nxt[0][0] / heur)
            unsat = best > (kept[b][W - 1][0] if len(kept[b]) == W else NEG)
            if (not unsat) or (early_stopping is True and len(kept[b]) == W) or at_max:
                done[b] = True
        beam_idx = nb_idx.view(-1)
        new_tok = nb_tok.view(-1, 1)
        beam_scores = nb_scores.view(-1)
        ids = torch.cat([ids.index_select(0, beam_idx), new_tok], 1)
        steps += 1
    width = max(len(kept[b][0][1]) for b in range(B))
    seq = torch.full((B, width), int(pad_token_id), dtype=torch.long)
    for b in range(B):
        seq[b, :len(kept[b][0][1])] = torch.tensor(kept[b][0][1])
    return dict(kept=kept, sequences=seq, scores=torch.tensor([float(kept[b][0][0]) for b in range(B)]), steps=steps)
