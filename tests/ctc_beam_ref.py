"""CTC prefix beam search restated on the CPU in float64, from the semantics in the header of huggingface_asr_amd/csrc/ctc_beam.hip (DESIGN.md 'CTC prefix beam
search'), with the two independent checks it is held to: `brute_force` enumerates every alignment, `ctc_logp` is the CTC forward recursion.  Pure Python on purpose:
no decoder library is involved anywhere.

`beam_search` also reports its own decision margins — how close the search came to deciding differently at a token cut, at a per-frame beam cut, and between the
hypotheses it returns — so that a test can keep the draws on which an fp32 device search must take the same decisions."""
import itertools
import math

import numpy as np

NEG_INF = float("-inf")


def logaddexp(a, b):
    m = a if a > b else b
    if m == NEG_INF:
        return NEG_INF
    return m + math.log1p(math.exp((b if a > b else a) - m))


def log_softmax(x):
    """x (T, V1) -> float64 log-probabilities; an entry of -inf stays -inf"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        lse = m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True))
        lp = x - lse
    lp[np.isneginf(x)] = NEG_INF
    return lp


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != blank and c != prev:
            out.append(int(c))
        prev = c
    return tuple(out)


def greedy(x, blank):
    return collapse(np.asarray(x).argmax(axis=-1).tolist(), blank)


def brute_force(lp, blank):
    """every alignment of (T, V1) log-probabilities: [(labels, log of the summed probability)] best first (equal scores: shorter, then lexicographic)"""
    lp = np.asarray(lp, dtype=np.float64)
    T, V1 = lp.shape
    acc = {}
    for path in itertools.product(range(V1), repeat=T):
        s = 0.0
        for t, c in enumerate(path):
            s += lp[t, c]
        key = collapse(path, blank)
        acc[key] = logaddexp(acc.get(key, NEG_INF), s)
    return sorted(((k, v) for k, v in acc.items() if v > NEG_INF), key=lambda kv: (-kv[1], len(kv[0]), kv[0]))


def ctc_logp(lp, labels, blank):
    """log p(labels | lp) by the CTC forward recursion over the blank-extended label sequence"""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    ext = [blank]
    for c in labels:
        ext += [int(c), blank]
    S = len(ext)
    if T == 0:
        return 0.0 if not labels else NEG_INF
    alpha = [NEG_INF] * S
    alpha[0] = lp[0, blank]
    if S > 1:
        alpha[1] = lp[0, ext[1]]
    for t in range(1, T):
        new = [NEG_INF] * S
        for s in range(S):
            a = alpha[s]
            if s >= 1:
                a = logaddexp(a, alpha[s - 1])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                a = logaddexp(a, alpha[s - 2])
            new[s] = a + lp[t, ext[s]]
        alpha = new
    return logaddexp(alpha[S - 1], alpha[S - 2]) if S > 1 else alpha[0]


def token_cut(row, blank, K):
    """the min(K, V1 - 1) non-blank classes with the largest values, equal values by lower class; and the gap between the last kept and the first cut value"""
    order = sorted((c for c in range(len(row)) if c != blank), key=lambda c: (-row[c], c))
    kept = order[:K]
    gap = float(row[order[K - 1]] - row[order[K]]) if len(order) > K else float("inf")
    return kept, gap


def beam_search(x, blank, beams, token_topk=None, nbest=1, length=None):
    """x (T, V1) logits -> dict(hyps = [(labels, score, frames)] the nbest best, best first; margins = dict(token_cut, beam_cut: the smallest gap over the frames,
    final: the gaps between consecutive hypotheses of the final beam's first nbest + 1))"""
    x = np.asarray(x, dtype=np.float64)
    T, V1 = x.shape
    n = T if length is None else max(0, min(int(length), T))
    K = min(beams, V1 - 1) if token_topk is None else token_topk
    lp = log_softmax(x[:n]) if n else np.zeros((0, V1))
    # prefixes are nodes of a trie (node 0 = the empty prefix): child[(node, class)] -> node, so the per-frame tables are keyed by small integers
    child, parent, last, entered = {}, [-1], [-1], [-1]
    beam = [(0, 0.0, NEG_INF, 0.0)]                       # (node, p_b, p_nb, score), best first
    m_tok = m_beam = float("inf")
    for t in range(n):
        toks, gap = token_cut(x[t], blank, K)
        m_tok = min(m_tok, gap)
        row = lp[t].tolist()
        lpb = row[blank]
        new = {}                                          # node -> [p_b', survivor term, extension term, tie order]
        ext = []                                          # (term, (parent node, class), tie order) of extensions to prefixes that are not survivors
        tots = []
        for r, (l, pb, pnb, _) in enumerate(beam):
            tot = logaddexp(pb, pnb)
            tots.append(tot)
            new[l] = [tot + lpb, pnb + row[last[l]] if l else NEG_INF, NEG_INF, (0, r, 0)]
        for r, (l, pb, pnb, _) in enumerate(beam):
            tot, ll = tots[r], last[l]
            for k, c in enumerate(toks):
                term = (pb if c == ll else tot) + row[c]
                e = new.get(child.get((l, c), -1))
                if e is None:
                    ext.append((term, (l, c), (1, r, k)))
                else:
                    e[2] = term                           # (one term: a prefix has one parent)
        cands = []
        for l, (pb, s_term, e_term, order) in new.items():
            pnb = logaddexp(s_term, e_term)
            sc = logaddexp(pb, pnb)
            if sc > NEG_INF:
                cands.append((-sc, order, l, pb, pnb))
        cands += [(-term, order, key, NEG_INF, term) for term, key, order in ext if term > NEG_INF]
        cands.sort(key=lambda c: (c[0], c[1]))
        if len(cands) > beams:
            m_beam = min(m_beam, cands[beams][0] - cands[beams - 1][0])
        beam = []
        for ns, _, l, pb, pnb in cands[:beams]:
            if isinstance(l, tuple):                      # a selected extension: the node its prefix had, or a new one
                node = child.get(l)
                if node is None:
                    node = child[l] = len(parent)
                    parent.append(l[0]); last.append(l[1]); entered.append(t)
                l = node
            beam.append((l, pb, pnb, -ns))
        if not beam:
            break

    def labels(node):
        out, fr = [], []
        while node > 0:
            out.append(last[node]); fr.append(entered[node])
            node = parent[node]
        return tuple(reversed(out)), list(reversed(fr))
    hyps = []
    for l, _, _, sc in beam[:nbest]:
        lab, fr = labels(l)
        hyps.append((lab, sc, fr))
    final = [beam[i][3] - beam[i + 1][3] for i in range(min(nbest, len(beam) - 1))]
    return dict(hyps=hyps, margins=dict(token_cut=m_tok, beam_cut=m_beam, final=final))


def min_margin(r):
    m = r["margins"]
    return min([m["token_cut"], m["beam_cut"]] + list(m["final"]))


def peaky(seed, T, V1, blank):
    """(T, V1) float32 logits: standard-normal noise plus a planted alignment — runs of 1-3 frames, a run is blank with probability 0.55, else a random token;
    +7.0 on the planted class, or only +1.5 on a quarter of the frames"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, V1))
    t = 0
    while t < T:
        run = int(rng.integers(1, 4))
        c = blank if rng.random() < 0.55 else int(rng.choice([k for k in range(V1) if k != blank]))
        for u in range(t, min(t + run, T)):
            x[u, c] += 1.5 if rng.random() < 0.25 else 7.0
        t += run
    return x.astype(np.float32)
