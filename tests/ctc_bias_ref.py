"""Contextual biasing of the CTC prefix beam search restated on the CPU in float64, from the semantics in the header of huggingface_asr_amd/csrc/ctc_beam_bias.hip
(DESIGN.md §4 'Contextual biasing'), on ctc_beam_ref's functions.  Four pieces:

  credit         the credit n(l) of a label sequence, straight from the definition: the matched string is kept explicitly and suffixes are found by string search — no
                 trie nodes, no failure table, no compiled tables (ctc_bias.CtcBias is held to it)
  enumerate_all  every label sequence l of at most T labels with ctc_logp(l) + w n(l): what a search that prunes nothing must rank
  BiasedSearch   the prefix search of ctc_beam_ref.beam_search with the biased selection value, suspended between calls as a beam stream is: walk(rows) any number of
                 times, then hyps() / committed(); it reports the same decision margins as beam_search, measured on the biased values
  beam_search    BiasedSearch over a whole utterance in one call, in beam_search's format plus the credits
"""
import itertools

import numpy as np

from ctc_beam_ref import NEG_INF, ctc_logp, log_softmax, logaddexp, token_cut


def credit(phrases, seq):
    """n(seq) for the phrase list: m is the string matched so far (always a prefix of some phrase), k what completed phrases have kept"""
    P = {tuple(p) for p in phrases}
    prefixes = {p[:i] for p in P for i in range(len(p) + 1)} | {()}
    m, k = (), 0
    for c in seq:
        c = int(c)
        if m + (c,) in prefixes:                              # 1. the match goes on
            m = m + (c,)
            continue
        keep = max((i for i in range(1, len(m) + 1) if m[:i] in P), default=0)
        if keep > 0:                                          # 2. a phrase has ended inside the match: it stays, the rest is given back
            k += keep
            m = ()
        else:                                                 # 3. the longest proper suffix that is still the beginning of a phrase
            while m and m + (c,) not in prefixes:
                m = next(m[i:] for i in range(1, len(m) + 1) if m[i:] in prefixes)
        if m + (c,) in prefixes:                              # 4.
            m = m + (c,)
    return k + len(m)


def biased(score, w, n):
    return NEG_INF if score == NEG_INF else score + w * n


def enumerate_all(x, blank, phrases, w):
    """x (T, V1) logits -> [(labels, ctc log-probability, credit)] of every label sequence with a finite probability, by biased value, best first (equal values:
    shorter, then lexicographic)"""
    x = np.asarray(x, dtype=np.float64)
    T, V1 = x.shape
    lp = log_softmax(x)
    labels = [c for c in range(V1) if c != blank]
    out = []
    for n in range(T + 1):
        for l in itertools.product(labels, repeat=n):
            s = ctc_logp(lp, list(l), blank)
            if s > NEG_INF:
                out.append((l, s, credit(phrases, l)))
    return sorted(out, key=lambda e: (-biased(e[1], w, e[2]), len(e[0]), e[0]))


class BiasedSearch:
    """ctc_beam_ref.beam_search's walk with the biased selection value, kept between calls.  phrases = [] or w = 0 is the unbiased search."""

    def __init__(self, blank, beams, token_topk=None, nbest=1, phrases=(), w=0.0):
        self.blank, self.beams, self.token_topk, self.nbest = blank, beams, token_topk, nbest
        self.phrases, self.w = [tuple(p) for p in phrases], float(w)
        self.reset()

    def reset(self):
        # prefixes are nodes of a trie (node 0 = the empty prefix), as in beam_search; cred[node] = n of the node's labels
        self.child, self.parent, self.last, self.entered, self.cred = {}, [-1], [-1], [-1], [0]
        self.beam = [(0, 0.0, NEG_INF, 0.0)]                  # (node, p_b, p_nb, score), best first by biased value
        self.t = 0
        self.m_tok = self.m_beam = float("inf")

    def labels(self, node):
        out, fr = [], []
        while node > 0:
            out.append(self.last[node]); fr.append(self.entered[node])
            node = self.parent[node]
        return tuple(reversed(out)), list(reversed(fr))

    def walk(self, x):
        """x (n, V1): the next n frames"""
        x = np.asarray(x, dtype=np.float64)
        if x.shape[0] == 0 or not self.beam:
            return
        K = min(self.beams, x.shape[1] - 1) if self.token_topk is None else self.token_topk
        lp = log_softmax(x)
        child, parent, last, cred, blank, w = self.child, self.parent, self.last, self.cred, self.blank, self.w
        for u in range(x.shape[0]):
            toks, gap = token_cut(x[u], blank, K)
            self.m_tok = min(self.m_tok, gap)
            row = lp[u].tolist()
            new, ext, tots = {}, [], []
            for r, (l, pb, pnb, _) in enumerate(self.beam):
                tot = logaddexp(pb, pnb)
                tots.append(tot)
                new[l] = [tot + row[blank], pnb + row[last[l]] if l else NEG_INF, NEG_INF, (0, r, 0)]
            for r, (l, pb, pnb, _) in enumerate(self.beam):
                tot, ll = tots[r], last[l]
                for k, c in enumerate(toks):
                    term = (pb if c == ll else tot) + row[c]
                    e = new.get(child.get((l, c), -1))
                    if e is None:
                        ext.append((term, (l, c), (1, r, k)))
                    else:
                        e[2] = term
            cands = []                                        # (-biased value, tie order, node or (parent, class), p_b, p_nb, score, credit)
            for l, (pb, s_term, e_term, order) in new.items():
                pnb = logaddexp(s_term, e_term)
                sc = logaddexp(pb, pnb)
                if sc > NEG_INF:
                    cands.append((-biased(sc, w, cred[l]), order, l, pb, pnb, sc, cred[l]))
            for term, key, order in ext:
                if term > NEG_INF:
                    node = child.get(key)
                    n = cred[node] if node is not None else credit(self.phrases, self.labels(key[0])[0] + (key[1],))
                    cands.append((-biased(term, w, n), order, key, NEG_INF, term, term, n))
            cands.sort(key=lambda c: (c[0], c[1]))
            if len(cands) > self.beams:
                self.m_beam = min(self.m_beam, cands[self.beams][0] - cands[self.beams - 1][0])
            self.beam = []
            for _, _, l, pb, pnb, sc, n in cands[:self.beams]:
                if isinstance(l, tuple):
                    node = child.get(l)
                    if node is None:
                        node = child[l] = len(parent)
                        parent.append(l[0]); last.append(l[1]); self.entered.append(self.t); cred.append(n)
                    l = node
                self.beam.append((l, pb, pnb, sc))
            self.t += 1
            if not self.beam:
                break

    def hyps(self):
        """[(labels, ctc score, frames, credit)] the nbest best"""
        return [(*self.labels(l)[:1], sc, self.labels(l)[1], self.cred[l]) for l, _, _, sc in self.beam[:self.nbest]]

    def committed(self):
        """the longest common prefix of ALL hypotheses of the beam"""
        labs = [self.labels(l)[0] for l, _, _, _ in self.beam]
        if not labs:
            return ()
        n = 0
        while all(len(a) > n for a in labs) and len({a[n] for a in labs}) == 1:
            n += 1
        return labs[0][:n]

    def margins(self):
        v = [biased(sc, self.w, self.cred[l]) for l, _, _, sc in self.beam]
        return dict(token_cut=self.m_tok, beam_cut=self.m_beam, final=[v[i] - v[i + 1] for i in range(min(self.nbest, len(v) - 1))])


def beam_search(x, blank, beams, token_topk=None, nbest=1, length=None, phrases=(), w=0.0):
    """x (T, V1) logits -> dict(hyps = [(labels, ctc score, frames, credit)], margins) as ctc_beam_ref.beam_search, biased"""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0] if length is None else max(0, min(int(length), x.shape[0]))
    s = BiasedSearch(blank, beams, token_topk, nbest, phrases, w)
    s.walk(x[:n])
    return dict(hyps=s.hyps(), margins=s.margins())


def min_margin(r):
    m = r["margins"]
    return min([m["token_cut"], m["beam_cut"]] + list(m["final"]))


# ---- the certified case, shared by tests/test_ctc_bias_cpu.py (which certifies the seeds) and tests/test_gpu_ctc_bias.py (which runs them on the device)
CERT_T, CERT_V1, CERT_W, CERT_K, CERT_NBEST = 48, 40, 8, 8, 4
CERT_WEIGHTS = (0.5, 2.0)                                     # dyadic: w n is exact in fp32
CERT_SEEDS = (1, 4, 10, 11)                                   # draws whose smallest float64 decision margin is >= CERT_MARGIN at both weights
CERT_MARGIN = 1e-3


def cert_case(seed):
    """-> (x (T, V1) float32 peaky logits, blank, phrases): three tokens of the greedy answer as one phrase, a two-token piece of it, and three random phrases"""
    from ctc_beam_ref import greedy, peaky
    blank = CERT_V1 - 1
    x = peaky(4000 + seed, CERT_T, CERT_V1, blank)
    g = greedy(x, blank)
    rng = np.random.default_rng(77 + seed)
    phrases = [list(g[2:5]), list(g[6:8])] + [[int(t) for t in rng.integers(0, blank, size=int(rng.integers(1, 4)))] for _ in range(3)]
    return x, blank, [p for p in phrases if p]


def phrases_4096():
    """64 phrases of 64 tokens over classes < 72 whose trie has exactly 4096 states: 62 with first tokens of their own (62 x 64 nodes), two that share their first token
    (1 + 63 + 63), and the root"""
    return [[i] + [70] * 63 for i in range(62)] + [[62] + [70] * 63, [62] + [71] * 63]
