"""The float64 restatement of the CTC prefix beam search (tests/ctc_beam_ref.py, imported, not modified) in suspended form: `BeamStream` holds the walk's state
between calls, as huggingface_asr_amd/csrc/ctc_beam_stream.hip does on the device, and reports the committed prefix — the longest common prefix of ALL hypotheses of
the beam.  The frame step below is beam_search's loop body, statement for statement; tests/test_stream_beam_cpu.py holds the two to each other for every way of
splitting the frames into calls."""
import numpy as np

import ctc_beam_ref as R

NEG_INF = R.NEG_INF


def lcp(seqs):
    """the longest common prefix of a list of sequences (the empty list: the empty prefix)"""
    seqs = [tuple(s) for s in seqs]
    if not seqs:
        return ()
    n = 0
    while all(len(s) > n for s in seqs) and len({s[n] for s in seqs}) == 1:
        n += 1
    return seqs[0][:n]


def compositions(T):
    """every way of delivering T frames as a sequence of calls of 0 or more frames: every composition of T into positive parts, and each of them with one empty call
    put in at every position (a call without frames changes nothing, so one at a time covers them)"""
    out = []
    for mask in range(1 << max(T - 1, 0)):
        parts, run = [], 1
        for i in range(T - 1):
            if mask >> i & 1:
                parts.append(run); run = 1
            else:
                run += 1
        parts.append(run)
        if T == 0:
            parts = []
        out.append(parts)
        for at in range(len(parts) + 1):
            out.append(parts[:at] + [0] + parts[at:])
    return out


# The planted case of the committed-prefix tests (CPU and GPU, the same inputs): peaked logits from a planted label sequence plus noise.  The seed was picked with this
# reference so that, in chunks of 5, the committed prefix grows in several steps (1, 2, ..., 11, 16 tokens) and lags the best hypothesis; the CPU test asserts that.
PLANTED = dict(seed=7, T=48, V1=12, W=8, K=8, chunk=5)


def planted_logits():
    c = PLANTED
    return R.peaky(c["seed"], c["T"], c["V1"], c["V1"] - 1)


def chunks(T, size):
    return [min(size, T - lo) for lo in range(0, T, size)]


class BeamStream:
    def __init__(self, blank, beams, token_topk=None):
        self.blank, self.beams, self.token_topk = blank, beams, token_topk
        self.child, self.parent, self.last, self.entered = {}, [-1], [-1], [-1]
        self.beam = [(0, 0.0, NEG_INF, 0.0)]                # (node, p_b, p_nb, score), best first
        self.t = 0                                          # frames walked: the stamps are global frame indices
        self.committed, self.committed_frames = (), []
        self.finished = False

    def _labels(self, node):
        out, fr = [], []
        while node > 0:
            out.append(self.last[node]); fr.append(self.entered[node])
            node = self.parent[node]
        return tuple(reversed(out)), list(reversed(fr))

    def hyps(self, nbest=None):
        """[(labels, score, frames)] of the beam's first nbest (all), best first"""
        out = []
        for l, _, _, sc in self.beam[:nbest]:
            labels, frames = self._labels(l)
            out.append((labels, sc, frames))
        return out

    def _frame(self, x_row):
        child, parent, last, entered, beams, blank, t = self.child, self.parent, self.last, self.entered, self.beams, self.blank, self.t
        V1 = len(x_row)
        K = min(beams, V1 - 1) if self.token_topk is None else self.token_topk
        toks, _ = R.token_cut(x_row, blank, K)
        row = R.log_softmax(np.asarray(x_row, dtype=np.float64)[None])[0].tolist()
        lpb = row[blank]
        new, ext, tots = {}, [], []
        for r, (l, pb, pnb, _) in enumerate(self.beam):
            tot = R.logaddexp(pb, pnb)
            tots.append(tot)
            new[l] = [tot + lpb, pnb + row[last[l]] if l else NEG_INF, NEG_INF, (0, r, 0)]
        for r, (l, pb, pnb, _) in enumerate(self.beam):
            tot, ll = tots[r], last[l]
            for k, c in enumerate(toks):
                term = (pb if c == ll else tot) + row[c]
                e = new.get(child.get((l, c), -1))
                if e is None:
                    ext.append((term, (l, c), (1, r, k)))
                else:
                    e[2] = term
        cands = []
        for l, (pb, s_term, e_term, order) in new.items():
            pnb = R.logaddexp(s_term, e_term)
            sc = R.logaddexp(pb, pnb)
            if sc > NEG_INF:
                cands.append((-sc, order, l, pb, pnb))
        cands += [(-term, order, key, NEG_INF, term) for term, key, order in ext if term > NEG_INF]
        cands.sort(key=lambda c: (c[0], c[1]))
        beam = []
        for ns, _, l, pb, pnb in cands[:beams]:
            if isinstance(l, tuple):
                node = child.get(l)
                if node is None:
                    node = child[l] = len(parent)
                    parent.append(l[0]); last.append(l[1]); entered.append(t)
                l = node
            beam.append((l, pb, pnb, -ns))
        self.beam = beam
        self.t = t + 1

    def feed(self, x, final=False):
        """x (n, V1) logits, n >= 0 -> the number of tokens this call committed"""
        assert not self.finished
        for x_row in np.asarray(x, dtype=np.float64):
            if not self.beam:                               # an empty beam: the one-shot walk stops there too
                break
            self._frame(x_row)
        before = len(self.committed)
        if self.beam:
            every = self.hyps()
            labels = every[0][0] if final else lcp([h[0] for h in every])
            assert labels[:before] == self.committed, "the committed prefix is append-only"
            self.committed = labels
            self.committed_frames = every[0][2][:len(labels)]
        self.finished = bool(final)
        return len(self.committed) - before
