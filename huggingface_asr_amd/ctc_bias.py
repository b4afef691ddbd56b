"""Contextual biasing of the CTC prefix beam search: a phrase list ("hotwords") compiled to the two tables the biased frame step reads
(csrc/ctc_beam_bias.hip states the semantics; DESIGN.md §4 'Contextual biasing' repeats them).

    ctx = CtcBias([[7, 3, 9], [12]], weight=1.5, vocab=V + 1, blank=V)
    ops.ctc_beam_decode(logits, V, pad, beams=10, bias=ctx)

A hypothesis with label prefix l is selected and ranked by score + weight * n(l); n(l), the credit, is an integer defined by walking l through the phrase trie:
the state is (s, k), start (root, 0); for a token c
  1. s has a child for c: s <- child(s, c);
  2. otherwise, keep(s) > 0 (a phrase ends on the path root -> s, the deepest at depth keep(s)): k <- k + keep(s), s <- root;
  3. otherwise: while s != root and s has no child for c, s <- fail(s) (the Aho-Corasick failure link); nothing is kept;
  4. after 2 or 3: if s has a child for c, s <- child(s, c);
and n(l) = k + depth(s).  n depends on s and c alone, so the walk compiles to a table: `col` (V1) maps a token to its alphabet column (0: in no phrase), `tab` (S, A1) holds
per (state, column) the word (dn << 16) | next with dn = n' - n as an int16 and next < S.  Pure host code: numpy builds the tables, torch only carries them to the device.
"""
from __future__ import annotations

import math

import numpy as np

MAX_STATES, MAX_COLUMNS, MAX_WORDS, MAX_WEIGHT = 4096, 1024, 1 << 20, 100.0


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


class CtcBias:
    """A bias context: `phrases` (lists of token ids in [0, vocab), none of them `blank`; duplicates count once; the list may be empty) and one `weight` in
    log-probability units per credited token (finite, |weight| <= 100, negative allowed), for logits of `vocab` = V + 1 classes.  ValueError for a phrase, token or
    weight outside that, and for a trie beyond 1 <= S <= 4096 states, A1 <= 1024 columns or S * A1 <= 2^20 words."""

    def __init__(self, phrases, weight, vocab, blank):
        if not _is_int(vocab) or not _is_int(blank):
            raise TypeError("CtcBias: vocab and blank are ints")
        vocab, blank = int(vocab), int(blank)
        if vocab < 2 or not 0 <= blank < vocab:
            raise ValueError(f"CtcBias: at least two classes and a blank inside them, got vocab={vocab}, blank={blank}")
        try:
            weight = float(weight)
        except (TypeError, ValueError):
            raise TypeError("CtcBias: weight is a number") from None
        if not math.isfinite(weight) or abs(weight) > MAX_WEIGHT:
            raise ValueError(f"CtcBias: weight must be finite and within +-{MAX_WEIGHT:g}, got {weight}")
        seen, kept = set(), []
        for ph in phrases:
            ph = tuple(ph)
            if not ph:
                raise ValueError("CtcBias: an empty phrase")
            for t in ph:
                if not _is_int(t):
                    raise TypeError(f"CtcBias: a phrase is a list of token ids, got {t!r}")
                if not 0 <= t < vocab or t == blank:
                    raise ValueError(f"CtcBias: token {t} outside [0, {vocab}) or equal to blank {blank}")
            ph = tuple(int(t) for t in ph)
            if ph not in seen:
                seen.add(ph)
                kept.append(ph)
        self.phrases, self.weight, self.vocab, self.blank = tuple(kept), float(np.float32(weight)), vocab, blank

        # ---- the trie: children, depth, phrase ends; nodes in creation order, the root is 0
        alphabet = sorted({t for ph in kept for t in ph})
        self.A1 = len(alphabet) + 1
        if self.A1 > MAX_COLUMNS:
            raise ValueError(f"CtcBias: {self.A1 - 1} distinct tokens; at most {MAX_COLUMNS - 1}")
        col = np.zeros((vocab,), np.int32)
        col[alphabet] = np.arange(1, self.A1, dtype=np.int32)
        children, depth, ends = [{}], [0], [False]
        for ph in kept:
            s = 0
            for t in ph:
                c = int(col[t])
                if c not in children[s]:
                    if len(children) >= MAX_STATES:
                        raise ValueError(f"CtcBias: the phrase trie has more than {MAX_STATES} states")
                    children[s][c] = len(children)
                    children.append({})
                    depth.append(depth[s] + 1)
                    ends.append(False)
                s = children[s][c]
            ends[s] = True
        self.S = len(children)
        if self.S * self.A1 > MAX_WORDS:
            raise ValueError(f"CtcBias: {self.S} states x {self.A1} columns exceed {MAX_WORDS} table words")

        # ---- breadth first: keep, the failure links and the plain Aho-Corasick goto G (rule 3 followed by rule 4)
        S, A1 = self.S, self.A1
        depth = np.asarray(depth, np.int64)
        keep, fail = np.zeros((S,), np.int64), np.zeros((S,), np.int64)
        G = np.zeros((S, A1), np.int64)
        has = np.zeros((S, A1), bool)
        order, head = [0], 0
        while head < len(order):
            s = order[head]
            head += 1
            if s:
                G[s] = G[fail[s]]
            for c, ch in children[s].items():
                fail[ch] = G[s, c] if s else 0                           # (read before the child overwrites it: the goto of s's failure state)
                keep[ch] = depth[ch] if ends[ch] else keep[s]
                order.append(ch)
            for c, ch in children[s].items():
                G[s, c] = ch
                has[s, c] = True
        # rule 2 where a phrase has ended on the path and the token has no child: the phrase stays, the walk restarts at the root
        rule2 = (keep > 0)[:, None] & ~has
        nxt = np.where(rule2, G[0][None, :], G)
        dn = depth[nxt] - depth[:, None] + np.where(rule2, keep[:, None], 0)
        assert nxt.min() >= 0 and nxt.max() < S and dn.min() >= -32768 and dn.max() <= 32767
        self.col = col
        self.tab = (((dn & 0xFFFF) << 16) | nxt).astype(np.uint32).view(np.int32).reshape(S, A1)
        self._dev = {}

    def credit(self, tokens) -> int:
        """n(tokens), by walking the compiled tables as the kernel does"""
        s = n = 0
        for t in tokens:
            w = int(self.tab[s, self.col[int(t)]])
            n += w >> 16
            s = w & 0xFFFF
        return n

    def to(self, device):
        """-> (col, tab) as int32 tensors on `device`; one copy per device, kept"""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.col).to(device), torch.from_numpy(self.tab).contiguous().to(device))
        return self._dev[key]

    def __repr__(self):
        return f"CtcBias({len(self.phrases)} phrases, weight={self.weight:g}, vocab={self.vocab}, blank={self.blank}, S={self.S}, A1={self.A1})"
