"""Host restatements of CTC forced alignment (csrc/ctc_align.hip), pure numpy / Python:

  viterbi64    the recursion in float64, with the exact decision margin of its answer;
  brute_force  every alignment of a tiny case, enumerated;
  viterbi32    the kernel's semantics bit for bit: np.float32 arithmetic in the stated order, the stated tie rules, the stated fills.

States of a target l_0 .. l_{n-1}: s = 0 .. 2n, blank at even s, l_{s >> 1} at odd s."""
import itertools

import numpy as np

NEG = float("-inf")


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def row_lse32(x):
    """float32 log-sum-exp of the rows of x (computed in float64, rounded once)"""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1)
    return (m + np.log(np.exp(x - m[..., None]).sum(-1))).astype(np.float32)


def rounding_bound(T, max_delta):
    """T * 2^-23 * max|delta|: what one rounded float32 add per frame can lose, for the chosen and for the optimal path together"""
    return T * 2.0 ** -23 * max_delta


def draw_labels(n, V1, seed, repeats=False):
    """n labels below the blank V1 - 1; with `repeats` every third label equals its predecessor"""
    g = np.random.default_rng(1000 + seed)
    lab = []
    for i in range(n):
        if repeats and i % 3 == 1:
            lab.append(lab[-1])
        else:
            c = int(g.integers(0, V1 - 1))
            while lab and c == lab[-1]:
                c = int(g.integers(0, V1 - 1))
            lab.append(c)
    return lab


def check_c_entry_refusals():
    """mi_ctc_align's documented refusals, from argument checks alone: nothing is launched, so this runs with or without a device"""
    from huggingface_asr_amd import _lib
    L = _lib.lib()
    buf = (_lib.C.c_char * 4096)()
    p = (_lib.C.addressof(buf) + 15) & ~15

    def call(V1=5, blank=4, T=4, U=2, B=1, dtype=0, ws=None, ws_bytes=0, spans=(p, p, p)):
        return L.mi_ctc_align(p, 64, 8, dtype, p, T, p, U, p, blank, V1, B, ws, ws_bytes, p, p, p, *spans, None)
    for kw in (dict(V1=1, blank=0), dict(blank=5), dict(blank=-1), dict(T=0), dict(U=-1), dict(B=0), dict(dtype=2), dict(spans=(p, None, p)), dict(spans=(None, None, p))):
        assert call(**kw) == _lib.ERR_ARG, kw
    for kw in (dict(U=1024), dict(T=(1 << 20) + 1)):
        assert call(**kw) == _lib.ERR_UNSUPPORTED, kw
    need = L.mi_ctc_align_workspace_bytes(1, 4096, 512)
    assert need == 512 * 768 * 4                                           # 512 rows of 8 frames x 768 pairs, a word each: U = 512 at T = 4096 is inside the bounds
    assert L.mi_ctc_align_workspace_bytes(3, 4096, 512) == 3 * need
    for kw in (dict(ws=None, ws_bytes=need), dict(ws=p, ws_bytes=need - 1), dict(ws=p + 8, ws_bytes=need)):      # missing, too small, not 16-byte aligned
        assert call(T=4096, U=512, **kw) == _lib.ERR_ARG, kw
    assert L.mi_ctc_align_workspace_bytes(32, 250, 40) == 0 and L.mi_ctc_align_workspace_bytes(32, 250, 120) == 0      # the head's shapes keep their backpointers in LDS
    assert L.mi_ctc_align_workspace_bytes(1, 1500, 400) > 0
    assert L.mi_ctc_align_workspace_bytes(1, 4, 1024) == 0 and L.mi_ctc_align_workspace_bytes(0, 4, 4) == 0             # refused shapes need nothing


def target(row):
    return [int(v) for v in row if v >= 0]


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        c = int(c)
        if c != blank and c != prev:
            out.append(c)
        prev = c
    return out


def extended(labels, blank):
    ext = [blank]
    for l in labels:
        ext += [int(l), blank]
    return ext


def path_score(lp, path):
    """float64 sum of lp (T, V1) along a per-frame class path"""
    return float(sum(float(lp[t, int(c)]) for t, c in enumerate(path)))


def _skips(ext, blank):
    return np.array([s >= 3 and (s & 1) == 1 and ext[s] != ext[s - 2] for s in range(len(ext))])


def viterbi64(lp, labels, blank):
    """lp (T, V1) log-probabilities (any float dtype; used as float64), labels: the target.  -> dict(score, states, path, margin, max_delta): the best alignment's
    log-probability, its state and class per frame, max_delta = the largest finite |delta[t][s]| of the recursion (what the rounding bound of a float32
    run of it scales with), and the exact decision margin = score minus the best score of any alignment through a (t, s) cell
    that is not on the returned path (+inf when there is no such alignment).  Infeasible: score -inf, states / path None, margin +inf."""
    lp = np.asarray(lp, dtype=np.float64)
    T = lp.shape[0]
    labels = [int(v) for v in labels]
    n = len(labels)
    ext = extended(labels, blank)
    S = 2 * n + 1
    skip = _skips(ext, blank)
    e = lp[:, ext]                                                         # (T, S)
    F = np.full((T, S), NEG)
    bp = np.zeros((T, S), dtype=np.int64)
    F[0, 0] = e[0, 0]
    if n:
        F[0, 1] = e[0, 1]
    for t in range(1, T):
        a0 = F[t - 1]
        a1 = np.concatenate([[NEG], a0[:-1]])
        a2 = np.where(skip, np.concatenate([[NEG, NEG], a0[:-2]])[:S], NEG)
        best, code = a0.copy(), np.zeros(S, dtype=np.int64)
        m = a1 > best
        best[m], code[m] = a1[m], 1
        m = a2 > best
        best[m], code[m] = a2[m], 2
        with np.errstate(invalid="ignore"):
            F[t] = best + e[t]
        bp[t] = code
    vhi, vlo = F[T - 1, 2 * n], (F[T - 1, 2 * n - 1] if n else NEG)
    s = 2 * n - 1 if vlo > vhi else 2 * n
    score = float(max(vhi, vlo))
    if not score > NEG:
        return dict(score=NEG, states=None, path=None, margin=float("inf"), max_delta=0.0)
    states = [0] * T
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    # backward max sweep: Bk[t][s] = the best continuation from state s at frame t (its own emission excluded) to a final state
    Bk = np.full((T, S), NEG)
    Bk[T - 1, 2 * n] = 0.0
    if n:
        Bk[T - 1, 2 * n - 1] = 0.0
    for t in range(T - 2, -1, -1):
        nxt = e[t + 1] + Bk[t + 1]
        b1 = np.concatenate([nxt[1:], [NEG]])
        b2 = np.concatenate([np.where(skip[2:], nxt[2:], NEG), [NEG, NEG]]) if S >= 2 else np.full(S, NEG)
        Bk[t] = np.maximum(nxt, np.maximum(b1, b2[:S]))
    through = F + Bk
    on = np.zeros((T, S), dtype=bool)
    on[np.arange(T), states] = True
    off = through[~on]
    off = off[off > NEG] if off.size else off
    margin = float(score - off.max()) if off.size else float("inf")
    return dict(score=score, states=states, path=[ext[s] for s in states], margin=margin, max_delta=float(np.abs(F[np.isfinite(F)]).max()))


def brute_force(lp, labels, blank):
    """every per-frame class sequence of lp (T <= 6, V1 <= 4) whose collapse is `labels`: -> (best score, [the paths that reach it]); (-inf, []) when none exists"""
    lp = np.asarray(lp, dtype=np.float64)
    T, V1 = lp.shape
    assert T <= 6 and V1 <= 4
    labels = [int(v) for v in labels]
    best, paths = NEG, []
    for p in itertools.product(range(V1), repeat=T):
        if collapse(p, blank) != labels:
            continue
        sc = path_score(lp, p)
        if sc > best:
            best, paths = sc, [list(p)]
        elif sc == best:
            paths.append(list(p))
    return best, paths


def viterbi32(x, lse, label_row, in_len, blank):
    """The kernel's semantics for one utterance: x (T, V1) the logits as float32 values, lse (T) float32, label_row (U) int64 with negative padding anywhere,
    in_len the frames that count.  -> dict(path (T) int32, score float32, tgt_len, start (U), end (U) int32, token_lp (U) float32) with the documented fills."""
    x = np.asarray(x, dtype=np.float32)
    lse = np.asarray(lse, dtype=np.float32)
    T, V1 = x.shape
    U = len(label_row)
    lab = target(label_row)
    n = len(lab)
    nb = min(max(int(in_len), 0), T)
    out = dict(path=np.full(T, -1, dtype=np.int32), score=np.float32(NEG), tgt_len=n, start=np.full(U, -1, dtype=np.int32), end=np.full(U, -1, dtype=np.int32),
               token_lp=np.zeros(U, dtype=np.float32))
    bad = any(l >= V1 or l == blank for l in lab)
    rep = sum(1 for i in range(1, n) if lab[i] == lab[i - 1])
    if bad or nb < n + rep or (nb == 0 and n > 0):
        return out
    if nb == 0:
        out["score"] = np.float32(0.0)
        return out
    ext = extended(lab, blank)
    S = 2 * n + 1
    skip = _skips(ext, blank)
    with np.errstate(invalid="ignore"):
        e = x[:nb][:, ext] - lse[:nb, None]                                # float32 - float32: one rounded subtraction per cell
    assert e.dtype == np.float32
    ninf = np.float32(NEG)
    d = np.full(S, ninf, dtype=np.float32)
    d[0] = e[0, 0]
    if n:
        d[1] = e[0, 1]
    bp = np.zeros((nb, S), dtype=np.int8)
    for t in range(1, nb):
        a1 = np.concatenate([[ninf], d[:-1]]).astype(np.float32)
        a2 = np.concatenate([[ninf, ninf], d[:-2]])[:S].astype(np.float32)
        best, code = d.copy(), np.zeros(S, dtype=np.int8)
        m = a1 > best                                                      # strictly greater: the earlier candidate keeps a tie
        best[m], code[m] = a1[m], 1
        m = skip & (a2 > best)
        best[m], code[m] = a2[m], 2
        with np.errstate(invalid="ignore"):
            d = best + e[t]                                                # float32 + float32
        assert d.dtype == np.float32
        bp[t] = code
    vhi, vlo = d[2 * n], (d[2 * n - 1] if n else ninf)
    lo = bool(vlo > vhi)
    score = vlo if lo else vhi
    if not score > ninf:
        return out
    s = 2 * n - 1 if lo else 2 * n
    states = np.zeros(nb, dtype=np.int64)
    for t in range(nb - 1, -1, -1):
        states[t] = s
        s -= int(bp[t, s])
    out["score"] = np.float32(score)
    out["path"][:nb] = np.asarray(ext, dtype=np.int32)[states]
    for u in range(n):
        fr = np.nonzero(states == 2 * u + 1)[0]
        assert fr.size and (np.diff(fr) == 1).all()
        out["start"][u], out["end"][u] = fr[0], fr[-1] + 1
        acc = np.float32(0.0)
        for t in fr:
            acc = np.float32(acc + e[t, 2 * u + 1])
        out["token_lp"][u] = acc
    return out


def viterbi32_batch(x, lse, labels, in_len, blank):
    """viterbi32 per utterance, stacked: x (B, T, V1), lse (B, T), labels (B, U), in_len (B) or None"""
    B, T, _ = x.shape
    rows = [viterbi32(x[b], lse[b], labels[b], T if in_len is None else in_len[b], blank) for b in range(B)]
    return {k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]}
