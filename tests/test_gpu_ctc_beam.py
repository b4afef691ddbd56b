"""GPU: CTC prefix beam search on the device (csrc/ctc_beam.hip; ops.ctc_beam_cut / ops.ctc_beam_decode, decoding.ctc_beam_decode, EBranchformerEngine.transcribe
with beams) against the float64 restatement of its semantics and the enumeration of every alignment (tests/ctc_beam_ref.py; tests/test_ctc_beam_cpu.py holds those two
to each other).

Tolerances are derived, not measured: scores absolute 1e-3 (fp32 accumulation, T ulp for |score| < 128 and T <= 64); launch A's log-probabilities 2e-5 for |x| <= 16.
A draw is compared hypothesis for hypothesis only where the float64 search itself reports decision margins above those errors; how many draws must qualify is asserted.
Logits are unquantised fp32 from seeded generators (quantised ones produce exact score ties)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ctc_beam_ref as R  # noqa: E402
from test_ctc_beam_cpu import SMALL, DRAWS, small_logits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = -5
SCORE_TOL, LP_TOL = 1e-3, 2e-5


def decode(x, blank, lengths=None, **kw):
    from huggingface_asr_amd import ops
    out = ops.ctc_beam_decode(torch.as_tensor(x).to(DEV), blank, PAD, None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).to(DEV), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def hyps_of(out, b):
    """[(labels, score)] of utterance b's rows that exist; asserts the padding and the filling of the rows that do not"""
    res = []
    nbest, T = out["tokens"].shape[1:]
    for r in range(nbest):
        n, sc = int(out["n_tokens"][b, r]), float(out["scores"][b, r])
        assert (out["tokens"][b, r, n:] == PAD).all()
        if "frames" in out:
            assert (out["frames"][b, r, n:] == -1).all()
        if sc == float("-inf"):
            assert n == 0 and (out["tokens"][b, r] == PAD).all()
            assert all(float(s) == float("-inf") for s in out["scores"][b, r:])          # missing rows come last
            continue
        res.append((tuple(int(v) for v in out["tokens"][b, r, :n]), sc))
    return res


def check_lower_bound(x, blank, hyps, n=None):
    """every returned score is the sum of SOME of its hypothesis' alignments: at most the exact log-probability; hypotheses distinct, scores non-increasing"""
    lp = R.log_softmax(np.asarray(x, dtype=np.float64)[:n])
    assert len({h[0] for h in hyps}) == len(hyps)
    assert all(a[1] >= b[1] for a, b in zip(hyps, hyps[1:]))
    for labels, sc in hyps:
        assert sc <= R.ctc_logp(lp, labels, blank) + SCORE_TOL, (labels, sc)


# ------------------------------------------------------------------------------------------------ 1. launch A alone
def _cut_rows(V1, seed):
    g = np.random.default_rng(seed)
    x = np.clip(g.standard_normal((2, 6, V1)) * 3.0, -16.0, 16.0).astype(np.float32)
    x[0, 1, : V1 // 2] = float("-inf")                                     # rows holding -inf entries: fewer finite classes than K
    x[0, 2, 1:] = float("-inf")
    x[1, 0, :] = 0.25                                                      # deliberately equal values: all, and a pair on top
    x[1, 1, 0] = x[1, 1, V1 - 2] = 9.5
    x[1, 2, :] = np.round(x[1, 2, :])                                      # many ties
    return x


def _cut_reference(x, blank, K):
    B, T, V1 = x.shape
    Kk = min(K, V1 - 1)
    ids = np.full((B, T, K), -1, dtype=np.int64)
    lp = np.full((B, T, K), float("-inf"))
    lpb = np.zeros((B, T))
    for b in range(B):
        full = R.log_softmax(x[b])
        for t in range(T):
            kept, _ = R.token_cut(x[b, t].tolist(), blank, Kk)             # a stable sort: value descending, index ascending
            ids[b, t, :Kk] = kept
            lp[b, t, :Kk] = full[t, kept]
            lpb[b, t] = full[t, blank]
    return ids, lp, lpb


def _close(got, want, tol):
    inf = np.isneginf(want)
    return np.array_equal(np.isneginf(got), inf) and (np.abs(got[~inf] - want[~inf]) <= tol).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V1", [5, 40, 301, 5001])
def test_cut_is_exact(V1, dtype):
    from huggingface_asr_amd import ops
    x = torch.from_numpy(_cut_rows(V1, 40 + V1)).to(dtype)
    xr = x.float().numpy()                                                 # the values the kernel sees
    B, T, _ = x.shape
    ld = (V1 + 7) // 8 * 8 + 8
    buf = torch.full((B, T, ld), 1e30, dtype=dtype)                        # the padding would win every row if it were read as classes
    views = []
    for off in (0, 1):                                                     # the engine's layout (rows 16-B aligned, padded to a multiple of 8), and rows that are not aligned
        bd = buf.clone()
        bd[..., off:off + V1] = x
        v = bd.to(DEV)[..., off:off + V1]
        assert v.stride() == (T * ld, ld, 1) and (v.data_ptr() % 16 == 0) == (off == 0)
        views.append(v)
    for blank in (V1 - 1, 2):
        for K in (1, 8, 24, 64):
            ids, lp, lpb = _cut_reference(xr, blank, K)
            for v in views:
                got = ops.ctc_beam_cut(v, blank, K)
                assert np.array_equal(got["ids"].cpu().numpy(), ids), (blank, K)
                assert _close(got["lp"].cpu().numpy().astype(np.float64), lp, LP_TOL), (blank, K)
                assert _close(got["lp_blank"].cpu().numpy().astype(np.float64), lpb, LP_TOL), (blank, K)
    lens = torch.tensor([4, 0], dtype=torch.int32, device=DEV)             # rows past the lengths are skipped: whatever was there stays
    got = ops.ctc_beam_cut(views[0], V1 - 1, 8, lens)
    ids, lp, _ = _cut_reference(xr, V1 - 1, 8)
    assert np.array_equal(got["ids"].cpu().numpy()[0, :4], ids[0, :4]) and _close(got["lp"].cpu().numpy().astype(np.float64)[0, :4], lp[0, :4], LP_TOL)


# ------------------------------------------------------------------------------------------------ 2. exhaustive regime
@functools.lru_cache(maxsize=None)
def exhaustive(T, V1):
    x = np.stack([small_logits(T, V1, s) for s in range(DRAWS)])
    want = [R.brute_force(R.log_softmax(x[s]), V1 - 1) for s in range(DRAWS)]
    return x, want, decode(x, V1 - 1, beams=64, token_topk=V1 - 1, nbest=8, return_frames=True)


@pytest.mark.parametrize("T,V1", SMALL)
def test_nothing_pruned_equals_the_enumeration(T, V1):
    x, want, out = exhaustive(T, V1)
    assert out["tokens"].shape == (DRAWS, 8, T) and out["tokens"].dtype == np.int64 and out["scores"].dtype == np.float32 and out["n_tokens"].dtype == np.int32
    kept = 0
    for s in range(DRAWS):
        top = want[s][:9]
        got = hyps_of(out, s)
        assert len(got) == min(8, len(want[s]))                            # the rows that exist, and only those
        if any(a[1] - b[1] < 2e-3 for a, b in zip(top, top[1:])):
            continue
        kept += 1
        assert [h[0] for h in got] == [w[0] for w in top[:8]], (s, got, top)
        for (labels, sc), (_, exact) in zip(got, top):
            print(f"T={T} V1={V1} draw {s}: {labels} device {sc:.6f} exact {exact:.6f}")
            assert abs(sc - exact) <= SCORE_TOL
    assert kept * 3 >= DRAWS * 2, kept


# ------------------------------------------------------------------------------------------------ 3. certified regime
CERT = dict(T=48, V1=40, W=8, K=8, nbest=8, draws=24)


@functools.lru_cache(maxsize=None)
def certified():
    c = CERT
    x = np.stack([R.peaky(s, c["T"], c["V1"], c["V1"] - 1) for s in range(c["draws"])])
    ref = [R.beam_search(x[s], c["V1"] - 1, c["W"], c["K"], nbest=c["nbest"]) for s in range(c["draws"])]
    return x, ref, decode(x, c["V1"] - 1, beams=c["W"], token_topk=c["K"], nbest=c["nbest"], return_frames=True)


def _match(got, ref, where):
    assert [h[0] for h in got] == [h[0] for h in ref["hyps"]], where
    for (labels, sc), (_, want, _) in zip(got, ref["hyps"]):
        print(f"{where}: {len(labels)} tokens, device {sc:.6f} float64 {want:.6f}")
        assert abs(sc - want) <= SCORE_TOL, where


def test_every_cut_certified_all_hypotheses_match():
    x, ref, out = certified()
    kept = [s for s in range(CERT["draws"]) if R.min_margin(ref[s]) >= 1e-3]
    assert len(kept) >= 8 and len(kept) * 3 >= CERT["draws"], kept
    for s in kept:
        got = hyps_of(out, s)
        assert len(got) == 8
        _match(got, ref[s], f"certified draw {s}")
        for r, (_, _, frames) in enumerate(ref[s]["hyps"]):                # the frame at which each token's prefix entered the beam
            assert out["frames"][s, r, :len(frames)].tolist() == frames


# ------------------------------------------------------------------------------------------------ 4. wide regime
WIDE = [(32, 300, 64, 24), (64, 300, 16, 20)]
WIDE_DRAWS = 8


@functools.lru_cache(maxsize=None)
def wide(T, V1, W, K):
    x = np.stack([R.peaky(100 + s, T, V1, V1 - 1) for s in range(WIDE_DRAWS)])
    ref, stable = [], []
    for s in range(WIDE_DRAWS):
        r = R.beam_search(x[s], V1 - 1, W, K, nbest=4)
        ok = len(r["hyps"]) == 4 and min(r["margins"]["final"]) >= 2e-3
        for j in range(2):                                                 # the same top 4 under two re-runs with 1e-4 Gaussian noise on the logits
            noisy = x[s] + np.random.default_rng(7000 + 2 * s + j).standard_normal(x[s].shape).astype(np.float32) * np.float32(1e-4)
            ok = ok and [h[0] for h in R.beam_search(noisy, V1 - 1, W, K, nbest=4)["hyps"]] == [h[0] for h in r["hyps"]]
        ref.append(r); stable.append(ok)
    return x, ref, stable, decode(x, V1 - 1, beams=W, token_topk=K, nbest=4)


@pytest.mark.parametrize("T,V1,W,K", WIDE)
def test_wide_beams_top4_match(T, V1, W, K):
    x, ref, stable, out = wide(T, V1, W, K)
    assert sum(stable) * 2 >= WIDE_DRAWS, stable
    for s in range(WIDE_DRAWS):
        if stable[s]:
            _match(hyps_of(out, s), ref[s], f"wide {(T, V1, W, K)} draw {s}")


# ------------------------------------------------------------------------------------------------ 5. lower bound
def test_scores_never_exceed_the_exact_log_probability():
    for T, V1 in SMALL:
        x, _, out = exhaustive(T, V1)
        for s in range(DRAWS):
            check_lower_bound(x[s], V1 - 1, hyps_of(out, s))
    x, _, out = certified()
    for s in range(CERT["draws"]):
        check_lower_bound(x[s], CERT["V1"] - 1, hyps_of(out, s))
    for c in WIDE:
        x, _, _, out = wide(*c)
        for s in range(WIDE_DRAWS):
            check_lower_bound(x[s], c[1] - 1, hyps_of(out, s))


# ------------------------------------------------------------------------------------------------ 6. batch and lengths
def test_batch_independence_lengths_bf16_and_reproducibility():
    from huggingface_asr_amd import ops
    T, V1, W, K = 48, 40, 8, 8
    lengths = [T, T - 7, 1, 0, T]
    x = torch.from_numpy(np.stack([R.peaky(300 + b, T, V1, V1 - 1) for b in range(5)])).to(torch.bfloat16)          # values both dtypes hold exactly
    xf, xb = x.float().to(DEV), x.to(DEV)
    lens = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    kw = dict(beams=W, token_topk=K, nbest=4, return_frames=True)
    out = ops.ctc_beam_decode(xf, V1 - 1, PAD, lens, **kw)
    again = ops.ctc_beam_decode(xf, V1 - 1, PAD, lens, **kw)
    half = ops.ctc_beam_decode(xb, V1 - 1, PAD, lens, **kw)
    i32 = ops.ctc_beam_decode(xf, V1 - 1, PAD, lens, dtype=torch.int32, **kw)
    for k in ("tokens", "n_tokens", "scores", "frames"):
        assert torch.equal(out[k], again[k]), k                            # two runs: the same bits
        assert torch.equal(out[k], half[k]), k                             # bf16 logits: the bits of fp32 logits holding the same values
    assert i32["tokens"].dtype == torch.int32 and torch.equal(i32["tokens"].long(), out["tokens"]) and torch.equal(i32["scores"], out["scores"])
    for b, n in enumerate(lengths):
        one = ops.ctc_beam_decode(xf[b:b + 1, :max(n, 1)].contiguous(), V1 - 1, PAD, None if n else lens[b:b + 1], **kw)
        m = max(n, 1)
        assert torch.equal(one["scores"][0], out["scores"][b]) and torch.equal(one["n_tokens"][0], out["n_tokens"][b]), b
        assert torch.equal(one["tokens"][0, :, :m], out["tokens"][b, :, :m]) and (out["tokens"][b, :, m:] == PAD).all(), b
        assert torch.equal(one["frames"][0, :, :m], out["frames"][b, :, :m]) and (out["frames"][b, :, m:] == -1).all(), b
        assert int(out["n_tokens"][b].max()) <= n
    o = {k: v.cpu().numpy() for k, v in out.items()}
    assert hyps_of(o, 3) == [((), 0.0)]                                    # no frames: the empty hypothesis with score 0, nothing else
    assert len(hyps_of(o, 2)) == 4 and len(hyps_of(o, 0)) == 4
    for b in (0, 1, 2, 4):                                                 # (bf16-rounded logits tie too often for a hypothesis-by-hypothesis comparison: the bound only)
        check_lower_bound(x[b].float().numpy(), V1 - 1, hyps_of(o, b), lengths[b])


# ------------------------------------------------------------------------------------------------ 7. long utterance
def test_long_utterance_equals_greedy_when_one_class_dominates():
    from huggingface_asr_amd import ops
    T, V1 = 1030, 40
    g = np.random.default_rng(77)
    x = g.standard_normal((2, T, V1)).astype(np.float32)
    for b in range(2):
        t = 0
        while t < T:
            run = int(g.integers(1, 4))
            x[b, t:t + run, int(g.integers(0, V1))] += 30.0                # runs of one class (the blank among them) 30 above the noise
            t += run
    xd = torch.from_numpy(x).to(DEV)
    lens = torch.tensor([T, T - 3], dtype=torch.int32, device=DEV)
    out = ops.ctc_beam_decode(xd, V1 - 1, PAD, lens, beams=64, nbest=2, return_frames=True)
    want = ops.ctc_greedy_decode(xd, V1 - 1, PAD, lens, return_frames=True)
    assert torch.equal(out["tokens"][:, 0], want["tokens"]) and torch.equal(out["n_tokens"][:, 0], want["n_tokens"])
    assert int(want["n_tokens"].min()) > 200
    for b in range(2):
        n, nb = int(out["n_tokens"][b, 0]), int(lens[b])
        fr = out["frames"][b, 0].cpu().numpy()
        assert (np.diff(fr[:n]) > 0).all() and fr[0] >= 0 and fr[n - 1] < nb and (fr[n:] == -1).all()
        assert (fr[:n] <= want["frames"][b, :n].cpu().numpy()).all()       # a prefix is in the beam no later than the frame its last token starts at (64 beams hold it earlier, as a poor candidate)
    assert (out["scores"][:, 0] > out["scores"][:, 1]).all() and (out["scores"][:, 0] > -1e-3).all()


# ------------------------------------------------------------------------------------------------ 8. engine
@pytest.mark.parametrize("span", ["valid", "all"])
def test_engine_transcribe_with_beams(span):
    from helpers import case_inputs, load_golden
    from huggingface_asr_amd import ops, shapes
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg = dict(shapes.TINY)
    cfg.update(ctc_zero_infinity=True, ctc_loss_reduction="mean")
    sd, x, am, _ = case_inputs(load_golden("tiny_rel"), cfg)
    eng = EBranchformerEngine(cfg, DEV)
    eng.load_state_dict(sd)
    xd, lens = x.to(DEV), am.sum(-1).to(DEV, torch.int32)
    V1, pad = cfg["vocab_size"] + 1, 3
    fwd = eng.forward(xd, lens)
    ln = fwd["outer_len"] if span == "valid" else None
    want = ops.ctc_beam_decode(fwd["logits"], V1 - 1, pad, ln, beams=8, nbest=4, return_frames=True)
    got = eng.transcribe(xd, lens, span=span, pad_id=pad, beams=8, nbest=4, return_frames=True, want_hidden=True)
    for a, b in (("nbest_tokens", "tokens"), ("nbest_n", "n_tokens"), ("scores", "scores"), ("nbest_frames", "frames")):
        assert torch.equal(got[a], want[b]), a
    assert torch.equal(got["tokens"], want["tokens"][:, 0]) and torch.equal(got["n_tokens"], want["n_tokens"][:, 0]) and torch.equal(got["frames"], want["frames"][:, 0])
    assert torch.equal(got["outer_len"], fwd["outer_len"]) and torch.equal(got["last_hidden"], fwd["last_hidden"]) and "best" not in got
    assert torch.isfinite(got["scores"]).all() and got["nbest_tokens"].shape == (xd.shape[0], 4, fwd["logits"].shape[1])
    plain = eng.transcribe(xd, lens, span=span, pad_id=pad, return_frames=True)          # without beams: the greedy path, as before
    ref = ops.ctc_greedy_decode(fwd["logits"], V1 - 1, pad, ln, return_frames=True)
    assert all(torch.equal(plain[k], ref[k]) for k in ("best", "tokens", "n_tokens", "frames")) and "scores" not in plain


# ------------------------------------------------------------------------------------------------ 9. the drop-in
def test_drop_in_returns_the_padded_best_hypotheses():
    from huggingface_asr_amd import decoding, ops

    class Tok:
        pad_token_id = 41
    x, _, _ = certified()
    V1 = CERT["V1"]
    xd = torch.from_numpy(x).to(DEV)
    got = decoding.ctc_beam_decode(xd, None, Tok(), 5)
    full = ops.ctc_beam_decode(xd, V1 - 1, 41, beams=5)
    L = int(full["n_tokens"].max())
    assert got.dtype == torch.int64 and got.device == xd.device and got.shape == (x.shape[0], L) and torch.equal(got, full["tokens"][:, 0, :L])
    kept = 0
    for s in range(x.shape[0]):
        ref = R.beam_search(x[s], V1 - 1, 5, nbest=1)                      # token_topk = min(5, V): what the reference's call passes
        if R.min_margin(ref) >= 1e-3:
            kept += 1
            labels = ref["hyps"][0][0]
            assert got[s, :len(labels)].tolist() == list(labels) and (got[s, len(labels):] == 41).all(), s
    assert kept >= 8, kept
