"""GPU: shallow-fusion LM rescoring on the HIP path (reference src/decoding/shallow_fussion.py; src/models/ctc_encoder_plus_autoregressive_decoder.py:398-403).
  1. the token step without cross-attention (`mi_gpt2_step` with cross_kv == NULL, every form) against transformers' fp32 `GPT2LMHeadModel`, teacher-forced;
  2. its fused two-launches-per-layer form against the launch-per-op form;
  3. `mi_beam_step_lm` against a host restatement of its arithmetic fed through the pinned loop (oracle/generate_ref.py);
  4. `decoder.generate(..., lm=, lm_weight=0.5)` against the reference's OWN generate() with its LM processor (fixture tests/golden/gen_tiny_lm.npz), by the three-step
     certification of tests/test_gpu_generate.py;
  5. the device loop and the host loop with the LM: identical hypotheses and scores;
  6. `model.generate` with `lm_model` / `lm_weight` in a GenerationConfigCustom, the `do_generate` call sequence."""
import numpy as np
import pytest
import torch

import gen_model as GM
import lm_model as LM
from helpers import AED_JCFG, gen_case_inputs, load_golden
from huggingface_asr_amd import shapes
from oracle import generate_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENC = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")
# tests/test_gpu_generate.py's TOL (a sum of <= 13 log-probabilities through the bf16 path against fp32) plus the same for the LM's share, scaled by its weight
TOL = 0.06 * (1 + LM.LM_WEIGHT)


def _lm_engine(lm, form=0):
    from huggingface_asr_amd.decoder import GPT2LMEngine, lm_cfg_dict
    eng = GPT2LMEngine(lm_cfg_dict(lm.config), DEV)
    eng.load_state_dict(lm.state_dict())
    eng._gcfg.step_form = form
    return eng


def _prefixes(rows, n, V):
    return torch.from_numpy(np.stack([np.concatenate([[2], 7 + (np.arange(n - 1) * (37 + 11 * r) + 101 * r) % (V - 7)]) for r in range(rows)])).long()


# (d, heads, vocabulary, rows, step form, new tokens of the first step): the fused form (<= 8 rows, d <= 512, head size 64), the general form (more than 8 rows), the
# GEMV form (form 1 at <= 8 rows, 4 d <= 2048), the streaming form (2), a size outside the fused and GEMV forms (launch per op on the MFMA kernels), a prompt step
STEP_CASES = [(128, 2, 51, 1, 0, 1), (128, 2, 51, 5, 0, 1), (128, 2, 51, 8, 0, 1), (128, 2, 51, 10, 0, 1), (128, 2, 51, 5, 1, 1), (128, 2, 51, 5, 2, 1),
              (768, 12, 5001, 5, 0, 1), (128, 2, 51, 5, 1, 4)]


@pytest.mark.parametrize("d,H,V,rows,form,U0", STEP_CASES)
def test_token_step_without_cross_attention_against_transformers(d, H, V, rows, form, U0):
    """7 steps, a different prefix in every row: the KV-cached HIP step's logits against transformers' GPT2LMHeadModel (CPU, fp32) run over the whole prefix — what the
    reference's processor does for every token.  Tolerance: tests/test_gpu_config5.py `test_token_step_logits_at_decred_base_size`'s."""
    torch.set_num_threads(8)
    lm = LM.random_lm(5, d, 2, H, V)
    n = U0 + 6
    ids = _prefixes(rows, n, V)
    with torch.no_grad():
        want = lm(ids).logits.float()[:, U0 - 1:]                       # (rows, 7, V)
    eng = _lm_engine(lm, form)
    cache = eng.init_cache(rows, 16)
    dev_ids = ids.to(DEV)
    got = [eng.step(dev_ids[:, :U0], cache)] + [eng.step(dev_ids[:, u:u + 1], cache) for u in range(U0, n)]
    got = torch.stack(got, 1).float().cpu()
    assert cache["past"] == n and torch.isfinite(got).all()
    std = float(want.std())
    err = (got - want).abs()
    print(f"cross-less step d={d} rows={rows} form={form} U0={U0}: max |dlogit| {float(err.max()):.4f} mean {float(err.mean()):.5f} std {std:.3f}")
    assert float(err.max()) < 0.06 * max(std, 1.0) + 0.03 and float(err.mean()) < 0.01 * max(std, 1.0), (float(err.max()), float(err.mean()), std)
    top2 = want.topk(2, -1).values
    clear = (top2[..., 0] - top2[..., 1]) > 0.1
    assert int(clear.sum()) >= 1 and bool((got.argmax(-1)[clear] == want.argmax(-1)[clear]).all())


@pytest.mark.parametrize("d", [128, 512])
@pytest.mark.parametrize("rows", [1, 5, 8])
def test_fused_two_launch_step_against_the_launch_per_op_step(d, rows):
    """Without cross-attention the fused form runs TWO launches per layer (csrc/decoder_fused.hip: the MLP launch's prologue sums the self-attention launch's per-head
    partials).  20 steps with a cache re-order half way against step_form 1; bounds of tests/test_gpu_config5.py `test_fused_token_step_against_the_launch_per_op_step`;
    and the fused form is bit-reproducible (fixed summation order, no atomics)."""
    lm = LM.random_lm(7, d, 2, d // 64, 51)
    ids = _prefixes(rows, 21, 51).to(DEV)
    fa, fb, fc = _lm_engine(lm, 0), _lm_engine(lm, 1), _lm_engine(lm, 0)
    ca, cb, cc = fa.init_cache(rows, 32), fb.init_cache(rows, 32), fc.init_cache(rows, 32)
    perm = torch.tensor([(r * 3 + 1) % rows for r in range(rows)], device=DEV)
    worst = 0.0
    for u in range(20):
        a, b, c = fa.step(ids[:, u:u + 1], ca), fb.step(ids[:, u:u + 1], cb), fc.step(ids[:, u:u + 1], cc)
        assert torch.isfinite(a).all() and torch.equal(a, c), u
        worst = max(worst, float((a - b).abs().max()))
        assert float((a - b).abs().max()) < 2e-2 and float((a - b).abs().mean()) < 2e-3, (u, float((a - b).abs().max()), float((a - b).abs().mean()), float(b.std()))
        if u == 9:
            for e, ch in ((fa, ca), (fb, cb), (fc, cc)):
                e.reorder_cache(ch, perm)
    for l in range(len(ca["k"])):
        for t in ("k", "v"):
            xa, xb = ca[t][l][:, :20].float(), cb[t][l][:, :20].float()
            assert torch.equal(ca[t][l][:, :20], cc[t][l][:, :20])
            assert float((xa - xb).abs().max()) <= 0.02 * float(xb.abs().max()) and float((xa - xb).abs().mean()) < 1e-3 * float(xb.abs().max())
    print(f"fused two-launch vs launch-per-op LM step, d = {d}, rows = {rows}: max |dlogit| over 20 steps {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------- 3. the beam kernel
def _beam_step_lm(st, logits, lse, ctc, w, lm_logits, lm_lse, w_lm, pad, eos, B, W, V, cur, max_length, lp, es, entry="mi_beam_step_lm"):
    from huggingface_asr_amd import _lib
    from huggingface_asr_amd.decoder import _ES_MODE, _step_denoms
    n, Lmax = B * W, st["ids"].shape[1]
    new_tok, beam_idx = torch.empty(n, dtype=torch.long, device=DEV), torch.empty(n, dtype=torch.long, device=DEV)
    top_s, top_i = torch.empty(B, 2 * W, device=DEV), torch.empty(B, 2 * W, dtype=torch.int32, device=DEV)
    denom, heur = _step_denoms(cur, max_length, lp, es)
    args = [logits.data_ptr(), logits.stride(0), lse.data_ptr(), ctc.data_ptr() if ctc is not None else None, float(1 - w), float(w), int(ctc is not None), pad, eos, B, W, V,
            cur, max_length, Lmax, denom, heur, _ES_MODE[es], st["ids"].data_ptr(), st["bs"].data_ptr(), new_tok.data_ptr(), beam_idx.data_ptr(), st["done"].data_ptr(),
            st["nfin"].data_ptr(), st["fs"].data_ptr(), st["fl"].data_ptr(), st["ft"].data_ptr(), top_s.data_ptr(), top_i.data_ptr(), None]
    if entry == "mi_beam_step_lm":
        args += [lm_logits.data_ptr() if lm_logits is not None else None, lm_logits.stride(0) if lm_logits is not None else 0,
                 lm_lse.data_ptr() if lm_lse is not None else None, float(w_lm)]
    _lib.check(getattr(_lib.lib(), entry)(*args, torch.cuda.current_stream().cuda_stream), entry)
    return new_tok, beam_idx, top_s, top_i


def _padded(t, V):
    buf = torch.zeros(t.shape[0], (V + 7) // 8 * 8)
    buf[:, :V] = t
    return buf.to(DEV)[:, :V]


def _follow_the_pinned_loop_with_lm(B, W, V, with_ctc, lp, es, ties=False, minus_inf=False):
    """A whole decode (max_length 11) through mi_beam_step_lm and through the pinned CPU loop on the same processed scores — the kernel's arithmetic restated on the host,
    one rounding per operation: s = logit - lse; pad -> logzero and s = (1 - w) s + w ctc with CTC; l = lm - lm_lse; m = w_lm l; s = s + m.  Candidates (values and
    indices) of every open utterance at every step, kept hypotheses, scores and order must agree exactly.  `ties`: every stream on a coarse grid; `minus_inf`: at steps 1
    and 2 the LM gives one utterance -inf everywhere but one token per beam.  -> (steps x utterances with fewer than 2W finite candidates, with equal values in the top 2W)"""
    from test_gpu_aed import _beam_state, _step_scores
    gen = torch.Generator().manual_seed(B * 1000 + W * 10 + V + 7 * ties + 13 * minus_inf + 1)
    pad, eos, max_length = V - 1, 1, 11
    steps, Lmax, w, w_lm = max_length - 1, max_length + 1, 0.3, 0.5
    n = B * W
    st = _beam_state(B, W, pad, Lmax)
    processed, tops = [], []
    for t in range(steps):
        cur = t + 1
        lg, ctc = _step_scores(gen, t, n, V, eos, with_ctc, ties, 5.0 if V > 1000 else 3.0)
        lm = torch.randn(n, V, generator=gen) * 2.0
        lm[:, eos] += 2.0 if t >= 1 else -5.0
        if ties:
            lm = lm.round().clamp(max=1)
        if minus_inf and t in (1, 2):
            b = (t - 1) % B
            keep = torch.zeros(W, V, dtype=torch.bool)
            keep[torch.arange(W), 3 + 7 * torch.arange(W)] = True        # one finite LM logit per beam, none of them EOS or pad: W finite candidates, fewer than 2W
            lm[b * W:(b + 1) * W][~keep] = -float("inf")
        lse, lm_lse = torch.logsumexp(lg, 1).float(), torch.logsumexp(lm, 1).float()        # inputs of the kernel: the same ones for kernel and host
        sc = (lg - lse[:, None]).numpy()
        if with_ctc:
            sc[:, pad] = np.float32(-10000000000.0)
            sc = np.float32(1 - w) * sc + np.float32(w) * ctc.numpy()
        l = (lm - lm_lse[:, None]).numpy()
        m = np.float32(w_lm) * l
        sc = sc + m
        processed.append(sc.astype(np.float32))
        was_done = st["done"].cpu().bool().numpy()
        _, _, top_s, top_i = _beam_step_lm(st, _padded(lg, V), lse.to(DEV), ctc.to(DEV) if with_ctc else None, w, _padded(lm, V), lm_lse.to(DEV), w_lm, pad, eos, B, W, V, cur,
                                           max_length, lp, es)
        tops.append((top_s.cpu().numpy(), top_i.cpu().numpy().astype(np.int64), was_done))
    calls = []

    def score_fn(rows):
        calls.append(rows.copy())
        return processed[len(calls) - 1]
    tr = {}
    seq, scores = G.beam_search(score_fn, B, W, V, max_length=max_length, eos=eos, pad=pad, start=2, length_penalty=lp, early_stopping=es, trace=tr)
    fs, fl, ft, nf = st["fs"].cpu().numpy(), st["fl"].cpu().numpy(), st["ft"].cpu().numpy(), st["nfin"].cpu().numpy()
    assert (nf == W).all() and bool(st["done"].cpu().all())
    for b in range(B):
        for k in range(W):
            want = seq[b * W + k]
            n_tok = int(fl[b, k])
            assert ft[b, k, :n_tok].tolist() == want[:n_tok].tolist() and (want[n_tok:] == pad).all(), (b, k, ft[b, k], want)
            assert fs[b, k] == scores[b * W + k], (b, k, fs[b, k], scores[b * W + k])
    few = tied = 0
    for t, (ts, ti, was_done) in enumerate(tops):
        if t < len(calls):
            ov, oi = tr["cands"][t]
            assert (tr["open"][t] == ~was_done).all(), (t, tr["open"][t], was_done)
            for b in np.nonzero(~was_done)[0]:
                assert ti[b].tolist() == oi[b].tolist() and ts[b].tolist() == ov[b].tolist(), (t, b, ts[b], ti[b], ov[b], oi[b])
                few += int(np.isfinite(tr["acc"][t][b]).sum() < 2 * W)
                tied += int((ov[b][:-1] == ov[b][1:]).any())
    assert len(calls) >= 3
    return few, tied


@pytest.mark.parametrize("es", [False, "never"])
@pytest.mark.parametrize("lp", [1.0, 1.6])
@pytest.mark.parametrize("with_ctc", [True, False])
@pytest.mark.parametrize("B,W,V", [(2, 1, 51), (2, 5, 51), (1, 5, 5001), (1, 8, 5001)])
def test_beam_step_lm_follows_the_pinned_loop(B, W, V, with_ctc, lp, es):
    """(1, 8, 5001): 8 * 5001 > 32 Ki candidates, the uncached pass; the others the register-cached pass in its two-half LM form (one, two and four groups of eight)."""
    _follow_the_pinned_loop_with_lm(B, W, V, with_ctc, lp, es)


@pytest.mark.parametrize("B,W,V", [(2, 4, 4096), (2, 5, 51), (1, 8, 5001)])
@pytest.mark.parametrize("kind", ["ties", "minus_inf"])
def test_beam_step_lm_ranks_ties_and_minus_inf_lm_logits_in_index_order(B, W, V, kind):
    few, tied = _follow_the_pinned_loop_with_lm(B, W, V, True, 1.0, False, ties=kind == "ties", minus_inf=kind == "minus_inf")
    if kind == "minus_inf":
        assert few >= 1, few                                      # the case did reach an open utterance with fewer than 2W finite candidates
    else:
        assert tied >= 1, tied                                    # ... and equal values inside the top 2W


@pytest.mark.parametrize("B,W,V", [(2, 5, 51), (1, 8, 5001)])
def test_beam_step_lm_without_an_lm_is_mi_beam_step(B, W, V):
    """lm_logits == NULL: the new entry launches the LM-off instantiation — the same bits as mi_beam_step in every output, step after step"""
    from test_gpu_aed import _beam_state, _step_scores
    gen = torch.Generator().manual_seed(99 + V)
    pad, eos, max_length = V - 1, 1, 8
    sa, sb = _beam_state(B, W, pad, max_length + 1), _beam_state(B, W, pad, max_length + 1)
    for t in range(max_length - 1):
        lg, ctc = _step_scores(gen, t, B * W, V, eos, True, False, 4.0)
        lse = torch.logsumexp(lg, 1).float().to(DEV)
        lgd, ctcd = _padded(lg, V), ctc.to(DEV)
        ra = _beam_step_lm(sa, lgd, lse, ctcd, 0.3, None, None, 0.0, pad, eos, B, W, V, t + 1, max_length, 1.0, False, entry="mi_beam_step")
        rb = _beam_step_lm(sb, lgd, lse, ctcd, 0.3, None, None, 0.7, pad, eos, B, W, V, t + 1, max_length, 1.0, False)
        for x, y in zip(ra, rb):
            assert torch.equal(x, y), t
        for k in sa:
            assert torch.equal(sa[k], sb[k]), (t, k)
    assert bool(sa["done"].cpu().all())


# ---------------------------------------------------------------------------------------------------------------- 4-6. decoding
def _engine(sd, dec_cfg):
    from huggingface_asr_amd.decoder import JointAEDEngine
    eng = JointAEDEngine(ENC, dec_cfg, AED_JCFG, DEV)
    eng.load_state_dict(sd)
    return eng


def _score_fn(sd, dec_cfg, x, am, W, cw, lm):
    """the reference's processed scores with the LM appended; greedy without the CTC processor adds the LM term to raw logits there — the device normalises the row
    first, which moves every candidate of the row by the same amount: compared in the normalised form"""
    fn, B = G.joint_score_fn(sd, ENC, dec_cfg, AED_JCFG, x, am, W, cw)
    if W == 1 and not cw > 0:
        raw = fn
        fn = lambda ids: torch.log_softmax(torch.from_numpy(np.asarray(raw(ids), np.float32)), -1).numpy()
    return LM.with_lm(fn, lm, LM.LM_WEIGHT), B


def certified_decode_lm(eng, lm_eng, lm, sd, dec_cfg, x, am, W, lp, es, ml, cw, tol=TOL):
    """tests/test_gpu_generate.py `certified_decode` with the LM passed to the device loop and appended to the oracle's score function: 1. the device's bookkeeping is
    exact (its candidates replayed through the pinned loop give its hypotheses, scores and order), 2. its candidate values are the fp32 oracle's within `tol`, 3. along
    the reference's trajectory the decisions are the reference's up to one its own numbers certify as a near tie (< 2 tol)."""
    from huggingface_asr_amd.decoder import generate
    V, pad, start, eos = GM.V, GM.PAD, GM.START, GM.EOS
    B = x.shape[0]
    tr = []
    got = generate(eng, x.to(DEV), am.sum(-1).to(DEV, torch.int32), num_beams=W, max_length=ml, ctc_weight=cw, length_penalty=lp, early_stopping=es, eos_token_id=eos, trace=tr,
                   lm=lm_eng, lm_weight=LM.LM_WEIGHT)
    dev = [(s.cpu().numpy(), i.cpu().numpy().astype(np.int64), d.cpu().numpy().astype(bool)) for s, i, d in tr]
    fn, _ = _score_fn(sd, dec_cfg, x, am, W, cw, lm)
    free = {}
    ref_seq, ref_sc = G.beam_search(fn, B, W, V, max_length=ml, eos=eos, pad=pad, start=start, length_penalty=lp, early_stopping=es, trace=free)
    fn2, _ = _score_fn(sd, dec_cfg, x, am, W, cw, lm)

    def cand_fn(step, running, open_):
        if step < len(dev):
            s, i, was_done = dev[step]
            assert (open_ == ~was_done).all(), (step, open_, was_done)
            return s, i
        return np.zeros((B, 2 * W), np.float32), np.zeros((B, 2 * W), np.int64)
    rep = {}
    rep_seq, rep_sc = G.beam_search(fn2, B, W, V, max_length=ml, eos=eos, pad=pad, start=start, length_penalty=lp, early_stopping=es, trace=rep, cand_fn=cand_fn)
    for b in range(B):
        hyps = got[b]["hypotheses"]
        assert len(hyps) == W
        for k, (s, toks) in enumerate(hyps):
            want = rep_seq[b * W + k]
            assert toks == want[: len(toks)].tolist() and (want[len(toks):] == pad).all(), ("bookkeeping", b, k, toks, want)
            assert abs(s - float(rep_sc[b * W + k])) < 1e-6 * max(1.0, abs(s)), ("bookkeeping score", b, k, s, rep_sc[b * W + k])
    worst = 0.0
    for t, (s, i, was_done) in enumerate(dev[: len(rep["acc"])]):
        acc = rep["acc"][t]
        for b in range(B):
            if was_done[b] or not rep["open"][t][b]:
                continue
            own = np.sort(acc[b])[::-1][: 2 * W]
            d_rank = np.abs(own - s[b]).max()
            d_cand = np.abs(acc[b][i[b]] - s[b]).max()
            worst = max(worst, float(d_rank), float(d_cand))
            assert d_rank < tol and d_cand < tol, ("candidate values", t, b, d_rank, d_cand)
    diverged = [False] * B
    for t in range(min(len(dev), len(free["cands"]))):
        fv, fi = free["cands"][t]
        s, i, was_done = dev[t]
        for b in range(B):
            if diverged[b] or was_done[b] or not free["open"][t][b]:
                continue
            assert (free["running"][t][b] == rep["running"][t][b]).all()
            if (fi[b] == i[b]).all():
                continue
            r = int(np.argmax(fi[b] != i[b]))
            acc_ref = free["acc"][t][b]
            gap = abs(float(acc_ref[fi[b, r]]) - float(acc_ref[i[b, r]]))
            assert gap < 2 * tol, ("decision differs from the reference outside a near tie", t, b, r, gap)
            diverged[b] = True
    for b in range(B):
        dev_h = got[b]["hypotheses"]
        if not diverged[b]:
            for k in range(W):
                want = ref_seq[b * W + k]
                toks = dev_h[k][1]
                assert toks == want[: len(toks)].tolist() and (want[len(toks):] == pad).all(), ("tokens", b, k, toks, want)
                assert abs(dev_h[k][0] - float(ref_sc[b * W + k])) < tol, ("score", b, k, dev_h[k][0], ref_sc[b * W + k])
        else:
            assert dev_h[0][0] >= float(ref_sc[b * W]) - tol, ("after a near tie the best hypothesis is worse than the reference's", b, dev_h[0], ref_sc[b * W])
    return got, (ref_seq, ref_sc), diverged, worst


def test_hip_generate_with_the_lm_against_the_reference_generate():
    from huggingface_asr_amd.decoder import lm_engine_for
    torch.set_num_threads(8)
    _, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    g = load_golden("gen_tiny_lm")
    eng = _engine(sd, dec_cfg)
    lm = LM.tiny_lm()
    lm_eng = lm_engine_for(lm, DEV)
    assert lm_engine_for(lm, DEV) is lm_eng                          # one engine per LM module
    exact = total = 0
    for W, lp, es, ml, cw in LM.SETTINGS:
        key = LM.setting_key(W, lp, es, ml, cw)
        got, (ref_seq, ref_sc), diverged, worst = certified_decode_lm(eng, lm_eng, lm, sd, dec_cfg, x, am, W, lp, es, ml, cw)
        print(f"{key}: worst candidate-value difference {worst:.4f} (tol {TOL}), diverged {diverged}")
        want = g[key + "/sequences"]
        if W > 1:                                                    # the trajectory followed IS the reference's (also asserted on the CPU, tests/test_lm_fusion_cpu.py)
            assert ref_seq.shape == want.shape and (ref_seq == want).all() and np.abs(ref_sc - g[key + "/sequences_scores"]).max() < 1e-5
        for b in range(x.shape[0]):
            total += 1
            if not diverged[b]:
                exact += 1
                for k in range(W):
                    row = want[b * W + k] if W > 1 else want[b]
                    toks = got[b]["hypotheses"][k][1]
                    n = len(toks)
                    assert toks == row[:n].tolist() and (row[n:] == GM.PAD).all(), (key, b, k, toks, row)
        if W == 1:
            assert float(g[key + "/min_margin"]) > 2 * TOL and not any(diverged), key
    print(f"gen_tiny + LM: {exact} of {total} utterance decodes equal the reference's token for token; the rest diverge at a certified near tie")
    assert 2 * exact >= total


@pytest.mark.parametrize("W,cw,trick", [(1, 0.0, False), (1, 0.3, False), (3, 0.0, False), (3, 0.3, False), (3, 0.3, True)])
def test_device_loop_and_host_loop_agree_with_the_lm(W, cw, trick):
    """Same arithmetic, operation for operation: identical hypotheses and scores.  With the eos / space trick `generate` routes to the host loop (and carries the LM along)."""
    from huggingface_asr_amd.decoder import generate, generate_stepwise, lm_engine_for
    _, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    eng = _engine(sd, dec_cfg)
    lm = LM.tiny_lm()
    lm_eng = lm_engine_for(lm, DEV)
    fl = am.sum(-1).to(DEV, torch.int32)
    kw = dict(num_beams=W, max_length=12, ctc_weight=cw, eos_token_id=GM.EOS, lm=lm_eng, lm_weight=LM.LM_WEIGHT)
    if trick:
        kw.update(space_token_id=20, apply_eos_space_trick=True, eos_space_trick_weight=0.5)
    a = generate(eng, x.to(DEV), fl, **kw)
    b = generate_stepwise(eng, x.to(DEV), fl, **kw)
    assert [h["hypotheses"] for h in a] == [h["hypotheses"] for h in b]
    if not trick:
        c = generate(eng, x.to(DEV), fl, lm_side_stream=True, **kw)      # the LM step on its own stream: the same results
        assert [h["hypotheses"] for h in a] == [h["hypotheses"] for h in c]
        plain = generate(eng, x.to(DEV), fl, **dict(kw, lm=None))
        assert [h["hypotheses"] for h in a] != [h["hypotheses"] for h in plain]          # the LM term is in


def test_model_generate_with_lm_model_follows_the_do_generate_call_sequence():
    """`do_generate` (general_utils.py:198-218) with the trainer's GenerationConfigCustom carrying `lm_model` / `lm_weight` (train_enc_dec_asr.py:72-73):
    `.sequences` / `.sequences_scores` are the engine-level result; the configuration keeps the SAME module and its engine is built once; `lm_weight=0` returns exactly what
    the call without an LM returns."""
    from test_surface_cpu import _joint_model
    from huggingface_asr_amd.decoder import generate, lm_engine_for
    from huggingface_asr_amd.decoding import GenerationConfigCustom
    g, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    model = _joint_model(False)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected
    model = model.to(DEV).eval()
    lm = LM.tiny_lm()                                                # stays on the CPU: the engine's load copies its parameters to the inputs' device
    W, lp, es, ml = 5, 1.0, False, 14
    gen_config = GenerationConfigCustom(bos_token_id=GM.START, pad_token_id=GM.PAD, decoder_start_token_id=GM.START, length_penalty=lp, early_stopping=es,
                                        eos_token_id=GM.EOS, max_length=ml, num_beams=W, ctc_weight=0.3, ctc_margin=0, lm_weight=LM.LM_WEIGHT, lm_model=lm, space_token_id=-1,
                                        apply_eos_space_trick=False, eos_space_trick_weight=1.0)
    model.generation_config = gen_config
    gen_config.num_return_sequences, gen_config.return_dict_in_generate, gen_config.output_scores = W, True, True
    sample = dict(input_values=x.to(DEV), attention_mask=am.to(DEV), labels=torch.tensor([[5, 6, 7], [8, 9, -100]], device=DEV))
    out = model.generate(generation_config=gen_config, **sample)
    assert gen_config.lm_model is lm
    lm_eng = lm.__dict__["_hfasr_lm_engine"][1]
    out2 = model.generate(generation_config=gen_config, **sample)
    assert lm.__dict__["_hfasr_lm_engine"][1] is lm_eng and torch.equal(out.sequences, out2.sequences) and torch.equal(out.sequences_scores, out2.sequences_scores)
    ref = generate(model._get_engine(DEV), x.to(DEV), am.sum(-1).to(DEV, torch.int32), num_beams=W, max_length=ml, ctc_weight=0.3, length_penalty=lp, eos_token_id=GM.EOS,
                   lm=lm_engine_for(lm, DEV), lm_weight=LM.LM_WEIGHT)
    B = x.shape[0]
    assert out.sequences.shape[0] == B * W and out.sequences_scores.shape == (B * W,)
    for b in range(B):
        for k in range(W):
            s, toks = ref[b]["hypotheses"][k]
            row = out.sequences[b * W + k].tolist()
            assert row[: len(toks)] == toks and all(v == GM.PAD for v in row[len(toks):])
            assert float(out.sequences_scores[b * W + k]) == pytest.approx(s, abs=1e-6)
    # the keyword form overrides the configuration; weight 0 switches the term off: the call without an LM
    off = model.generate(generation_config=gen_config, lm_weight=0, **sample)
    gen_config.lm_weight, gen_config.lm_model = 0, None
    plain = model.generate(generation_config=gen_config, **sample)
    assert torch.equal(off.sequences, plain.sequences) and torch.equal(off.sequences_scores, plain.sequences_scores)
    assert out.sequences.shape != plain.sequences.shape or not torch.equal(out.sequences, plain.sequences)          # the LM term was in
    kwform = model.generate(generation_config=gen_config, lm_weight=LM.LM_WEIGHT, lm_model=lm, **sample)
    assert torch.equal(kwform.sequences, out.sequences) and torch.equal(kwform.sequences_scores, out.sequences_scores)
