"""GPU: two-pass joint decoding (csrc/rescore.hip, GPT2DecoderEngine.token_nll, decoder.rescore / decoder.score, the model surface) against tests/rescore_ref.py.

  1. mi_rescore_pack, exact, at its edges (the empty hypothesis, k = U - 1, k = U, a token outside the vocabulary, a non-finite score; int32 and int64 tokens);
  2. mi_rescore_select bit for bit against `select32` (planted equal totals, -inf rows, an utterance without a hypothesis), every case twice with equal bits;
  3. token_nll on the aed_tiny decoder: fp32 within 1e-3 of the oracle (SURVEY §7 tier (i)), bf16 within 0.06 (tests/test_gpu_generate.py's TOL) of the nll taken in
     fp32 from the same engine's forward() logits; ignored positions exactly 0; the ids past a hypothesis' end do not reach its valid positions' bits;
  4. the CTC term of score() against the beam search's own scores where nothing is pruned;
  5. end to end on the gen_tiny model (tests/rescore_cases.py): order, totals, att and ctc are `select32` of the device's own n-best, nll and CTC scores, bit for bit;
     in fp32 precision the top-1 is the CPU oracle's wherever the oracle's gap between ranks 1 and 2 exceeds 5e-3;
  6. the model surface: return layouts, score() of rescore()'s output, the HFASR_JOINT_RESCORE route of generate(), JointAEDEngine.transcribe / .align.
"""
import functools

import numpy as np
import pytest
import torch

import gen_model as GM
import rescore_cases as RC
import rescore_ref as RR
from helpers import AED_JCFG, TINY_DEC, aed_case_inputs, load_golden
from test_rescore_cpu import EOS, PAD, START, pack_edge_case, random_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32_BAR = 1e-3          # SURVEY §7 tier (i): fp32-mode kernels vs the fp32 oracle
BF16_TOL = 0.06         # tests/test_gpu_generate.py TOL: the bf16 path on a decoder score
CTC_TOL = 1e-3          # tests/test_gpu_ctc_beam.py SCORE_TOL: kernel scores vs ctc_beam_ref


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(got, want, keys=None):
    for k in (keys or want):
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (k, g.dtype, want[k].dtype, g.shape, want[k].shape)
        assert np.array_equal(bits(g), bits(want[k])), k


# ------------------------------------------------------------------------------------------------ 1. pack
def _pack_dev(tokens, n, ctc, V, U):
    from huggingface_asr_amd import ops
    out = ops.rescore_pack(torch.from_numpy(tokens).to(DEV), torch.from_numpy(n).to(DEV), torch.from_numpy(ctc).to(DEV), vocab=V, U=U, start_id=START, eos_id=EOS, pad_id=PAD)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_pack_is_exact_at_its_edges():
    got = _pack_dev(np.full((1, 1, 1), PAD, dtype=np.int64), np.zeros((1, 1), np.int32), np.zeros((1, 1), np.float32), 51, 1)        # (1, 1, 1, 1): only the empty hypothesis
    assert got["ids"].tolist() == [[START]] and got["labels"].tolist() == [[EOS]] and got["len"].tolist() == [1]
    for dtype in (np.int64, np.int32):
        tokens, n, ctc, V, U = pack_edge_case(dtype)                                     # (2, 3, 7, 5): too long, non-existent, out of vocabulary
        ids, labels, ln = RR.pack(tokens, n, ctc, V, U, START, EOS, PAD)
        got = _pack_dev(tokens, n, ctc, V, U)
        assert got["ids"].dtype == np.int64 and got["labels"].dtype == np.int64 and got["len"].dtype == np.int32
        assert np.array_equal(got["ids"], ids) and np.array_equal(got["labels"], labels) and np.array_equal(got["len"], ln)
        assert ln.tolist() == [1, 5, 0, 0, 0, 3]
        g = np.random.default_rng(3)                                                      # (3, 64, 40, 41): more than one block's worth of rows, rows longer than a wave
        B, N, Tt, U = 3, 64, 40, 41
        tokens = g.integers(0, 51, size=(B, N, Tt)).astype(dtype)
        n = g.integers(0, Tt + 1, size=(B, N)).astype(np.int32)
        n[0, :4] = [0, 40, 39, 41]                                                        # U - 1 = 40 fits; 41 is past U - 1 and past the token row
        ctc = (-g.random((B, N)) * 30).astype(np.float32)
        ctc[1, 5], ctc[1, 6], ctc[2, 7] = -np.inf, np.nan, np.inf
        tokens[2, 8, 3], tokens[2, 9, 0] = 51, -1
        n[2, 8], n[2, 9] = 10, 5
        ids, labels, ln = RR.pack(tokens, n, ctc, 51, U, START, EOS, PAD)
        assert ln[1] == 41 and ln[3] == 0 and ln[N + 5] == ln[N + 6] == ln[2 * N + 7] == ln[2 * N + 8] == ln[2 * N + 9] == 0 and (ln > 0).sum() > 150
        got = _pack_dev(tokens, n, ctc, 51, U)
        assert np.array_equal(got["ids"], ids) and np.array_equal(got["labels"], labels) and np.array_equal(got["len"], ln)


# ------------------------------------------------------------------------------------------------ 2. select
def _select_inputs(B, N, U):
    c = random_case(500 + 7 * B + N + U, B, N, U)
    if N >= 5:
        c["ln"][0, [1, 3, 4]] = min(3, U)                   # planted equal totals: three rows with the same numbers
        for n in (3, 4):
            c["nll"][0, n], c["ctc"][0, n] = c["nll"][0, 1], c["ctc"][0, 1]
        c["ln"][0, 2] = max(c["ln"][0, 2], 1)
        c["ctc"][0, 2] = -np.inf                            # a row whose total is -inf although it has tokens
    if B >= 2:
        c["ln"][B - 1] = 0                                  # an utterance without an existing row
    return c


@pytest.mark.parametrize("B,N,U", [(1, 1, 1), (2, 5, 9), (3, 64, 65), (2, 17, 130)])
def test_select_is_select32_bit_for_bit(B, N, U):
    from huggingface_asr_amd import ops
    c = _select_inputs(B, N, U)
    dv = {k: torch.from_numpy(v).to(DEV) for k, v in c.items()}
    for lp in (0.0, 0.6, 1.0):
        denom = RR.length_denoms(U, lp)
        dd = torch.from_numpy(denom).to(DEV)
        for w in (0.0, 0.3, 1.0):
            w_ctc, w_att = float(w), float(1 - w)
            for K in sorted({1, N}):
                for tok_dtype, frames in ((torch.int64, True), (torch.int32, False)):
                    want = RR.select32(c["nll"], c["ln"], c["ctc"], denom, np.float32(w_ctc), np.float32(w_att), K, c["tokens"], c["frames"] if frames else None, EOS, PAD)
                    runs = [ops.rescore_select(dv["nll"].reshape(-1), dv["ln"].reshape(-1), dv["ctc"], dd, dv["tokens"].to(tok_dtype), w_ctc=w_ctc, w_att=w_att, K=K,
                                               eos_id=EOS, pad_id=PAD, frames=dv["frames"] if frames else None) for _ in range(2)]
                    assert ("frames" in runs[0]) == frames
                    same_bits(runs[0], want)
                    same_bits(runs[1], want)                # the second run: the same bits
    if B >= 2:
        assert np.isneginf(want["total"][B - 1]).all() and want["order"][B - 1].tolist() == list(range(N))[:want["order"].shape[1]]
    if N >= 5:
        o = want["order"][0].tolist()
        assert o.index(3) == o.index(1) + 1 and o.index(4) == o.index(3) + 1


def test_select_and_pack_refuse_bad_arguments_before_any_launch():
    from huggingface_asr_amd import _lib
    L = _lib.lib()
    t = torch.zeros(64, dtype=torch.int64, device=DEV)
    p = t.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    sel = lambda N, K, U, order=p: L.mi_rescore_select(p, p, p, p, 0.3, 0.7, 1, N, U, K, p, 1, 1, None, EOS, PAD, order, p, p, p, p, p, p, None, st)
    assert sel(65, 1, 1) == _lib.ERR_ARG and sel(0, 1, 1) == _lib.ERR_ARG and sel(2, 3, 1) == _lib.ERR_ARG and sel(2, 0, 1) == _lib.ERR_ARG
    assert sel(2, 1, 0) == _lib.ERR_ARG and sel(2, 1, 1, None) == _lib.ERR_ARG
    assert L.mi_rescore_select(p, p, p, p, 0.3, 0.7, 1, 2, 1, 1, p, 1, 1, p, EOS, PAD, p, p, p, p, p, p, p, None, st) == _lib.ERR_ARG       # frames without out_frames
    assert L.mi_rescore_pack(p, 1, p, p, 1, 1, 1, 51, 0, START, EOS, PAD, p, p, p, st) == _lib.ERR_ARG
    assert L.mi_rescore_pack(p, 2, p, p, 1, 1, 1, 51, 1, START, EOS, PAD, p, p, p, st) == _lib.ERR_ARG
    assert L.mi_rescore_pack(p, 1, p, p, 1, 1, 1, 51, 1, START, EOS, PAD, None, p, p, st) == _lib.ERR_ARG
    assert L.mi_rows_nll_f32(p, 4, p, p, 8, p, 1, st) == _lib.ERR_ARG and L.mi_rows_nll_f32(None, 8, p, p, 8, p, 1, st) == _lib.ERR_ARG
    torch.cuda.synchronize()


def test_rows_nll_is_lse_minus_the_label_logit():
    from huggingface_asr_amd import ops
    g = torch.Generator().manual_seed(5)
    M, V = 600, 51
    buf = torch.randn(M, 56, generator=g).to(DEV)
    x = buf[:, :V]
    labels = torch.randint(0, V, (M,), generator=g)
    labels[::7] = -100
    labels[3] = V                                           # past the vocabulary: ignored as well
    lse = ops.row_lse(x)
    nll = ops.rows_nll(x, lse, labels.to(DEV)).cpu()
    ok = (labels >= 0) & (labels < V)
    want = lse.cpu() - x.cpu().gather(1, labels.clamp(0, V - 1)[:, None])[:, 0]
    assert torch.equal(nll[ok], want[ok]) and (nll[~ok] == 0).all() and not torch.signbit(nll[~ok]).any()


# ------------------------------------------------------------------------------------------------ 3. token_nll
def _dec_engine(precision):
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    sd, _, _, _ = aed_case_inputs(load_golden("aed_tiny"))
    eng = GPT2DecoderEngine(dict(TINY_DEC), DEV, precision=precision)
    eng.load_state_dict(sd)
    return sd, eng


@functools.lru_cache(maxsize=None)
def _nll_case(N, U):
    """B = 2 utterances with different enc_len, N hypotheses each: random tokens, lengths (U, 1, 0, ...) first, packed by the restatement"""
    g = np.random.default_rng(10 * N + U)
    B, T, d, V = 2, 37, TINY_DEC["n_embd"], TINY_DEC["vocab_size"]
    enc = torch.from_numpy(g.standard_normal((B, T, d)).astype(np.float32))
    lens = torch.tensor([T, 20], dtype=torch.int32)
    tokens = g.integers(3, V - 1, size=(B, N, U)).astype(np.int64)
    n = g.integers(1, U, size=(B, N)).astype(np.int32)
    ctc = -np.ones((B, N), dtype=np.float32)
    n[0, :3] = [U - 1, 0, 0]
    ctc[0, 2] = -np.inf                                      # len = (U, 1, 0, ...)
    ids, labels, ln = RR.pack(tokens, n, ctc, V, U, START, EOS, PAD)
    assert ln[:3].tolist() == [U, 1, 0]
    return enc, lens, torch.from_numpy(ids), torch.from_numpy(labels), ln


@functools.lru_cache(maxsize=None)
def _nll_oracle(N, U):
    from oracle import aed_ref as A
    sd, _, _, _ = aed_case_inputs(load_golden("aed_tiny"))
    enc, lens, ids, labels, ln = _nll_case(N, U)
    mask = (torch.arange(enc.shape[1])[None] < lens[:, None].long()).repeat_interleave(N, 0)
    with torch.no_grad():
        logits = A.decoder_forward(sd, "decoder.", dict(TINY_DEC), ids, enc.repeat_interleave(N, 0), mask, None)[1]
    lp = torch.log_softmax(logits.double(), -1)
    return -lp.gather(-1, labels.clamp(min=0)[..., None])[..., 0]                  # (rows, U); meaningful where labels >= 0


@pytest.mark.parametrize("N,U", [(3, 6), (5, 33)], ids=["N3xU6", "N5xU33"])       # 5 x 33 = 165 queries per utterance: past one 128-query block of the cross-attention
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_token_nll(precision, N, U):
    sd, eng = _dec_engine(precision)
    enc, lens, ids, labels, ln = _nll_case(N, U)
    B, T, d = enc.shape
    e = enc.to(DEV).view(B * T, d)
    e = e if precision == "fp32" else e.to(torch.bfloat16)
    idd, lad, ld = ids.to(DEV), labels.to(DEV), lens.to(DEV)
    nll = eng.token_nll(idd, lad, e, T, ld, N)
    assert nll.shape == (B * N * U,) and nll.dtype == torch.float32
    got = nll.view(B * N, U).cpu()
    valid = labels >= 0
    assert valid.sum() == int(ln.sum()) and (got[~valid] == 0).all()               # ignored positions: exactly 0
    if precision == "fp32":
        worst = float((got.double() - _nll_oracle(N, U))[valid].abs().max())
        print(f"RESCORE token_nll fp32 N={N} U={U}: max |nll - oracle| = {worst:.3e} (bar {F32_BAR:.0e})")
        assert worst <= F32_BAR
        eng.NLL_SCRATCH_BYTES = 56 * 4 * 7                                         # the head in chunks of 7 rows: the same bits
        again = eng.token_nll(idd, lad, e, T, ld, N)
        assert torch.equal(again, nll)
    else:
        rep = e.view(B, T, d).repeat_interleave(N, 0).reshape(B * N * T, d)        # forward() reads one encoder table per row
        logits = eng.forward(idd, rep, T, ld.repeat_interleave(N))["logits"]
        ref = -torch.log_softmax(logits.float(), -1).gather(-1, lad.clamp(min=0)[..., None])[..., 0].cpu()
        worst = float((got - ref)[valid].abs().max())
        vs_oracle = float((got.double() - _nll_oracle(N, U))[valid].abs().max())
        print(f"RESCORE token_nll bf16 N={N} U={U}: max |nll - nll(forward logits)| = {worst:.3e} (tol {BF16_TOL}); vs the fp32 oracle {vs_oracle:.3e}")
        assert worst <= BF16_TOL
    # other ids beyond every hypothesis' end: the valid positions keep their bits
    other = idd.clone()
    past = torch.arange(U, device=DEV)[None] >= torch.from_numpy(ln.astype(np.int64)).to(DEV)[:, None].clamp(min=1)
    other[past] = 7
    assert not torch.equal(other, idd)
    if precision == "fp32":
        eng.NLL_SCRATCH_BYTES = type(eng).NLL_SCRATCH_BYTES
    moved = eng.token_nll(other, lad, e, T, ld, N).view(B * N, U).cpu()
    assert torch.equal(moved[valid], got[valid])


def test_token_nll_refuses_a_position_table_that_is_too_short():
    _, eng = _dec_engine("bf16")
    U = TINY_DEC["n_positions"] + 1
    ids = torch.full((1, U), 5, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match="n_positions"):
        eng.token_nll(ids, ids, torch.zeros((8, TINY_DEC["n_embd"]), dtype=torch.bfloat16, device=DEV), 8, None, 1)


# ------------------------------------------------------------------------------------------------ 4. the CTC term
def test_ctc_term_equals_the_beam_scores_where_nothing_is_pruned():
    from huggingface_asr_amd import decoder as D
    from huggingface_asr_amd import ops
    from test_ctc_beam_cpu import DRAWS, SMALL, small_logits
    checked = 0
    for T, V1 in SMALL:
        x = torch.from_numpy(np.stack([small_logits(T, V1, s) for s in range(DRAWS)])).to(DEV)
        out = ops.ctc_beam_decode(x, V1 - 1, -5, None, beams=64, token_topk=V1 - 1, nbest=8)         # padded with a negative id: padding for the CTC loss as well
        lens = torch.full((DRAWS,), T, dtype=torch.int32, device=DEV)
        ctc = D.ctc_term(x, lens, out["tokens"]).cpu()
        sc = out["scores"].cpu()
        exists = torch.isfinite(sc)
        assert ctc.shape == sc.shape and exists.sum() >= DRAWS
        worst = float((ctc - sc)[exists].abs().max())
        print(f"RESCORE ctc term T={T} V1={V1}: max |ctc_loss term - beam score| = {worst:.3e} (bound {CTC_TOL:.0e})")
        assert worst <= CTC_TOL
        checked += int(exists.sum())
    assert checked > 200
    # a token that is no CTC class, and a transcript longer than the frames allow: -inf
    x = torch.from_numpy(small_logits(3, 4, 0)[None]).to(DEV)
    hyps = torch.tensor([[[0, 1, -1, -1], [3, -1, -1, -1], [0, 0, 0, -1], [-1, -1, -1, -1]]], device=DEV)
    ctc = D.ctc_term(x, torch.tensor([3], dtype=torch.int32, device=DEV), hyps).cpu()
    assert torch.isfinite(ctc[0, 0]) and torch.isneginf(ctc[0, 1]) and torch.isneginf(ctc[0, 2]) and torch.isfinite(ctc[0, 3])


# ------------------------------------------------------------------------------------------------ 5. end to end
@functools.lru_cache(maxsize=None)
def _joint(precision):
    from huggingface_asr_amd.decoder import JointAEDEngine
    c = RC.end_to_end_case()
    eng = JointAEDEngine(RC.ENC, c["dec_cfg"], AED_JCFG, DEV, precision=precision)
    eng.load_state_dict(c["sd"])
    return eng


def _select32_of_trace(tr, K):
    n = lambda t: t.cpu().numpy()
    return RR.select32(n(tr["nll"]), n(tr["len"]), n(tr["ctc"]), n(tr["denom"]), np.float32(tr["w_ctc"]), np.float32(tr["w_att"]), K, n(tr["tokens"]), n(tr["frames"]), GM.EOS, GM.PAD)


@pytest.mark.parametrize("max_length", [RC.MAX_LENGTH, RC.SHORT_MAX_LENGTH])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_rescore_end_to_end(precision, max_length):
    from huggingface_asr_amd import decoder as D
    c = RC.end_to_end_case(max_length)
    eng = _joint(precision)
    x, fl = c["x"].to(DEV), c["am"].sum(-1).to(DEV, torch.int32)
    tr, stats = {}, {}
    out = D.rescore(eng, x, fl, num_beams=RC.W, nbest=RC.NBEST, ctc_weight=RC.CTC_WEIGHT, length_penalty=RC.LENGTH_PENALTY, max_length=max_length, eos_token_id=GM.EOS,
                    trace=tr, stats=stats)
    assert set(stats) == {"encoder_ms", "ctc_beam_ms", "decoder_pass_ms", "select_ms"} and all(v >= 0 for v in stats.values())
    B = x.shape[0]
    longest = int(tr["n_tokens"].max())
    assert tr["U"] == min(longest + 1, max_length - 1) and tr["nll"].numel() == B * RC.NBEST * tr["U"]
    ids, labels, ln = RR.pack(tr["tokens"].cpu().numpy(), tr["n_tokens"].cpu().numpy(), tr["ctc"].cpu().numpy(), TINY_DEC["vocab_size"], tr["U"], GM.START, GM.EOS, GM.PAD)
    assert np.array_equal(tr["ids"].cpu().numpy(), ids) and np.array_equal(tr["labels"].cpu().numpy(), labels) and np.array_equal(tr["len"].cpu().numpy(), ln)
    assert (ln == 0).any() == (longest + 1 > max_length - 1) and (ln > 0).any()   # hypotheses that do not fit are dropped, and only those
    if max_length == RC.SHORT_MAX_LENGTH and precision == "fp32":                 # (the bf16 encoder's n-best need not be the oracle's)
        assert (ln == 0).any()
    want = _select32_of_trace(tr, RC.NBEST)
    same_bits(tr["select"], want)                                                 # order, totals, att, ctc (and the gathered rows), bit for bit
    for b, h in enumerate(out):
        assert h["order"] == want["order"][b].tolist() and len(h["hypotheses"]) == RC.NBEST
        assert np.array_equal(np.array([s for s, _ in h["hypotheses"]], dtype=np.float32), want["total"][b])
        assert np.array_equal(np.array(h["att_score"], dtype=np.float32), want["att"][b]) and np.array_equal(np.array(h["ctc_score"], dtype=np.float32), want["ctc"][b])
        assert h["tokens"] == h["hypotheses"][0][1] and h["score"] == h["hypotheses"][0][0]
        for k, (s, toks) in enumerate(h["hypotheses"]):
            n = int(want["n_tokens"][b, k])
            assert toks == [GM.START] + want["tokens"][b, k, :n].tolist() + [GM.EOS]
            assert len(h["token_logprobs"][k]) == n + 1 and h["frames"][k] == want["frames"][b, k, :n].tolist()
            if np.isfinite(s):
                assert float(np.float32(sum(np.float32(v) for v in h["token_logprobs"][k]))) == pytest.approx(h["att_score"][k], rel=1e-5)
    if precision == "fp32":
        kept = 0
        for b, rows in enumerate(c["oracle"]):
            gap = rows[0]["total"] - rows[1]["total"] if len(rows) > 1 else float("inf")
            dev = [(s, t) for s, t in out[b]["hypotheses"] if np.isfinite(s)]
            print(f"RESCORE e2e fp32 max_length={max_length} utt {b}: oracle top-1 {rows[0]['total']:.5f} gap {gap:.4f} device top-1 {dev[0][0]:.5f}; "
                  f"{len(dev)} device hypotheses, {len(rows)} oracle")
            if gap > RC.TOP1_GAP:
                kept += 1
                assert out[b]["tokens"] == [GM.START] + rows[0]["labels"] + [GM.EOS], b
        assert kept >= B - 1
    else:
        again = D.rescore(eng, x, fl, num_beams=RC.W, nbest=RC.NBEST, ctc_weight=RC.CTC_WEIGHT, length_penalty=RC.LENGTH_PENALTY, max_length=max_length,
                          eos_token_id=GM.EOS, num_return=2)
        for a, h in zip(again, out):                                              # fewer returned: the same ranking cut short
            assert a["hypotheses"] == h["hypotheses"][:2] and a["order"] == h["order"][:2]


def test_score_ranks_given_hypotheses_like_rescore():
    """decoder.score of the hypotheses rescore ranked: the same decoder pass (att within the bf16 tolerance of a re-laid-out pass), the exact CTC term in place of the
    beam search's kept mass (never below it), totals = select32 of score()'s own terms"""
    from huggingface_asr_amd import decoder as D
    c = RC.end_to_end_case()
    eng = _joint("bf16")
    x, fl = c["x"].to(DEV), c["am"].sum(-1).to(DEV, torch.int32)
    kw = dict(ctc_weight=RC.CTC_WEIGHT, length_penalty=RC.LENGTH_PENALTY, max_length=RC.MAX_LENGTH, eos_token_id=GM.EOS)
    tr = {}
    first = D.rescore(eng, x, fl, num_beams=RC.W, nbest=RC.NBEST, trace=tr, **kw)
    hyps = torch.where(torch.arange(tr["tokens"].shape[2], device=DEV)[None, None] < tr["n_tokens"][..., None], tr["tokens"], torch.full_like(tr["tokens"], -1))
    ts = {}
    got = D.score(eng, x, fl, hyps, trace=ts, **kw)
    same_bits(ts["select"], RR.select32(*(ts[k].cpu().numpy() for k in ("nll", "len", "ctc", "denom")), np.float32(ts["w_ctc"]), np.float32(ts["w_att"]), RC.NBEST,
                                        ts["tokens"].cpu().numpy(), None, GM.EOS, GM.PAD))
    for b in range(x.shape[0]):
        by_n = {n: k for k, n in enumerate(got[b]["order"])}
        for k, n in enumerate(first[b]["order"]):
            if not np.isfinite(first[b]["hypotheses"][k][0]):
                continue
            j = by_n[n]
            assert got[b]["hypotheses"][j][1] == first[b]["hypotheses"][k][1] and got[b]["frames"][j] is None
            d_att = abs(got[b]["att_score"][j] - first[b]["att_score"][k])
            d_ctc = got[b]["ctc_score"][j] - first[b]["ctc_score"][k]
            print(f"RESCORE score-vs-rescore utt {b} n {n}: d att {d_att:.3e}, exact CTC - beam CTC {d_ctc:.4f}")
            assert d_att <= BF16_TOL and d_ctc >= -CTC_TOL


# ------------------------------------------------------------------------------------------------ 6. the model surface
@functools.lru_cache(maxsize=None)
def _model():
    from test_surface_cpu import _joint_model
    from huggingface_asr_amd.decoding import GenerationConfigCustom
    c = RC.end_to_end_case()
    model = _joint_model(False)
    missing, unexpected = model.load_state_dict(c["sd"], strict=False)
    assert not missing and not unexpected
    model = model.to(DEV).eval()
    model.generation_config = GenerationConfigCustom(bos_token_id=GM.START, pad_token_id=GM.PAD, decoder_start_token_id=GM.START, length_penalty=RC.LENGTH_PENALTY,
                                                     early_stopping=False, eos_token_id=GM.EOS, max_length=RC.MAX_LENGTH, num_beams=RC.W, ctc_weight=RC.CTC_WEIGHT,
                                                     ctc_margin=0, lm_weight=0, lm_model=None, space_token_id=-1, apply_eos_space_trick=False, eos_space_trick_weight=1.0)
    return model


def test_model_rescore_score_and_the_generate_route(monkeypatch):
    from huggingface_asr_amd import decoder as D
    c = RC.end_to_end_case()
    model = _model()
    x, am = c["x"].to(DEV), c["am"].to(DEV)
    B, W = x.shape[0], RC.W
    ref = D.rescore(model._get_engine(DEV), x, am.sum(-1).to(torch.int32), num_beams=W, ctc_weight=RC.CTC_WEIGHT, length_penalty=RC.LENGTH_PENALTY, max_length=RC.MAX_LENGTH,
                    eos_token_id=GM.EOS)
    r = model.rescore(input_values=x, attention_mask=am, num_return_sequences=W, return_dict=True)
    L = r["sequences"].shape[1]
    assert set(r) == {"sequences", "sequences_scores", "ctc_scores", "attention_scores", "token_logprobs", "frames"}
    assert r["sequences"].shape == (B * W, L) and r["sequences"].dtype == torch.long and r["sequences"].is_cuda and L == max(len(t) for h in ref for _, t in h["hypotheses"])
    assert r["sequences_scores"].shape == r["ctc_scores"].shape == r["attention_scores"].shape == (B * W,) and r["token_logprobs"].shape == (B * W, L - 1)
    assert len(r["frames"]) == B * W
    for b in range(B):
        for k in range(W):
            s, toks = ref[b]["hypotheses"][k]
            row = r["sequences"][b * W + k].tolist()
            assert row[:len(toks)] == toks and all(v == GM.PAD for v in row[len(toks):])
            assert float(r["sequences_scores"][b * W + k]) == s and r["frames"][b * W + k] == ref[b]["frames"][k]
            tl = r["token_logprobs"][b * W + k].tolist()
            assert tl[:len(toks) - 1] == [float(np.float32(v)) for v in ref[b]["token_logprobs"][k]] and all(v == 0 for v in tl[len(toks) - 1:])
        sc = r["sequences_scores"][b * W:(b + 1) * W]
        assert bool((sc[:-1] >= sc[1:]).all())
    one = model.rescore(x, am)                                                     # the tensor return, one per utterance, options from the generation configuration
    assert isinstance(one, torch.Tensor) and one.shape[0] == B
    for b in range(B):
        toks = ref[b]["tokens"]
        assert one[b, :len(toks)].tolist() == toks and all(v == GM.PAD for v in one[b, len(toks):].tolist())
    # score() of rescore()'s own output: the rows' order is kept; the decoder term is reproduced, the CTC term is the exact probability (never below the beam search's
    # kept mass) and the totals are the objective of those two terms
    s = model.score(input_values=x, attention_mask=am, sequences=r["sequences"], return_dict=True)
    assert torch.equal(s["sequences"], r["sequences"]) and torch.equal(model.score(x, am, r["sequences"].view(B, W, L)), s["sequences_scores"])
    real = torch.isfinite(r["sequences_scores"])
    assert real.sum() >= 3 * B
    d_att = (s["attention_scores"] - r["attention_scores"])[real].abs().max()
    d_ctc = (s["ctc_scores"] - r["ctc_scores"])[real]
    n_gen = (r["sequences"] != GM.PAD).sum(-1).float() - 1                        # generated tokens, the EOS included
    recomputed = (RC.CTC_WEIGHT * s["ctc_scores"] + (1 - RC.CTC_WEIGHT) * s["attention_scores"]) / n_gen ** RC.LENGTH_PENALTY
    print(f"RESCORE model.score vs model.rescore: max d att {float(d_att):.3e}, exact CTC - beam CTC in [{float(d_ctc.min()):.4f}, {float(d_ctc.max()):.4f}]")
    assert float(d_att) <= BF16_TOL and float(d_ctc.min()) >= -CTC_TOL
    assert torch.allclose(s["sequences_scores"][real], recomputed[real], rtol=1e-5, atol=1e-6)
    assert bool((s["sequences_scores"][real] >= r["sequences_scores"][real] - (RC.CTC_WEIGHT * CTC_TOL + (1 - RC.CTC_WEIGHT) * BF16_TOL)).all())
    # generate() under the opt-in route returns rescore()'s sequences; without the variable it decodes token by token as before
    monkeypatch.setenv("HFASR_JOINT_RESCORE", "1")
    g1 = model.generate(input_values=x, attention_mask=am, num_beams=W)
    assert torch.equal(g1, one)
    g5 = model.generate(input_values=x, attention_mask=am, num_beams=W, num_return_sequences=W, return_dict_in_generate=True, output_scores=True)
    assert torch.equal(g5.sequences, r["sequences"]) and torch.equal(g5.sequences_scores, r["sequences_scores"])
    monkeypatch.delenv("HFASR_JOINT_RESCORE")
    plain = D.generate(model._get_engine(DEV), x, am.sum(-1).to(torch.int32), num_beams=W, max_length=RC.MAX_LENGTH, ctc_weight=RC.CTC_WEIGHT,
                       length_penalty=RC.LENGTH_PENALTY, eos_token_id=GM.EOS)
    g0 = model.generate(input_values=x, attention_mask=am, num_beams=W)
    for b in range(B):
        assert g0[b, :len(plain[b]["tokens"])].tolist() == plain[b]["tokens"]


def test_joint_engine_transcribe_and_align_are_the_encoder_engines():
    c = RC.end_to_end_case()
    eng = _joint("bf16")
    x, fl = c["x"].to(DEV), c["am"].sum(-1).to(DEV, torch.int32)
    for kw in (dict(), dict(return_frames=True), dict(beams=4, nbest=2, return_frames=True)):
        a, b = eng.transcribe(x, fl, pad_id=GM.PAD, **kw), eng.enc.transcribe(x, fl, pad_id=GM.PAD, **kw)
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a), kw
    labels = torch.tensor([[5, 6, 7, -100], [8, 9, -100, -100]], device=DEV)
    a, b = eng.align(x, fl, labels), eng.enc.align(x, fl, labels)
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a) and torch.isfinite(a["score"]).all()
