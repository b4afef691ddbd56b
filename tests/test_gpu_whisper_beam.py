"""GPU: Whisper beam search on the HIP path — the score kernel (`mi_whisper_beam_scores`) against transformers' processors on log-probabilities, the fan-out of the
self-attention cache, the device loop (`whisper.beam_decode`) against the reference loop of tests/whisper_beam_ref.py driven by the same engine's steps, and the routed
`generate` end to end."""
import os
import sys
import types

import pytest
import torch

from huggingface_asr_amd import ops, synth
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_whisper_generate import _generate_layout, _histories, _logits  # noqa: E402
from test_whisper_beam_cpu import closing_model  # noqa: E402
from whisper_beam_ref import beam_search_ref  # noqa: E402
from whisper_generate_common import LANG_TO_ID, NO_TIMESTAMPS, features, restore_generate, tiny_model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")
EOS, PAD = 2, 0


def _ts_processor(tb, eos, max_initial, detect, begin):
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    cfg = types.SimpleNamespace(no_timestamps_token_id=tb - 1, eos_token_id=eos, bos_token_id=eos, max_initial_timestamp_index=max_initial, _detect_timestamp_from_logprob=detect)
    return WhisperTimeStampLogitsProcessor(cfg, begin_index=begin)


def _margin(pre, tb):
    """|lse_ts - max_text| in fp64 over the columns that survive suppression and rules 1-4 (`pre`: the processor's output with rule 5 off)"""
    pre = pre.double()
    return torch.nan_to_num((torch.logsumexp(pre[:, tb:], -1) - pre[:, :tb].max(-1).values).abs(), nan=float("inf"))


# ------------------------------------------------------------------------------------------------------------------ 1. the score kernel
def score_cases():
    """(name, V, tb, ld, B, history, max_initial, detect, rules, suppress)"""
    out = []
    for V, tb, ld in ((120, 110, 120), (120, 110, 121), (1003, 900, 1016)):       # ld 121: rows off 16-byte alignment (the scalar path); V 1003: a tail of three columns
        for B in (1, 5):
            for name, h in _histories(V, tb).items():
                for mi in ((None, 0, 50) if not h else (None,)):
                    out.append((f"V{V} ld{ld} B{B} {name} max_initial {mi}", V, tb, ld, B, h, mi, True, True, True))
        h = _histories(V, tb)["text after a closed pair"]
        out.append((f"V{V} ld{ld} B5 no detection from logprob", V, tb, ld, 5, h, None, False, True, True))
        out.append((f"V{V} ld{ld} B5 rules off", V, tb, ld, 5, h, None, True, False, True))
        out.append((f"V{V} ld{ld} B5 no suppression vector", V, tb, ld, 5, h, None, True, True, False))
        out.append((f"V{V} ld{ld} B5 neither", V, tb, ld, 5, h, None, True, False, False))
    # a row longer than one sweep of the block (256 threads x 4 columns), V % 4 = 1
    out.append(("V51865 B6 text after a closed pair", 51865, 50364, 51872, 6, _histories(51865, 50364)["text after a closed pair"], None, True, True, True))
    return out


def score_reference():
    """every case's inputs and CPU reference, computed once: raw logits (the suppressed columns finite: they count in the normaliser), the suppression vector, and
    transformers' processors applied to log_softmax(raw) in `_retrieve_logit_processors`' order"""
    from transformers.generation.logits_process import SuppressTokensLogitsProcessor
    rows = []
    for name, V, tb, ld, B, h, mi, detect, rules, suppress in score_cases():
        P, eos = 3, 2
        x = _logits(V, tb, B, name)
        sup_cols = torch.from_numpy(synth.uniform(77, name + "/sup", (V,), 0.0, 1.0)) < 0.1
        raw = x.clone()
        raw[:, sup_cols] = torch.from_numpy(synth.normal(78, name + "/raw", (B, int(sup_cols.sum())), 3.0)).float() + 3.0        # large: leaving them out would move lse
        ids = torch.tensor([[1, tb - 8, tb - 6] + h] * B, dtype=torch.long)
        if len(h) >= 2 and B > 1:
            ids[1, -2:] = ids[1, -2:].flip(0)
            if ids[2, -1] >= tb:
                ids[2, -1] = min(int(ids[2, -1]) + 1, V - 1)
        sup = None
        if suppress:
            sup = torch.zeros(V)
            sup[sup_cols] = NINF
        logp = torch.log_softmax(raw, -1)
        if suppress:
            logp = SuppressTokensLogitsProcessor(sup_cols.nonzero().flatten().tolist(), device="cpu")(ids, logp)
        want, margin = logp, torch.full((B,), float("inf"))
        if rules:
            want = _ts_processor(tb, eos, mi, detect, P)(ids, logp.clone())
            if detect:
                margin = _margin(_ts_processor(tb, eos, mi, False, P)(ids, logp.clone()), tb)
        rows.append((name, raw, ids, P, tb, eos, mi, detect, rules, sup, ld, want == NINF, margin))
    return rows


def test_score_kernel_against_transformers_processors():
    """Per case: the set of -inf columns == that of processors(ids, log_softmax(raw)) on the CPU, every other value == the input bit for bit, lse == ops.row_lse(raw) bit
    for bit, columns past V untouched, two runs identical.  Rows whose rule-5 margin (fp64) is under 1e-4 are left out; at most 5 % may be."""
    rows = score_reference()
    total = sum(r[1].shape[0] for r in rows)
    under = sum(int((r[12] < 1e-4).sum()) for r in rows)
    print(f"{len(rows)} cases, {total} rows, {under} under the margin")
    assert under <= 0.05 * total
    for name, raw, ids, P, tb, eos, mi, detect, rules, sup, ld, want_inf, margin in rows:
        B, V = raw.shape
        idbuf = torch.full((B, ids.shape[1] + 5), V - 1, dtype=torch.long, device=DEV)       # timestamps behind cur_len must not be seen
        idbuf[:, :ids.shape[1]] = ids.to(DEV)
        kw = dict(begin_index=P, cur_len=ids.shape[1], suppress=sup.to(DEV) if sup is not None else None, eos_token_id=eos)
        if rules:
            kw.update(no_timestamps_token_id=tb - 1, max_initial_timestamp_index=mi, detect_from_logprob=detect)
        outs = []
        for _ in range(2):
            buf = torch.full((B, ld), 9.0e9, device=DEV)
            buf[:, :V] = raw.to(DEV)
            want_lse = ops.row_lse(buf[:, :V])
            lse = ops.whisper_beam_scores(buf[:, :V], idbuf, **kw)
            assert torch.equal(lse.view(torch.int32), want_lse.view(torch.int32)), (name, lse.tolist(), want_lse.tolist())
            assert bool((buf[:, V:] == 9.0e9).all()), name
            outs.append((buf.cpu(), lse.cpu()))
        assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(outs[0][1], outs[1][1]), name
        got = outs[0][0][:, :V]
        keep = margin >= 1e-4
        got_inf = got == NINF
        assert torch.equal(got_inf[keep], want_inf[keep]), (name, (got_inf != want_inf).nonzero().tolist()[:8], margin.tolist())
        same = got.view(torch.int32) == raw.view(torch.int32)
        assert bool((same | got_inf).all()), name                        # whatever is not -inf now is the input, bit for bit
    with pytest.raises(ValueError):
        ops.whisper_beam_scores(torch.zeros((2, 120), device=DEV), torch.ones((2, 4), dtype=torch.long, device=DEV), begin_index=3, cur_len=5)
    with pytest.raises(RuntimeError):
        ops.whisper_beam_scores(torch.zeros((2, 120), device=DEV), torch.ones((2, 4), dtype=torch.long, device=DEV), begin_index=3, cur_len=3, no_timestamps_token_id=120)


# ------------------------------------------------------------------------------------------------------------------ 2. the cache fan-out
def _engines(model, form=None):
    from huggingface_asr_amd.whisper import _decoder_engine_for, _engine_for
    enc, dec = _engine_for(model.model.encoder), _decoder_engine_for(model.model.decoder)
    dec.step_form = form
    return enc, dec


def test_cache_fan_out():
    """L = 2, d = 128, B = 2, W = 3, 12 positions of which 4 are consumed: dst[b W + k, :4] == src[b, :4] bit for bit in every layer's K and V, positions >= 4 of dst
    keep the sentinel they held"""
    from huggingface_asr_amd.whisper import fan_out_cache
    _, eng = _engines(tiny_model().to(DEV))
    B, W, Lmax, used = 2, 3, 12, 4
    src, dst = eng.init_cache(B, Lmax), eng.init_cache(B * W, Lmax)
    g = torch.Generator().manual_seed(5)
    for name in ("k", "v"):
        for t in src[name]:
            t.copy_(torch.randn(t.shape, generator=g).to(DEV, torch.bfloat16))
        for t in dst[name] + dst[name + "2"]:
            t.fill_(7.0)
    src["past"] = used
    out = fan_out_cache(eng, src, W, dst=dst)
    assert out is dst and dst["past"] == used and len(dst["k"]) == 2 and tuple(dst["k"][0].shape) == (B * W, Lmax, 128)
    for name in ("k", "v"):
        for s, t in zip(src[name], dst[name]):
            assert torch.equal(t[:, :used].view(torch.int16), s[:, :used].repeat_interleave(W, 0).view(torch.int16))
            assert bool((t[:, used:] == 7.0).all())
        for t in dst[name + "2"]:
            assert bool((t == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------ 3. the device loop
class EngineSteps:
    """`step_fn` and the scoring of the reference loop on the HIP engine: the prompt once per utterance, the cache fanned out, then `step(beams=W)` after the cache
    followed the beams — `beam_decode`'s own calls —; candidate values = logits - lse in fp32 with the kernel's lse, transformers' processors applied to them on the CPU.
    A row whose rule-5 margin is under 1e-4 takes the device's mask; for every other row the device's mask is asserted equal to the processors'."""

    def __init__(self, enc_eng, eng, x, prompt, W, max_length, gc, timestamps, state=None):
        from huggingface_asr_amd.packing import suppression_vectors
        from huggingface_asr_amd.whisper import fan_out_cache
        self.eng, self.W, self.P, self.fan = eng, W, prompt.shape[1], fan_out_cache
        B = prompt.shape[0]
        if state is None:
            e = enc_eng.forward(input_features=x)
            self.T2 = e.shape[1]
            self.kvs = eng.cross_kv(ops.cast_bf16(e.reshape(-1, e.shape[2])))
            self.cache1 = eng.init_cache(B, max_length)
        else:
            self.kvs, self.T2, self.cache1 = state["kvs"], state["T2"], state["cache"]
        self.every, self.first = suppression_vectors(120, gc.suppress_tokens, gc.begin_suppress_tokens, DEV)
        self.gc, self.timestamps = gc, timestamps
        self.cache, self.dev_logits = None, None
        self.skipped = self.compared = self.reorders = 0

    def step(self, new_tok, beam_idx):
        if beam_idx is None:
            base = self.eng.step(new_tok[::self.W, self.cache1["past"]:].to(DEV).contiguous(), self.cache1, self.kvs, self.T2)
            self.cache = self.fan(self.eng, self.cache1, self.W)
            self.dev_logits = base.repeat_interleave(self.W, 0).contiguous()
        else:
            self.reorders += int((beam_idx != torch.arange(beam_idx.numel())).any())
            self.eng.reorder_cache(self.cache, beam_idx.to(DEV))
            self.dev_logits = self.eng.step(new_tok.to(DEV), self.cache, self.kvs, self.T2, beams=self.W)
        return self.dev_logits.cpu()

    def scores(self, ids, logits):
        from transformers.generation.logits_process import SuppressTokensLogitsProcessor
        P, cur = self.P, ids.shape[1]
        sup = self.first if cur == P else self.every
        kw = dict(begin_index=P, cur_len=cur, suppress=sup, eos_token_id=EOS)
        ts = self.timestamps
        if ts is not None:
            kw.update(no_timestamps_token_id=NO_TIMESTAMPS, max_initial_timestamp_index=ts["max_initial_timestamp_index"], detect_from_logprob=True)
        masked = self.dev_logits.clone()
        lse = ops.whisper_beam_scores(masked, ids.to(DEV), **kw)
        dev_inf = masked.cpu() == NINF
        logp = logits - lse.cpu()[:, None]
        sup_ids = list(self.gc.suppress_tokens) + (list(self.gc.begin_suppress_tokens) if cur == P else [])
        want = SuppressTokensLogitsProcessor(sup_ids, device="cpu")(ids, logp.clone())
        margin = torch.full((ids.shape[0],), float("inf"))
        if ts is not None:
            tb = NO_TIMESTAMPS + 1
            margin = _margin(_ts_processor(tb, EOS, ts["max_initial_timestamp_index"], False, P)(ids, want.clone()), tb)
            want = _ts_processor(tb, EOS, ts["max_initial_timestamp_index"], True, P)(ids, want)
        near = margin < 1e-4
        self.skipped += int(near.sum())
        self.compared += int((~near).sum())
        assert torch.equal(dev_inf[~near], (want == NINF)[~near]), (cur, margin.tolist())
        want[near] = torch.where(dev_inf[near], torch.full_like(logp[near], NINF), logp[near])
        return want


LOOP_CASES = [
    # (name, W, route, timestamps, per-row language prompt, start from detect_language's state, length_penalty, early_stopping)
    ("W2", 2, None, False, False, False, 1.0, False),
    ("W5 timestamps", 5, None, True, False, False, 1.0, False),
    ("W5 languages, penalty 0.5, early stopping", 5, None, False, True, False, 0.5, True),
    ("W2 timestamps, after detect_language", 2, None, True, False, True, 1.0, "never"),
    ("W5 forced onto the wide route", 5, "device_wide", True, True, False, 1.0, False),
    ("W20 (the wide route)", 20, None, False, False, False, 1.0, False),
    ("W20 timestamps, after detect_language", 20, None, True, True, True, 2.0, False),
]


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("case", range(len(LOOP_CASES)))
def test_device_loop_equals_the_reference_loop(case, form):
    """`beam_decode` == the reference loop over the same engine's steps: ids, the kept hypotheses and their scores (fp32, bit for bit), B = 3, 12 new tokens, on the
    model whose EOS row is scaled so that hypotheses close before max_length.  At most 5 % of the scored rows may be under the rule-5 margin."""
    from huggingface_asr_amd.decoder import beam_loop_route
    from huggingface_asr_amd.whisper import beam_decode, detect_language, encode_for_decoding
    name, W, route, timestamps, languages, detected, lp, es = LOOP_CASES[case]
    model = closing_model(max_initial_timestamp_index=3).to(DEV)
    gc = model.generation_config
    enc_eng, eng = _engines(model, form)
    B, n_new = 3, 12
    x = features(B).to(DEV)
    rows = [[1, 100, 104], [1, 101, 104], [1, 102, 105]] if languages else [[1, 100, 104]] * 3
    ts = dict(no_timestamps_token_id=NO_TIMESTAMPS, max_initial_timestamp_index=3, detect_from_logprob=True) if timestamps else None

    def start():
        r = [list(q) for q in rows]
        state = None
        if detected:
            state = encode_for_decoding(enc_eng, eng, x, len(r[0]) + 1 + n_new)
            for q, lid in zip(r, detect_language(eng, state, 1, LANG_TO_ID.values()).tolist()):
                q[1] = lid
        return torch.tensor([q + ([] if timestamps else [NO_TIMESTAMPS]) for q in r], dtype=torch.long), state
    prompt, state = start()
    P = prompt.shape[1]
    want_route = route or beam_loop_route(W, 120, P + n_new)
    assert want_route == ("device_wide" if (W > 16 or route) else "device")
    calls = []
    fwd = enc_eng.forward
    enc_eng.forward = lambda *a, **k: calls.append(1) or fwd(*a, **k)
    try:
        stats = {}
        got = beam_decode(enc_eng, eng, x, prompt.to(DEV), max_new_tokens=n_new, eos_token_id=EOS, pad_token_id=PAD, num_beams=W, length_penalty=lp, early_stopping=es,
                          suppress_tokens=gc.suppress_tokens, begin_suppress_tokens=gc.begin_suppress_tokens, timestamps=ts, state=state, route=route, stats=stats)
    finally:
        del enc_eng.forward
    assert len(calls) == (0 if detected else 1) and stats["route"] == want_route       # after detect_language the encoder has already run, once
    prompt2, state2 = start()
    assert torch.equal(prompt2, prompt)
    drv = EngineSteps(enc_eng, eng, x, prompt, W, P + n_new, gc, ts, state2)
    ref = beam_search_ref(drv.step, lambda l: l, [drv.scores], prompt, num_beams=W, max_length=P + n_new, eos_token_id=EOS, pad_token_id=PAD, length_penalty=lp,
                          early_stopping=es)
    closed = sum(1 for k in ref["kept"] for s, t in k if t[-1] == EOS and len(t) < P + n_new)
    print(f"{name}, form {form}: route {stats['route']}, {stats['steps']} steps enqueued, reference {ref['steps']}; {drv.compared} rows scored, {drv.skipped} under the margin; "
          f"{closed} kept hypotheses closed before max_length, {drv.reorders} steps re-ordered the cache; ids {got[:, P:].tolist()}")
    assert drv.skipped <= 0.05 * (drv.skipped + drv.compared)
    assert ref["steps"] >= 5 and drv.reorders >= 2 and closed > 0        # the case is one: beams change places and hypotheses close while others run on
    assert got.dtype == torch.long and torch.equal(got.cpu(), ref["sequences"]), (got.tolist(), ref["sequences"].tolist())
    assert len(stats["hypotheses"]) == B
    for hyps, kept in zip(stats["hypotheses"], ref["kept"]):
        assert [t for _, t in hyps] == [t for _, t in kept]
        assert [s for s, _ in hyps] == [float(s) for s, _ in kept]
    if timestamps:
        tb = NO_TIMESTAMPS + 1
        for row in got[:, P:].tolist():
            row = row[:row.index(EOS)] if EOS in row else row
            assert tb <= row[0] <= tb + 3
            stamps = [t for t in row if t >= tb]
            assert stamps == sorted(stamps) and NO_TIMESTAMPS not in row
            assert not any(all(t >= tb for t in row[i:i + 3]) for i in range(len(row) - 2))


def test_shared_step_against_replicated_cross_kv():
    """`WhisperDecoderEngine.step(beams=W)` on the un-replicated cross K/V against `step` on W-fold replicated tables — the same caches, tokens and re-ordering —, held to
    `_compare` of tests/test_gpu_decode_long.py: the bound tests/test_gpu_wide_beam.py holds the joint model's shared-K/V step to against its replicated call
    (max |diff| < 0.06 max(std, 1) + 0.03, mean < 0.01 max(std, 1), equal argmax where the top-2 gap is over 0.1).  `beams=1` is untouched: bit-equal to the call
    without the keyword."""
    from test_gpu_decode_long import _compare
    from huggingface_asr_amd.whisper import fan_out_cache
    model = tiny_model().to(DEV)
    enc_eng, eng = _engines(model, 1)
    B, W, steps = 3, 5, 6
    e = enc_eng.forward(input_features=features(B).to(DEV))
    T2, d = e.shape[1], e.shape[2]
    shared = eng.cross_kv(ops.cast_bf16(e.reshape(B * T2, d)))
    repl = eng.cross_kv(ops.cast_bf16(e.repeat_interleave(W, 0).reshape(B * W * T2, d)))
    prompt = torch.tensor([[1, 100, 104, NO_TIMESTAMPS]] * B, device=DEV)

    def run(kvs, beams):
        c1 = eng.init_cache(B, 4 + steps)
        base = eng.step(prompt, c1, shared, T2)
        cache = fan_out_cache(eng, c1, W)
        out = []
        for u in range(steps):
            if u == 3:
                eng.reorder_cache(cache, torch.tensor([b * W + (k + 1) % W for b in range(B) for k in range(W)], device=DEV))
            tok = torch.tensor([[3 + (7 * r + 13 * u) % 100] for r in range(B * W)], device=DEV)
            out.append((eng.step(tok, cache, kvs, T2, beams=beams) if beams > 1 else eng.step(tok, cache, kvs, T2)).float().cpu())
        return base.float().cpu(), torch.stack(out, 1)
    base_s, got = run(shared, W)
    base_r, rep = run(repl, 1)
    assert torch.equal(base_s, base_r)
    worst = _compare(got, rep, B * W)
    print(f"shared vs replicated: max |diff| {worst:.2e}, bit-equal {torch.equal(got, rep)}")
    c = eng.init_cache(B, 6)
    c2 = eng.init_cache(B, 6)
    assert torch.equal(eng.step(prompt, c, shared, T2), eng.step(prompt, c2, shared, T2, beams=1))
    with pytest.raises(ValueError):
        eng.step(prompt, eng.init_cache(B, 6), shared, T2, beams=3)


# ------------------------------------------------------------------------------------------------------------------ 4. through generate
def test_beams_through_generate():
    """After `install_whisper(generate=True, beams=True)` under HFASR_WHISPER_STRICT=1 a beam call runs on the HIP path and returns `beam_decode`'s ids in the layout of
    Whisper's `generate` (long, no prompt columns, no EOS, pads on the right); with return_timestamps the rows obey the grammar; num_beams = 1 returns what it returned
    before the opt-in; with the switch off again the beam call is refused as before."""
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd import bind
    from huggingface_asr_amd import whisper as W
    os.environ["HFASR_WHISPER_STRICT"] = "1"
    bind.bind_all()
    restore_generate()
    try:
        model = tiny_model(suppress_tokens=[0, 5, 17, *range(110, 120)]).to(DEV)        # pad and the timestamp tokens suppressed: every call decodes one window
        gc = model.generation_config
        B = 4
        x = features(B).to(DEV)
        W.install_whisper(generate=True)
        greedy_before = model.generate(input_features=x, max_length=12, num_beams=1, language="en")
        with pytest.raises(NotImplementedError, match="num_beams > 1"):
            model.generate(input_features=x, max_length=12, num_beams=3, language="en")
        W.install_whisper(generate=True, beams=True)
        out = model.generate(input_features=x, max_length=12, num_beams=3, language="en")
        enc_eng, eng = _engines(model)
        prompt = torch.tensor([[1, 100, 104, NO_TIMESTAMPS]] * B, device=DEV)
        rules = dict(eos_token_id=EOS, pad_token_id=PAD, suppress_tokens=gc.suppress_tokens, begin_suppress_tokens=gc.begin_suppress_tokens)
        want = W.beam_decode(enc_eng, eng, x, prompt, max_new_tokens=12, num_beams=3, **rules)           # max_length 12 + the prompt's 4, as transformers counts it
        assert out.dtype == torch.long and torch.equal(out, _generate_layout(want, 4, EOS, PAD)), (out.tolist(), want.tolist())
        assert not bool((out == EOS).any()) and not bool((out[:, 0] == 1).any())
        gc4 = tiny_model(suppress_tokens=[0, 5, 17, *range(110, 120)], num_beams=3).to(DEV)              # the trainer's way: generation_config.num_beams
        assert torch.equal(gc4.generate(input_features=x, max_length=12, language="en"), out)
        assert torch.equal(model.generate(input_features=x, max_length=12, num_beams=1, language="en"), greedy_before)
        tsm = tiny_model(max_initial_timestamp_index=2, suppress_tokens=[0, 5, 17]).to(DEV)
        seq = tsm.generate(input_features=x[:2], max_length=12, num_beams=3, language="en", return_timestamps=True)      # several windows per row: a closed pair moves the window
        print(f"beams with timestamps through generate: {tuple(seq.shape)} {seq.tolist()}")
        assert seq.dtype == torch.long and seq.shape[0] == 2 and bool(((seq[:, 0] >= 110) & (seq[:, 0] <= 112)).all()) and not bool((seq == EOS).any())
        for row in seq.tolist():                                        # within a window: a timestamp opens it, none is below the one before it, <|notimestamps|> never
            row = [t for t in row if t != PAD]
            assert NO_TIMESTAMPS not in row and row[0] >= 110
        W.install_whisper(generate=True)
        with pytest.raises(NotImplementedError, match="num_beams > 1"):
            model.generate(input_features=x, max_length=12, num_beams=3, language="en")
    finally:
        restore_generate()
        W.BEAMS_ON_HIP = False
        os.environ.pop("HFASR_WHISPER_STRICT", None)
    assert MW.WhisperForConditionalGeneration.generate.__module__.startswith("transformers.")
