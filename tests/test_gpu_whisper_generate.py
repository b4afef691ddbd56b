"""GPU: `WhisperForConditionalGeneration.generate` on the HIP path — the timestamp-rule kernel against transformers' `WhisperTimeStampLogitsProcessor`, the device token
loop under those rules against a host loop over the same step, language detection against transformers' `detect_language`, and the routed `generate` end to end."""
import os
import sys
import types
import warnings

import pytest
import torch

from huggingface_asr_amd import ops, synth
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from whisper_generate_common import LANG_TO_ID, NO_TIMESTAMPS, features, restore_generate, tiny_model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")


# ------------------------------------------------------------------------------------------------------------------ 1. the rule kernel
def _histories(V, tb):
    """sampled-token histories by branch of the processor; text tokens are < tb - 1"""
    a, b = 7 % (tb - 1), 11 % (tb - 1)
    return {
        "first position": [],
        "text, no timestamp before it": [a],
        "a single sampled timestamp": [tb + 3],
        "text then a timestamp (the equal one stays allowed)": [a, tb + 4],
        "timestamp then timestamp": [tb + 2, tb + 2],
        "timestamp then text": [tb + 3, b],
        "text after a closed pair": [tb + 1, a, tb + 5, tb + 5, b],
        "last timestamp = V - 1": [a, V - 1],
        "open segment, long": [tb + 0, a, b, a, b, a, b, a],
    }


def _logits(V, tb, B, tag):
    """seeded fp32 rows: N(0, 3); a tenth of the columns -inf as from the suppress vector; by row: every text logit -inf / the timestamps' summed probability beats the
    best text token although no single one does / the best text token beats the sum / plain"""
    x = torch.from_numpy(synth.normal(77, tag, (B, V), 3.0)).float()
    x[:, torch.from_numpy(synth.uniform(77, tag + "/sup", (V,), 0.0, 1.0)) < 0.1] = NINF
    for r in range(B):
        kind = r % 4
        if kind == 1:
            x[r, :tb] = NINF
        elif kind == 2:
            m = float(x[r, :tb - 1].max())
            x[r, tb:] = m - 0.5                      # ten or more equal timestamps: their log-sum-exp is m - 0.5 + log(n) > m
        elif kind == 3:
            m = float(x[r, :tb - 1].max())
            x[r, tb:] = torch.minimum(x[r, tb:], torch.tensor(m - 12.0))        # even V - tb = 1501 of them sum to m - 12 + 7.3 < m
    return x


def _reference(x, ids, begin, tb, eos, max_initial, detect):
    """-> (argmax of transformers' processor on the CPU, |lse_ts - max_text| in fp64 over the columns that survive rules 1-4)"""
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    cfg = lambda d: types.SimpleNamespace(no_timestamps_token_id=tb - 1, eos_token_id=eos, bos_token_id=eos, max_initial_timestamp_index=max_initial, _detect_timestamp_from_logprob=d)
    want = torch.argmax(WhisperTimeStampLogitsProcessor(cfg(detect), begin_index=begin)(ids, x), -1)
    pre = WhisperTimeStampLogitsProcessor(cfg(False), begin_index=begin)(ids, x).double()
    margin = (torch.logsumexp(pre[:, tb:], -1) - pre[:, :tb].max(-1).values).abs()
    return want, torch.nan_to_num(margin, nan=float("inf"))


def rule_cases():
    """(name, V, tb, ld, B, history, max_initial, detect)"""
    out = []
    for V, tb, ld in ((120, 110, 120), (1003, 900, 1016)):
        for B in (1, 5):
            for name, h in _histories(V, tb).items():
                for mi in ((None, 0, 50) if not h else (None,)):
                    out.append((f"V{V} B{B} {name} max_initial {mi}", V, tb, ld, B, h, mi, True))
        out.append((f"V{V} B5 no detection from logprob", V, tb, ld, 5, _histories(V, tb)["text after a closed pair"], None, False))
    for V, tb, ld in ((120, 110, 121), (1003, 900, 1003)):           # row strides that leave rows off 16-byte alignment: the kernel's scalar path
        for name in ("first position", "text then a timestamp (the equal one stays allowed)", "text after a closed pair"):
            out.append((f"V{V} B5 {name}, rows not 16-byte aligned", V, tb, ld, 5, _histories(V, tb)[name], None, True))
    out.append(("V51865 B5 text after a closed pair", 51865, 50364, 51872, 5, _histories(51865, 50364)["text after a closed pair"], None, True))
    return out


def reference_rows():
    """every case's inputs and CPU reference, computed once: [(name, x (B, V), ids (B, P + n), P, tb, eos, max_initial, detect, ld, want, margin)]"""
    rows = []
    for name, V, tb, ld, B, h, mi, detect in rule_cases():
        P, eos = 3, 2
        x = _logits(V, tb, B, name)
        ids = torch.tensor([[1, tb - 8, tb - 6] + h] * B, dtype=torch.long)
        if len(h) >= 2 and B > 1:                     # the rows of a batch differ in their histories too: row 1 swaps its last two tokens, row 2 raises its last timestamp
            ids[1, -2:] = ids[1, -2:].flip(0)
            if ids[2, -1] >= tb:
                ids[2, -1] = min(int(ids[2, -1]) + 1, V - 1)
        want, margin = _reference(x, ids, P, tb, eos, mi, detect)
        rows.append((name, x, ids, P, tb, eos, mi, detect, ld, want, margin))
    return rows


def test_rule_kernel_against_transformers_processor():
    """Token == argmax(WhisperTimeStampLogitsProcessor(ids, logits)) bit for bit, except rows whose rule-5 margin |lse_ts - max_text| (fp64) is under 1e-4: the reference
    alone leaves 0 of the 177 rows of these 53 cases under it (checked on the CPU; at most 5 % may be).  Two runs give identical output; an ids buffer longer than the
    history and a row stride larger than V are what the token loop passes; strides of 121 and 1003 floats put rows off 16-byte alignment (the scalar path)."""
    rows = reference_rows()
    total = sum(r[1].shape[0] for r in rows)
    under = sum(int((r[10] < 1e-4).sum()) for r in rows)
    print(f"{len(rows)} cases, {total} rows, {under} under the margin")
    assert under <= 0.05 * total
    for name, x, ids, P, tb, eos, mi, detect, ld, want, margin in rows:
        B, V = x.shape
        buf = torch.full((B, ld), 9.0e9, device=DEV)                    # a value that would win if a column past V were read
        buf[:, :V] = x.to(DEV)
        idbuf = torch.full((B, ids.shape[1] + 5), V - 1, dtype=torch.long, device=DEV)       # timestamps behind cur_len must not be seen
        idbuf[:, :ids.shape[1]] = ids.to(DEV)
        kw = dict(begin_index=P, cur_len=ids.shape[1], no_timestamps_token_id=tb - 1, eos_token_id=eos, max_initial_timestamp_index=mi, detect_from_logprob=detect)
        got = ops.whisper_timestamp_argmax(buf[:, :V], idbuf, **kw)
        again = ops.whisper_timestamp_argmax(buf[:, :V], idbuf, **kw)
        assert got.dtype == torch.int32 and torch.equal(got, again)
        keep = margin >= 1e-4
        assert torch.equal(got.cpu().long()[keep], want[keep]), (name, got.tolist(), want.tolist(), margin.tolist())
    x = torch.full((2, 120), NINF, device=DEV)                          # nothing survives: 0, as torch.argmax over a row of -inf
    assert ops.whisper_timestamp_argmax(x, torch.ones((2, 4), dtype=torch.long, device=DEV), begin_index=3, cur_len=3, no_timestamps_token_id=109, eos_token_id=2).tolist() == [0, 0]
    with pytest.raises(ValueError):
        ops.whisper_timestamp_argmax(x, torch.ones((2, 4), dtype=torch.long, device=DEV), begin_index=3, cur_len=5, no_timestamps_token_id=109, eos_token_id=2)
    with pytest.raises(RuntimeError):
        ops.whisper_timestamp_argmax(x, torch.ones((2, 4), dtype=torch.long, device=DEV), begin_index=3, cur_len=3, no_timestamps_token_id=120, eos_token_id=2)


# ------------------------------------------------------------------------------------------------------------------ 2. the device loop under the rules
@pytest.fixture(scope="module")
def strict():
    os.environ["HFASR_WHISPER_STRICT"] = "1"
    yield
    os.environ.pop("HFASR_WHISPER_STRICT", None)


def _engines(model, form=None):
    from huggingface_asr_amd.whisper import _decoder_engine_for, _engine_for
    enc, dec = _engine_for(model.model.encoder), _decoder_engine_for(model.model.decoder)
    dec.step_form = form
    return enc, dec


@pytest.mark.parametrize("form", [1, 2])
def test_device_loop_with_timestamps_equals_a_host_loop(form):
    """greedy_decode(timestamps=...) == a host loop over the same `step` that applies transformers' suppression + timestamp processors to the step's logits on the CPU and
    takes torch.argmax; rows whose rule-5 margin is under 1e-4 (fp64) are not compared and the host loop follows the device's token there.  The output obeys the grammar."""
    from transformers.generation.logits_process import WhisperTimeStampLogitsProcessor
    from huggingface_asr_amd.packing import suppression_vectors
    from huggingface_asr_amd.whisper import greedy_decode
    model = tiny_model(max_initial_timestamp_index=3).to(DEV)
    gc = model.generation_config
    enc_eng, eng = _engines(model, form)
    B, max_new, tb, eos, pad = 3, 30, NO_TIMESTAMPS + 1, 2, 0
    x = features(B).to(DEV)
    prompt = torch.tensor([[1, 100, 104], [1, 101, 104], [1, 102, 105]], device=DEV)
    P = prompt.shape[1]
    ts = dict(no_timestamps_token_id=NO_TIMESTAMPS, max_initial_timestamp_index=3, detect_from_logprob=True)
    got = greedy_decode(enc_eng, eng, x, prompt, max_new_tokens=max_new, eos_token_id=eos, pad_token_id=pad, suppress_tokens=gc.suppress_tokens,
                        begin_suppress_tokens=gc.begin_suppress_tokens, timestamps=ts)
    # the host loop
    every, first = suppression_vectors(120, gc.suppress_tokens, gc.begin_suppress_tokens, DEV)
    proc = lambda d: WhisperTimeStampLogitsProcessor(types.SimpleNamespace(no_timestamps_token_id=NO_TIMESTAMPS, eos_token_id=eos, bos_token_id=1, max_initial_timestamp_index=3,
                                                                             _detect_timestamp_from_logprob=d), begin_index=P)
    e = enc_eng.forward(input_features=x)
    kvs = eng.cross_kv(ops.cast_bf16(e.reshape(-1, e.shape[2])))
    cache = eng.init_cache(B, P + max_new)
    ids, new = prompt.cpu(), prompt
    done = torch.zeros(B, dtype=torch.bool)
    skipped = compared = 0
    for n in range(got.shape[1] - P):
        logits = (eng.step(new, cache, kvs, e.shape[1]) + (first if n == 0 else every)).cpu()
        tok = torch.argmax(proc(True)(ids, logits), -1)
        pre = proc(False)(ids, logits).double()
        margin = torch.nan_to_num((torch.logsumexp(pre[:, tb:], -1) - pre[:, :tb].max(-1).values).abs(), nan=float("inf"))
        tok = torch.where(done, torch.full_like(tok, pad), tok)
        dev_tok = got[:, P + n].cpu()
        for b in range(B):
            if not done[b] and margin[b] < 1e-4:
                skipped += 1
                tok[b] = dev_tok[b]
            else:
                compared += 1
        assert torch.equal(tok, dev_tok), (n, tok.tolist(), dev_tok.tolist(), margin.tolist())
        ids = torch.cat([ids, tok[:, None]], 1)
        done = done | (tok == eos)
        new = tok[:, None].to(DEV)
    print(f"form {form}: {compared} tokens compared, {skipped} under the margin; ids {got[:, P:].tolist()}")
    assert skipped <= 0.05 * (skipped + compared)
    for row in got[:, P:].tolist():
        row = row[:row.index(eos)] if eos in row else row
        assert tb <= row[0] <= tb + 3                                                    # the first token is a timestamp <= timestamp_begin + max_initial
        stamps = [t for t in row if t >= tb]
        assert stamps == sorted(stamps)                                                  # non-decreasing
        assert not any(all(t >= tb for t in row[i:i + 3]) for i in range(len(row) - 2))  # no three in a row
        assert NO_TIMESTAMPS not in row


# ------------------------------------------------------------------------------------------------------------------ 3. language detection
def test_language_detection_against_transformers(strict):
    """HIP ids == transformers' fp32 `detect_language` (un-patched encoder and decoder forwards) wherever the reference's top-2 margin among the language logits is >= 2 x
    transformers' own bf16-autocast gap on the same inputs; at most 15 % of the rows may fall under that margin (these inputs: gap 0.013, 0 of 24 rows under it, two
    languages found).  The encoder runs once per `hip_generate` call."""
    from transformers.modeling_outputs import BaseModelOutput
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd import bind
    from huggingface_asr_amd.whisper import detect_language, encode_for_decoding, hip_generate
    bind.bind_all()
    model = tiny_model().to(DEV)
    gc = model.generation_config
    B = 24
    x = features(B, "lang_feats").to(DEV)
    lang = sorted(LANG_TO_ID.values())
    start = torch.full((B, 1), 1, dtype=torch.long, device=DEV)

    def ref_logits(autocast):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            e = MW.WhisperEncoder._hfasr_reference_forward(model.model.encoder, x).last_hidden_state
            return model(encoder_outputs=BaseModelOutput(last_hidden_state=e), decoder_input_ids=start, use_cache=False).logits[:, -1].float()[:, lang], e
    ref, e32 = ref_logits(False)
    gap = float((ref_logits(True)[0] - ref).abs().max())
    top = ref.topk(2, -1).values
    decisive = (top[:, 0] - top[:, 1]) >= 2.0 * gap
    want = model.detect_language(encoder_outputs=BaseModelOutput(last_hidden_state=e32), generation_config=gc)
    assert torch.equal(want, torch.tensor(lang, device=DEV)[ref.argmax(-1)])
    enc_eng, eng = _engines(model)
    state = encode_for_decoding(enc_eng, eng, x, 8)
    got = detect_language(eng, state, 1, LANG_TO_ID.values())
    under = int((~decisive).sum())
    print(f"gap {gap:.4f}; rows under the margin {under} of {B}; languages found {sorted(set(got.tolist()))}; equal {int((got == want).sum())} of {B}")
    assert under <= 0.15 * B and state["cache"]["past"] == 1
    assert got.dtype == torch.long and set(got.tolist()) <= set(lang) and not bool((decisive & (got != want)).any())
    # one encoder run per call, detection included; the call equals the one with the detected languages given
    calls = []
    fwd = enc_eng.forward
    enc_eng.forward = lambda *a, **k: calls.append(1) or fwd(*a, **k)
    try:
        out = hip_generate(model, x[:5], max_new_tokens=10)
    finally:
        del enc_eng.forward
    assert len(calls) == 1
    name = {v: k for k, v in LANG_TO_ID.items()}
    assert out[:, 1].tolist() == got[:5].tolist() and bool((out[:, 0] == 1).all()) and bool((out[:, 2] == NO_TIMESTAMPS).all())
    given = hip_generate(model, x[:5], max_new_tokens=10, language=[name[i] for i in got[:5].tolist()], task=None)
    assert given[:, :4].tolist() == [[1, i, 104, NO_TIMESTAMPS] for i in got[:5].tolist()]        # (a given language brings the default task token with it)


# ------------------------------------------------------------------------------------------------------------------ 4. the routed generate
def _generate_layout(ids, P, eos, pad):
    """what transformers' Whisper `generate` makes of greedy ids (B, P + n): no prompt columns, the row up to its EOS, right-padded to the longest"""
    rows = []
    for r in ids[:, P:].tolist():
        rows.append(r[:r.index(eos)] if eos in r else r)
    width = max(len(r) for r in rows)
    return torch.tensor([r + [pad] * (width - len(r)) for r in rows], dtype=torch.long, device=ids.device)


def test_generate_routed_end_to_end(strict):
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd import bind
    from huggingface_asr_amd import whisper as W
    bind.bind_all()
    restore_generate()
    W.install_whisper(generate=True)
    try:
        # pad and the timestamp tokens suppressed: rows are unambiguous and every call decodes one window
        model = tiny_model(suppress_tokens=[0, 5, 17, *range(110, 120)]).to(DEV)
        gc = model.generation_config
        B, eos, pad = 4, 2, 0
        x = features(B).to(DEV)
        m = torch.ones((B, 200), dtype=torch.long, device=DEV)
        enc_eng, eng = _engines(model)
        rules = dict(eos_token_id=eos, pad_token_id=pad, suppress_tokens=gc.suppress_tokens, begin_suppress_tokens=gc.begin_suppress_tokens)
        out = model.generate(input_features=x, attention_mask=m, max_length=20, num_beams=1, language="en")
        prompt = torch.tensor([[1, 100, 104, NO_TIMESTAMPS]] * B, device=DEV)
        want = W.greedy_decode(enc_eng, eng, x, prompt, max_new_tokens=20, **rules)                  # max_length 20 + the prompt's 4, as transformers counts it
        assert out.dtype == torch.long and torch.equal(out, _generate_layout(want, 4, eos, pad)), (out.tolist(), want.tolist())
        ref = MW.WhisperForConditionalGeneration._hfasr_reference_generate(model, input_features=x, attention_mask=m, max_length=20, num_beams=1, language="en")
        print(f"hip {tuple(out.shape)} reference {tuple(ref.shape)}; equal tokens {int((out[:, :min(out.shape[1], ref.shape[1])] == ref[:, :min(out.shape[1], ref.shape[1])]).sum())} of {out.numel()}")
        assert ref.dtype == out.dtype and ref.device == out.device and ref.shape[0] == out.shape[0] and ref.shape[1] <= 20 and out.shape[1] <= 20
        for t in (out, ref):                                                                          # no prompt columns, no EOS, pads on the right only, no all-pad column
            assert not bool((t == eos).any()) and not bool((t[:, 0] == 1).any())
            assert all(pad not in r[:len([v for v in r if v != pad])] for r in t.tolist()) and bool((t != pad).any(0).all())
        # the layout of the two, shape included, on rows of one length (EOS suppressed too: no near tie can end a row early in one of them only)
        fixed = tiny_model(suppress_tokens=[0, 2, 5, 17, *range(110, 120)]).to(DEV)
        call = dict(input_features=x, attention_mask=m, max_length=20, num_beams=1, language="en")
        o2, r2 = fixed.generate(**call), MW.WhisperForConditionalGeneration._hfasr_reference_generate(fixed, **call)
        print(f"EOS suppressed: hip {tuple(o2.shape)} reference {tuple(r2.shape)}; equal tokens {int((o2 == r2).sum()) if o2.shape == r2.shape else -1} of {o2.numel()}")
        assert o2.shape == r2.shape == (B, 20) and o2.dtype == r2.dtype and o2.device == r2.device and not bool((o2[:, 0] == 1).any()) and not bool((r2[:, 0] == 1).any())
        # no language: detection on the device == the detected languages given per row
        auto = model.generate(input_features=x, max_length=20)
        # the keyword arguments Seq2SeqTrainer.prediction_step passes for the recipes (the collator's labels among them) take the HIP path — STRICT is on — and change nothing
        labels = torch.full((B, 7), -100, dtype=torch.long, device=DEV)
        assert torch.equal(auto, model.generate(input_features=x, attention_mask=m, labels=labels, max_length=20, num_beams=1, synced_gpus=False))
        state = W.encode_for_decoding(enc_eng, eng, x, 8)
        name = {v: k for k, v in LANG_TO_ID.items()}
        langs = [name[i] for i in W.detect_language(eng, state, 1, LANG_TO_ID.values()).tolist()]
        task_to_id = gc.task_to_id
        del gc.task_to_id                                                                             # (with it a given language would add the task token)
        assert torch.equal(auto, model.generate(input_features=x, max_length=20, language=langs))
        gc.task_to_id = task_to_id
        # forced_decoder_ids of the generation config: the prompt transformers builds
        gc.forced_decoder_ids = [[1, 101], [2, 105], [3, NO_TIMESTAMPS]]
        forced = model.generate(input_features=x, max_new_tokens=9)
        assert model._retrieve_init_tokens(x, batch_size=B, generation_config=_with_rt(gc), config=model.config, num_segment_frames=200, kwargs={}).tolist() == [[1, 101, 105, NO_TIMESTAMPS]] * B
        fp = torch.tensor([[1, 101, 105, NO_TIMESTAMPS]] * B, device=DEV)
        assert torch.equal(forced, _generate_layout(W.greedy_decode(enc_eng, eng, x, fp, max_new_tokens=9, **rules), 4, eos, pad))
        gc.forced_decoder_ids = None
        # timestamps through generate: the grammar holds per row
        tsm = tiny_model(max_initial_timestamp_index=2, suppress_tokens=[0, 5, 17]).to(DEV)
        seq = tsm.generate(input_features=x, max_length=16, language="en", return_timestamps=True)     # several windows per row: a closed pair moves the window behind it
        print(f"timestamps through generate: {tuple(seq.shape)}")
        assert seq.dtype == torch.long and seq.shape[0] == B and bool(((seq[:, 0] >= 110) & (seq[:, 0] <= 112)).all()) and not bool((seq == eos).any())
        # beams: refused under STRICT; handed to transformers with one warning without it
        with pytest.raises(NotImplementedError, match="num_beams > 1"):
            model.generate(input_features=x, max_length=12, num_beams=2, language="en")
        os.environ.pop("HFASR_WHISPER_STRICT")
        W._stock_generate.said.clear()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            beams = model.generate(input_features=x, max_length=12, num_beams=2, language="en")
            model.generate(input_features=x, max_length=12, num_beams=2, language="en")
        os.environ["HFASR_WHISPER_STRICT"] = "1"
        assert len([w for w in rec if "num_beams > 1" in str(w.message)]) == 1
        assert torch.equal(beams, MW.WhisperForConditionalGeneration._hfasr_reference_generate(model, input_features=x, max_length=12, num_beams=2, language="en"))
    finally:
        restore_generate()
    assert MW.WhisperForConditionalGeneration.generate.__module__.startswith("transformers.")


def _with_rt(gc):
    import copy
    g = copy.deepcopy(gc)
    g.return_timestamps = False
    return g
