"""CPU: the host side of `WhisperForConditionalGeneration.generate` on the HIP path — the prompt builder against transformers' own `_retrieve_init_tokens`, the routing
(`generate_route`, HFASR_WHISPER_STRICT, `install_whisper(generate=True)`), and the segment loop (`generate_segments`) against transformers' own `generate` with
transformers' token loop injected as the decoder, so that the returned layout is the installed version's, multi-segment timestamp outputs included."""
import copy
import itertools
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from whisper_generate_common import LANG_TO_ID, NO_TIMESTAMPS, SEED, TASK_TO_ID, features, fill, restore_generate, tiny_model  # noqa: E402,F401


@pytest.fixture(autouse=True)
def _warned_once_sets_as_found():
    """the bound forwards warn once per reason and process: what these tests make them say must not count as said for the tests that run after them"""
    from huggingface_asr_amd import whisper as W
    before = [(f, set(f.said)) for f in (W._stock_forward, W._stock_decoder_forward, W._stock_generate)]
    yield
    for f, said in before:
        f.said.clear()
        f.said.update(said)


# ------------------------------------------------------------------------------------------------------------------ 1. the prompt builder
B = 3
DETECTED = [101, 102, 100]
LANGUAGES = [None, "en", "english", "<|en|>", ["en", "de", "fr"], ["en", "de"], "klingon", "ja", ["en", None, "fr"]]
TASKS = [None, "transcribe", "translate", "transcription"]
FORCED = [None, [[1, None], [2, 104]], [[1, 100], [2, 104], [3, NO_TIMESTAMPS]], [[1, 100], [3, NO_TIMESTAMPS]]]


def _outcome(fn):
    try:
        return ("ok", fn())
    except Exception as e:          # noqa: BLE001 — the type is what is compared
        return ("raised", type(e))


def test_prompt_builder_against_transformers():
    """Equal token lists, equal exception types, over language x task x return_timestamps x forced_decoder_ids x is_multilingual (9 x 4 x 2 x 4 x 2 = 576 calls), the
    reference being `_set_language_and_task` + `_retrieve_init_tokens` of the installed transformers on a copy of the generation config, `detect_language` stubbed."""
    from huggingface_asr_amd.whisper import build_prompt
    model = tiny_model()
    model.detect_language = lambda **kw: torch.tensor(DETECTED)
    x = torch.zeros(B, 80, 200)
    seen = {"ok": 0, "raised": 0}
    for language, task, rt, forced, multi in itertools.product(LANGUAGES, TASKS, (False, True), FORCED, (True, False)):
        gc = copy.deepcopy(model.generation_config)
        gc.forced_decoder_ids = copy.deepcopy(forced)

        def reference():
            g = copy.deepcopy(gc)
            g.return_timestamps = rt
            model._set_language_and_task(language=language, task=task, is_multilingual=multi, generation_config=g)
            return model._retrieve_init_tokens(x, batch_size=B, generation_config=g, config=model.config, num_segment_frames=200, kwargs={}).tolist()

        calls = []
        want = _outcome(reference)
        got = _outcome(lambda: build_prompt(gc, model.config, B, language=language, task=task, is_multilingual=multi, return_timestamps=rt,
                                            detect_language=lambda: calls.append(1) or list(DETECTED)))
        assert got == want, (language, task, rt, forced, multi, got, want)
        assert len(calls) <= 1
        assert gc.to_dict() == {**copy.deepcopy(model.generation_config).to_dict(), "forced_decoder_ids": forced}          # the builder leaves the config alone
        seen[want[0]] += 1
    assert seen["ok"] >= 100 and seen["raised"] >= 100, seen


def test_prompt_builder_cases_by_hand():
    from huggingface_asr_amd.whisper import build_prompt
    model = tiny_model()
    gc, cfg = model.generation_config, model.config
    det = lambda: list(DETECTED)
    assert build_prompt(gc, cfg, 3, detect_language=det) == [[1, 101, NO_TIMESTAMPS], [1, 102, NO_TIMESTAMPS], [1, 100, NO_TIMESTAMPS]]
    assert build_prompt(gc, cfg, 2, language="German") == [[1, 101, 104, NO_TIMESTAMPS]] * 2
    assert build_prompt(gc, cfg, 2, language=["fr", "<|es|>"], task="translate", return_timestamps=True) == [[1, 102, 105], [1, 103, 105]]
    g2 = copy.deepcopy(gc)
    g2.forced_decoder_ids = [[1, None], [2, 105], [3, NO_TIMESTAMPS]]
    assert build_prompt(g2, cfg, 1, detect_language=lambda: [103]) == [[1, 103, 105, NO_TIMESTAMPS]]
    assert build_prompt(g2, cfg, 1, detect_language=lambda: [103], return_timestamps=True) == [[1, 103, 105]]
    g3 = copy.deepcopy(gc)
    del g3.lang_to_id, g3.task_to_id, g3.no_timestamps_token_id, g3.is_multilingual                  # an English-only checkpoint's config
    assert build_prompt(g3, cfg, 2) == [[1], [1]]
    cfg2 = copy.deepcopy(cfg)
    cfg2.forced_decoder_ids = [[1, 100], [2, 104]]                                                    # the model config's, when the generation config has none
    assert build_prompt(g3, cfg2, 1) == [[1, 100, 104]]
    with pytest.raises(ValueError, match="language has to be detected"):
        build_prompt(gc, cfg, 1)
    from huggingface_asr_amd.whisper import LANGUAGE_TO_DETECT, prompt_template
    assert prompt_template(gc, cfg, 2) == ([[1, LANGUAGE_TO_DETECT, NO_TIMESTAMPS]] * 2, True)       # one call: the prompt's length and whether to detect
    assert prompt_template(gc, cfg, 2, language="fr") == ([[1, 102, 104, NO_TIMESTAMPS]] * 2, False)
    g4 = copy.deepcopy(gc)
    g4.decoder_start_token_id = None                                                                  # the model config's start token stands in; none at all is an error
    assert build_prompt(g4, cfg, 1, language="en") == [[1, 100, 104, NO_TIMESTAMPS]]
    import types
    cfg3 = types.SimpleNamespace(forced_decoder_ids=None, decoder_start_token_id=None)               # (`build_prompt` only reads these two)
    with pytest.raises(ValueError, match="decoder_start_token_id"):
        build_prompt(g4, cfg3, 1, language="en")


# ------------------------------------------------------------------------------------------------------------------ 2. routing
class _Cuda:
    """stands in for a device tensor: `generate_route` only asks for `.is_cuda`"""
    is_cuda = True


def _route(model, input_shape=(2, 80, 200), **kw):
    from huggingface_asr_amd.whisper import generate_route, resolved_generation_config
    gc = resolved_generation_config(model, None, kw)
    return generate_route(dict(kw, input_features=kw.get("input_features", _Cuda())), gc, model.config, input_shape)


def test_generate_route():
    model = tiny_model()
    hip = ("hip", None)
    assert _route(model, max_length=20) == hip
    assert _route(model, max_length=448, num_beams=1, synced_gpus=False) == hip
    # what Seq2SeqTrainer.prediction_step passes for the recipes: the collator's batch — labels included, which transformers' generate does not read — + its gen_kwargs
    assert _route(model, attention_mask=_Cuda(), labels=_Cuda(), max_length=448, num_beams=1, synced_gpus=False) == hip
    assert _route(model, max_new_tokens=5, language="en", task="translate", is_multilingual=True, attention_mask=_Cuda(), do_sample=False, temperature=0.0) == hip
    assert _route(model, max_length=20, language=["en", "de"], return_timestamps=True, return_dict_in_generate=False, decoder_input_ids=_Cuda()) == hip
    assert _route(model, max_length=20, temperature=(0.0,)) == hip
    handed = {
        "num_beams > 1": dict(num_beams=2),
        "sampling": dict(do_sample=True),
        "temperature fallback": dict(temperature=(0.0, 0.2, 0.4)),
        "prompt_ids": dict(prompt_ids=torch.tensor([3, 4])),
        "condition_on_prev_tokens": dict(condition_on_prev_tokens=True),
        "return_token_timestamps": dict(return_token_timestamps=True),
        "return_segments": dict(return_segments=True),
        "no_speech_threshold / logprob_threshold / compression_ratio_threshold": dict(no_speech_threshold=0.6),
        "custom logits processors / stopping criteria": dict(logits_processor=[lambda i, s: s]),
        "streamer": dict(streamer=object()),
        "assistant model": dict(assistant_model=object()),
        "return_dict_in_generate": dict(return_dict_in_generate=True),
        "CPU tensors": dict(input_features=torch.zeros(1)),
        "generation_config.repetition_penalty": dict(repetition_penalty=1.2),
        "keyword arguments ['head_mask']": dict(head_mask=torch.ones(2)),
    }
    for why, kw in handed.items():
        assert _route(model, max_length=20, **kw) == ("stock", why), (why, _route(model, max_length=20, **kw))
    for kw in (dict(logprob_threshold=-1.0), dict(compression_ratio_threshold=1.35)):
        assert _route(model, max_length=20, **kw)[1] == "no_speech_threshold / logprob_threshold / compression_ratio_threshold"
    assert _route(model, max_length=20, stopping_criteria=[lambda i, s: False])[1] == "custom logits processors / stopping criteria"
    assert _route(model, max_length=20, temperature=0.7) == ("stock", "sampling")
    assert _route(model, (2, 80, 600), max_length=20) == ("stock", "long-form input, or input features that are not (B, mel, 2 max_source_positions)")
    assert _route(model, (2, 80, 100), max_length=20)[0] == "stock" and _route(model, None, max_length=20)[0] == "stock"
    old = tiny_model()
    del old.generation_config.lang_to_id, old.generation_config.no_timestamps_token_id
    assert _route(old, max_length=20, language="en") == ("stock", "language on a generation config without lang_to_id")
    assert _route(old, max_length=20, return_timestamps=True) == ("stock", "return_timestamps on a generation config without no_timestamps_token_id")
    assert _route(old, max_length=20) == hip
    assert _route(tiny_model(num_beams=4), max_length=20) == ("stock", "num_beams > 1")             # the trainer sets generation_config.num_beams


def test_install_and_strict(monkeypatch):
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd import whisper as W
    cls = MW.WhisperForConditionalGeneration
    restore_generate()
    try:
        W.install_whisper()
        assert cls.generate.__module__.startswith("transformers.") and not hasattr(cls, "_hfasr_reference_generate")
        W.install_whisper(generate=True)
        ref = cls._hfasr_reference_generate
        assert cls.generate is W.hip_whisper_generate and ref.__module__.startswith("transformers.")
        W.install_whisper(generate=True)
        W.install_whisper()
        assert cls.generate is W.hip_whisper_generate and cls._hfasr_reference_generate is ref        # idempotent; the original is kept
        model, x = tiny_model(), features(2)
        want = ref(model, input_features=x, max_length=12, language="en")
        monkeypatch.delenv("HFASR_WHISPER_STRICT", raising=False)
        W._stock_generate.said.clear()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got = model.generate(input_features=x, max_length=12, language="en")                      # CPU tensors: transformers' own generate, said once
            model.generate(input_features=x, max_length=12, language="en")
        assert torch.equal(got, want)
        assert len([w for w in rec if "CPU tensors" in str(w.message) and "huggingface_asr_amd" in str(w.message)]) == 1
        monkeypatch.setenv("HFASR_WHISPER_STRICT", "1")
        with pytest.raises(NotImplementedError, match="CPU tensors"):
            model.generate(input_features=x, max_length=12, language="en")
        with pytest.raises(NotImplementedError, match="num_beams > 1"):
            model.generate(input_features=x, max_length=12, num_beams=2)
        assert "_hfasr_engine" not in model.model.decoder.__dict__                                     # nothing was built on the way
    finally:
        restore_generate()
    assert cls.generate.__module__.startswith("transformers.") and not hasattr(cls, "_hfasr_reference_generate")


def test_bind_all_reads_the_environment(monkeypatch):
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd import bind
    from huggingface_asr_amd import whisper as W
    cls = MW.WhisperForConditionalGeneration
    restore_generate()
    try:
        monkeypatch.delenv("HFASR_WHISPER_GENERATE", raising=False)
        bind.bind_all()
        assert cls.generate.__module__.startswith("transformers.")
        monkeypatch.setenv("HFASR_WHISPER_GENERATE", "1")
        bind.bind_all()
        assert cls.generate is W.hip_whisper_generate
    finally:
        restore_generate()


def test_hip_generate_takes_the_new_options_up_to_the_device():
    """language / task / return_timestamps are no longer refused where the generation config defines them: the call gets as far as asking for the GPU; the prompt
    builder's errors come first"""
    from huggingface_asr_amd.whisper import hip_generate
    model, x = tiny_model(), features(2)
    for kw in (dict(language="en"), dict(task="translate", language=["en", "de"]), dict(return_timestamps=True), dict(is_multilingual=True), dict()):
        with pytest.raises(RuntimeError, match="GPU"):
            hip_generate(model, x, max_new_tokens=4, **kw)
    with pytest.raises(ValueError, match="Unsupported language"):
        hip_generate(model, x, max_new_tokens=4, language="klingon")
    with pytest.raises(ValueError, match="English-only"):
        hip_generate(model, x, max_new_tokens=4, language="en", is_multilingual=False)
    with pytest.raises(ValueError, match="max_target_positions"):
        hip_generate(model, x, max_new_tokens=37, language="en")                                      # the prompt is four tokens
    with pytest.raises(NotImplementedError):
        hip_generate(model, x, max_new_tokens=4, prompt_ids=torch.tensor([3]))
    assert "_hfasr_engine" not in model.model.decoder.__dict__ and "_hfasr_engine" not in model.model.encoder.__dict__


# ------------------------------------------------------------------------------------------------------------------ 3. the segment loop
def _transformers_token_loop(model, gc, timestamps):
    """`decode_segment` for `generate_segments` made of transformers' own parts: `GenerationMixin.generate` under the processors Whisper's generate would hand it"""
    from transformers.generation.logits_process import SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor, WhisperTimeStampLogitsProcessor
    from transformers.generation.utils import GenerationMixin

    def decode_segment(segment_input, prompt, n_new, first):
        g = copy.deepcopy(gc)
        P = prompt.shape[1]
        procs = [SuppressTokensAtBeginLogitsProcessor(g.begin_suppress_tokens, begin_index=P, device="cpu"), SuppressTokensLogitsProcessor(g.suppress_tokens, device="cpu")]
        if timestamps:
            procs.append(WhisperTimeStampLogitsProcessor(g, begin_index=P))
        g.suppress_tokens = g.begin_suppress_tokens = None
        g.max_length, g.max_new_tokens = None, n_new
        return GenerationMixin.generate(model, segment_input, generation_config=g, logits_processor=procs, decoder_input_ids=prompt.contiguous())
    return decode_segment


SEGMENT_CALLS = [
    dict(max_length=20, language="en"),
    dict(max_new_tokens=12, language=["en", "de", "fr", "es", "en"], task="translate"),
    dict(max_length=30, language="en", return_timestamps=True),
    dict(max_length=14, language="de", return_timestamps=True, max_initial_timestamp_index=1),
    dict(max_new_tokens=30, language="en", return_timestamps=True),
]


@pytest.mark.parametrize("call", range(len(SEGMENT_CALLS)))
def test_segment_loop_returns_what_transformers_generate_returns(call):
    """`generate_segments` around transformers' own token loop == transformers' `generate`, exactly (dtype, shape, prompt columns stripped, EOS removed, right padding),
    B = 5, with and without timestamps, max_length (which transformers raises by the prompt length) and max_new_tokens, one language and one per row.  Call 3 closes
    segments (consecutive timestamp tokens) early in its windows, so `seek` moves, 17 windows are decoded and the batch shrinks as rows finish."""
    from huggingface_asr_amd.whisper import build_prompt, generate_segments, resolved_generation_config
    restore_generate()
    kw = dict(SEGMENT_CALLS[call])
    model = tiny_model(max_initial_timestamp_index=kw.pop("max_initial_timestamp_index", None), eos_token_id=2)
    x = features(5)
    with torch.no_grad():
        want = model.generate(input_features=x, **kw)
        gc = resolved_generation_config(model, None, kw)
        rt = bool(kw.get("return_timestamps"))
        init = torch.tensor(build_prompt(gc, model.config, 5, language=kw.get("language"), task=kw.get("task"), return_timestamps=rt))
        calls = []
        inner = _transformers_token_loop(model, gc, rt)

        def decode_segment(segment_input, prompt, n_new, first):
            calls.append((segment_input.shape[0], n_new, first))
            return inner(segment_input, prompt, n_new, first)
        got = generate_segments(gc, model.config, x, decode_segment, init_tokens=init)
    print(f"call {call}: windows decoded (rows, new tokens, first) {calls}; output {tuple(want.shape)}, row lengths {[int((r != 0).sum()) for r in want]}")
    assert got.dtype == want.dtype == torch.long and got.shape == want.shape and torch.equal(got, want), (got.tolist(), want.tolist())
    assert calls[0][2] is True and not any(c[2] for c in calls[1:])
    if call == 3:           # a closed pair early in the window: `seek` moves behind it, further windows are decoded, and rows that are through leave the batch
        assert len(calls) > 3 and len({c[0] for c in calls}) > 1, calls
