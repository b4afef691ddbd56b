"""CPU: Whisper beam search on the HIP path, host side — the shared reference loop (tests/whisper_beam_ref.py) against transformers' own `_beam_search` on the tiny
model, the opt-in routing (`generate_route(..., beams=True)`, `install_whisper(generate=True, beams=True)`, HFASR_WHISPER_BEAMS), and the new kernel's scratch-free build."""
import copy
import os
import re
import subprocess
import sys
import tempfile

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from whisper_beam_ref import beam_search_ref  # noqa: E402
from whisper_generate_common import NO_TIMESTAMPS, features, restore_generate, tiny_model  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS, PAD = 2, 0


@pytest.fixture(autouse=True)
def _generate_and_switch_as_found():
    """other modules assert that `generate` is transformers' own after a default binding and that num_beams > 1 is refused under HFASR_WHISPER_STRICT"""
    from huggingface_asr_amd import whisper as W
    said = set(W._stock_generate.said)
    yield
    restore_generate()
    W.BEAMS_ON_HIP = False
    W._stock_generate.said.clear()
    W._stock_generate.said.update(said)


# ------------------------------------------------------------------------------------------------------------------ 1. the reference loop is transformers' loop
def closing_model(scale=2.5, **gen):
    """the tiny model with the EOS row of the (tied) token embedding scaled: the stock one never emits EOS within 20 tokens (it repeats one token), this one closes
    hypotheses at different lengths, and whole utterances before max_length (scale 4 closes everything within three tokens, 1.5 hardly anything)"""
    model = tiny_model(**gen)
    with torch.no_grad():
        model.model.decoder.embed_tokens.weight[EOS] *= scale
    return model


def processors_for(gc, P, timestamps):
    from transformers.generation.logits_process import SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor, WhisperTimeStampLogitsProcessor
    procs = [SuppressTokensAtBeginLogitsProcessor(gc.begin_suppress_tokens, begin_index=P, device="cpu"), SuppressTokensLogitsProcessor(gc.suppress_tokens, device="cpu")]
    if timestamps:
        procs.append(WhisperTimeStampLogitsProcessor(gc, begin_index=P))
    return procs


def hf_step_fn(model, x, W):
    """transformers' own cached decoder forward on W-fold expanded encoder states: what `_beam_search` calls, cache re-ordering included"""
    from transformers.modeling_outputs import BaseModelOutput
    enc = BaseModelOutput(last_hidden_state=model.model.encoder(x).last_hidden_state.repeat_interleave(W, 0))
    st = {"cache": None}

    def step(new_tok, beam_idx):
        if beam_idx is not None:
            st["cache"].reorder_cache(beam_idx)
        out = model(encoder_outputs=enc, decoder_input_ids=new_tok, past_key_values=st["cache"], use_cache=True)
        st["cache"] = out.past_key_values
        return out.logits[:, -1].float()
    return step


def transformers_beam_search(model, x, prompt, W, n_new, timestamps, length_penalty, early_stopping):
    from transformers.generation.utils import GenerationMixin
    g = copy.deepcopy(model.generation_config)
    procs = processors_for(g, prompt.shape[1], timestamps)
    g.suppress_tokens = g.begin_suppress_tokens = None
    g.max_length, g.max_new_tokens = None, n_new
    return GenerationMixin.generate(model, x, generation_config=g, logits_processor=procs, decoder_input_ids=prompt, num_beams=W, length_penalty=length_penalty,
                                    early_stopping=early_stopping, return_dict_in_generate=True, output_scores=True)


def prompt_for(B, timestamps):
    rows = [[1, 100, 104], [1, 101, 104], [1, 102, 105]][:B]
    return torch.tensor([r + ([] if timestamps else [NO_TIMESTAMPS]) for r in rows], dtype=torch.long)


CALLS = [(W, ts, lp, es) for W in (2, 3, 5) for ts in (False, True) for lp, es in ((1.0, False), (0.5, True))] + [(3, False, 0.5, False), (3, True, 1.0, True)]


@pytest.fixture(scope="module")
def models():
    return dict(stock=tiny_model(max_initial_timestamp_index=3), closing=closing_model(max_initial_timestamp_index=3))


@pytest.mark.parametrize("which", ["stock", "closing"])
@pytest.mark.parametrize("W,timestamps,length_penalty,early_stopping", CALLS)
def test_reference_loop_is_transformers_loop(models, which, W, timestamps, length_penalty, early_stopping):
    """Sequences equal token for token, `sequences_scores` within 1e-6 absolute (4 fp32 ulps at |score| < 8, one ulp at the |score| of 13 that length_penalty 0.5
    reaches here: both sides evaluate one expression on the same cached forward), B = 3, 16 new tokens.  transformers fills its static buffers with
    `pad_token_id or eos_token_id` — EOS here, the pad id being 0 —, so behind a row's hypothesis its fill value is expected, not the pad id.  The `closing` model closes hypotheses before max_length (asserted below, on transformers' output alone)."""
    model = models[which]
    B, n_new = 3, 16
    x, prompt = features(B), prompt_for(B, timestamps)
    P = prompt.shape[1]
    with torch.no_grad():
        want = transformers_beam_search(model, x, prompt, W, n_new, timestamps, length_penalty, early_stopping)
        got = beam_search_ref(hf_step_fn(model, x, W), lambda l: torch.log_softmax(l, -1), processors_for(model.generation_config, P, timestamps), prompt, num_beams=W,
                              max_length=P + n_new, eos_token_id=EOS, pad_token_id=PAD, length_penalty=length_penalty, early_stopping=early_stopping)
    seq = want.sequences
    fill = PAD or EOS
    assert seq.shape[0] == B
    rows = [k[0][1] for k in got["kept"]]
    assert seq.shape[1] == max(len(r) for r in rows), (seq.tolist(), rows)
    for b, r in enumerate(rows):
        assert seq[b, :len(r)].tolist() == r and bool((seq[b, len(r):] == fill).all()), (b, seq[b].tolist(), r)
    assert float((want.sequences_scores - got["scores"]).abs().max()) <= 1e-6, (want.sequences_scores.tolist(), got["scores"].tolist())
    if which == "closing":
        closed_early = sum(1 for r in rows if r[-1] == EOS and len(r) < P + n_new)
        assert closed_early > 0, rows


def test_the_closing_model_closes_hypotheses_before_max_length():
    """On transformers alone: best hypotheses end in EOS before max_length, and utterances are done before max_length (the reference loop, which the test above holds to
    transformers, stops early).  How many hypotheses an utterance keeps is counted: under `_beam_search`'s rules an utterance is done only with W kept — the early-stop
    rule compares against -1e9 while fewer are kept, `early_stopping=True` waits for W, and at max_length the first W candidates all stop — unless its best running beam
    itself is at -1e9; none of these calls reaches that, so every count is W (a count below W would be a bug of the loop, not a case it misses)."""
    model = closing_model(max_initial_timestamp_index=3)
    x = features(3)
    short, early = [], 0
    for W, ts in ((3, False), (5, False), (5, True)):
        prompt = prompt_for(3, ts)
        P = prompt.shape[1]
        with torch.no_grad():
            want = transformers_beam_search(model, x, prompt, W, 16, ts, 1.0, False)
            got = beam_search_ref(hf_step_fn(model, x, W), lambda l: torch.log_softmax(l, -1), processors_for(model.generation_config, P, ts), prompt, num_beams=W,
                                  max_length=P + 16, eos_token_id=EOS, pad_token_id=PAD)
        eos_at = [(row[P:] == EOS).nonzero() for row in want.sequences]
        assert any(len(e) and int(e[0]) < 15 for e in eos_at), want.sequences.tolist()
        short += [len(k) for k in got["kept"] if len(k) < W]
        early += got["steps"] < 16
    print(f"utterances that ended with fewer than W kept hypotheses: {short}; calls that ended before max_length: {early} of 3")
    assert not short and early > 0


# ------------------------------------------------------------------------------------------------------------------ 2. routing
class _Cuda:
    is_cuda = True


def _route(model, beams, input_shape=(2, 80, 200), **kw):
    from huggingface_asr_amd.whisper import generate_route, resolved_generation_config
    gc = resolved_generation_config(model, None, kw)
    args = (dict(kw, input_features=kw.get("input_features", _Cuda())), gc, model.config, input_shape)
    return generate_route(*args, beams=True) if beams else generate_route(*args)


HANDED = {
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


def test_routing_is_opt_in():
    model = tiny_model()
    hip = ("hip", None)
    for why, kw in HANDED.items():                                     # beams off: the table of tests/test_whisper_generate_cpu.py, answer for answer
        assert _route(model, False, max_length=20, **kw) == ("stock", why), why
    assert _route(tiny_model(num_beams=4), False, max_length=20) == ("stock", "num_beams > 1")
    assert _route(model, False, max_length=20) == hip and _route(model, True, max_length=20) == hip
    for why, kw in HANDED.items():                                     # beams on: only the beam reason goes
        assert _route(model, True, max_length=20, **kw) == (hip if why == "num_beams > 1" else ("stock", why)), why
    assert _route(model, True, max_length=20, num_beams=2) == hip
    assert _route(tiny_model(num_beams=4), True, max_length=20) == hip                             # the trainer sets generation_config.num_beams
    assert _route(model, True, max_length=20, num_beams=64, length_penalty=0.5, early_stopping="never", num_return_sequences=1, return_timestamps=True, language="en") == hip
    assert _route(model, True, max_length=20, num_beams=3, early_stopping=True) == hip
    route, why = _route(model, True, max_length=20, num_beams=65)
    assert route == "stock" and "device beam loop" in why and why != "num_beams > 1"
    assert _route(model, True, max_length=20, num_beams=2, num_return_sequences=2) == ("stock", "generation_config.num_return_sequences")
    assert _route(model, True, max_length=20, num_beams=2, do_sample=True) == ("stock", "sampling")
    assert _route(model, True, (2, 80, 600), max_length=20, num_beams=2)[1].startswith("long-form input")
    assert _route(model, True, max_length=20, num_beams=2, num_beam_groups=2)[0] == "stock"


def test_install_sets_and_resets_the_switch(monkeypatch):
    from transformers.models.whisper import modeling_whisper as MW
    from huggingface_asr_amd import bind
    from huggingface_asr_amd import whisper as W
    cls = MW.WhisperForConditionalGeneration
    restore_generate()
    assert W.BEAMS_ON_HIP is False
    W.install_whisper(generate=True, beams=True)
    assert W.BEAMS_ON_HIP is True and cls.generate is W.hip_whisper_generate
    W.install_whisper()                                                 # a default binding leaves the switch alone
    assert W.BEAMS_ON_HIP is True
    W.install_whisper(generate=True)
    assert W.BEAMS_ON_HIP is False and cls.generate is W.hip_whisper_generate
    with pytest.raises(ValueError):
        W.install_whisper(beams=True)
    # with the switch on a beam call passes the routing (and stops at the CPU tensors); with it off it is refused as before
    model, x = tiny_model(), features(2)
    monkeypatch.setenv("HFASR_WHISPER_STRICT", "1")
    W.install_whisper(generate=True, beams=True)
    with pytest.raises(NotImplementedError, match="CPU tensors"):
        model.generate(input_features=x, max_length=12, num_beams=2, language="en")
    W.install_whisper(generate=True)
    with pytest.raises(NotImplementedError, match="num_beams > 1"):
        model.generate(input_features=x, max_length=12, num_beams=2, language="en")
    with pytest.raises(NotImplementedError, match="num_beams > 1"):
        W.hip_generate(model, x, max_new_tokens=4, num_beams=2)         # the greedy entry keeps refusing beams
    # the environment: HFASR_WHISPER_BEAMS=1 implies generate
    restore_generate()
    monkeypatch.delenv("HFASR_WHISPER_GENERATE", raising=False)
    monkeypatch.setenv("HFASR_WHISPER_BEAMS", "1")
    bind.bind_all()
    assert cls.generate is W.hip_whisper_generate and W.BEAMS_ON_HIP is True
    monkeypatch.delenv("HFASR_WHISPER_BEAMS")
    monkeypatch.setenv("HFASR_WHISPER_GENERATE", "1")
    bind.bind_all()
    assert cls.generate is W.hip_whisper_generate and W.BEAMS_ON_HIP is False


def test_beam_decode_refuses_what_the_device_loop_does_not_serve():
    """before anything is enqueued: the checks come before the first device call, so CPU tensors reach them only past the device-tensor check — given here as stand-ins"""
    from huggingface_asr_amd.whisper import beam_decode

    class Eng:
        cfg = dict(vocab_size=120)
        device = "cpu"
    prompt = type("T", (), dict(is_cuda=True, shape=(2, 4)))()
    with pytest.raises(NotImplementedError, match="64 beams"):
        beam_decode(None, Eng(), prompt, prompt, max_new_tokens=4, eos_token_id=2, pad_token_id=0, num_beams=65)
    Eng.cfg = dict(vocab_size=1 << 22)
    with pytest.raises(NotImplementedError):
        beam_decode(None, Eng(), prompt, prompt, max_new_tokens=4, eos_token_id=2, pad_token_id=0, num_beams=4)
    with pytest.raises(ValueError, match="num_beams >= 2"):
        beam_decode(None, Eng(), prompt, prompt, max_new_tokens=4, eos_token_id=2, pad_token_id=0, num_beams=1)
    with pytest.raises(RuntimeError, match="device tensors"):
        beam_decode(None, Eng(), torch.zeros(2, 80, 200), torch.ones(2, 4, dtype=torch.long), max_new_tokens=4, eos_token_id=2, pad_token_id=0, num_beams=2)


def test_step_denoms_with_a_prompt():
    """the length-penalty denominators: `_step_denoms` with the prompt length in place of 1 is transformers' (cur_len + 1 - P) ** lp and, for "never" with a positive
    penalty, (max_length - P) ** lp; with the default it is what it was"""
    import numpy as np
    from huggingface_asr_amd.decoder import _step_denoms
    f = lambda v: float(np.float32(v))
    for lp in (1.0, 0.5, 2.0):
        assert _step_denoms(7, 20, lp, False, prompt_len=4) == (f(4 ** lp), f(4 ** lp))
        assert _step_denoms(7, 20, lp, "never", prompt_len=4) == (f(4 ** lp), f(16 ** lp))
        assert _step_denoms(7, 20, lp, False) == (f(7 ** lp), f(7 ** lp)) and _step_denoms(7, 20, lp, "never") == (f(7 ** lp), f(19 ** lp))
    assert _step_denoms(7, 20, -1.0, "never", prompt_len=4) == (f(0.25), f(0.25))


# ------------------------------------------------------------------------------------------------------------------ 3. the kernel's build
def test_new_kernel_is_declared_bound_and_uses_no_scratch():
    """the entry in the header, the binding and the built library; in the gfx950 code object the kernel has no private segment (no spills, no per-thread arrays in
    memory) and a few words of LDS"""
    from huggingface_asr_amd import _lib
    header = open(os.path.join(ROOT, "include", "hfasr_hip.h")).read()
    assert re.search(r"\bint mi_whisper_beam_scores\(", header) and "mi_whisper_beam_scores" in _lib.SIGNATURES and hasattr(_lib.lib(), "mi_whisper_beam_scores")
    so = os.path.join(ROOT, "huggingface_asr_amd", "libhfasr_hip.so")
    llvm = "/opt/rocm/lib/llvm/bin"
    found = {}
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "lib.fatbin"), os.path.join(td, "lib.co")
        subprocess.run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fb], check=True)
        blob = open(fb, "rb").read()                                   # one bundle per translation unit, back to back
        starts = [m.start() for m in re.finditer(re.escape(magic), blob)]
        for lo, hi in zip(starts, starts[1:] + [len(blob)]):
            if b"whisper_beam_scores_kernel" not in blob[lo:hi]:
                continue
            with open(fb, "wb") as f:
                f.write(blob[lo:hi])
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}",
                            f"--output={co}"], check=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for block in notes.split("- .agpr_count")[1:]:
                name = re.search(r"\.name:\s+(\S*whisper_beam_scores_kernel\S*)", block)
                if name:
                    num = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))
                    found[name.group(1)] = (num("private_segment_fixed_size"), num("group_segment_fixed_size"), num("vgpr_count"))
    assert len(found) == 1, sorted(found)
    for name, (scratch, lds, vgprs) in found.items():
        assert scratch == 0 and lds <= 256 and vgprs <= 128, (name, scratch, lds, vgprs)
