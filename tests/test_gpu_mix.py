"""GPU: DeCRED head mixing on the HIP path — the token step with a multi-tap head (mi_decoder_step_taps) in every step form, the plain decoder's bits through the old
entries, teacher-forced mixed logits and the evaluation loss against the CPU restatement (tests/mix_ref.py), and `generate` / `generate_stepwise` with the three mixing
modes and `average_logits` through `certified_decode` of tests/test_gpu_generate.py (token for token up to a decision the reference trajectory certifies as a near tie)."""
import numpy as np
import pytest
import torch

import gen_model as GM
import mix_cases as MC
import mix_ref as MR
from helpers import AED_JCFG, TINY_DEC, load_golden, synth_labels
from huggingface_asr_amd import shapes, synth
from oracle import aed_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENC = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")
# (mixing mode, average_logits) of the decoding cases
VARIANTS = [("scalar", False), ("linear", False), ("full", False), (None, True)]
SETTINGS = [(1, 1.0, False, 14), (3, 1.0, False, 14), (5, 1.0, False, 14)]          # greedy, 3 and 5 beams (ctc_weight 0.3)


def test_plain_decoder_keeps_its_bits_through_the_old_entries():
    """mi_gpt2_step / mi_decoder_step_beams share their body with the new entry: a plain decoder's logits are the ones recorded on the commit before it, bit for bit, in
    every form and on both sides of every form boundary (tests/golden/step_plain_bits.npz, written by tests/mix_cases.py `plain_bits`)"""
    want = load_golden("step_plain_bits")
    got = MC.plain_bits(DEV)
    assert sorted(got) == sorted(want.files)
    for k, v in got.items():
        assert np.array_equal(v, want[k]), (k, float(np.abs(v - want[k]).max()))


def _tap_engine(locs, mode):
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    H, V = len(locs) + 1, TINY_DEC["vocab_size"]
    cfg = dict(TINY_DEC, head_locations=list(locs), head_weights=[0.3, 0.2, 0.5][:H] if H == 3 else [0.4, 0.6], mixing_mode=mode, average_logits=mode is None)
    sd = MC.decoder_sd(locs)
    u = lambda name, *sh: torch.from_numpy(synth.uniform(MC.SEED, name, sh, -0.2, 0.2))
    if mode == "scalar":
        sd["decoder.lm_mixing"] = 0.5 + u("taps/scalar", H)
    elif mode == "linear":
        sd["decoder.lm_mixing"] = 0.5 + u("taps/linear", H, V)
    elif mode == "full":
        sd["decoder.lm_mixing.weight"] = torch.eye(V).repeat(1, H) * 0.5 + 0.1 * u("taps/full_w", V, H * V)
        sd["decoder.lm_mixing.bias"] = u("taps/full_b", V)
    eng = GPT2DecoderEngine(cfg, DEV)
    eng.load_state_dict(sd)
    return eng


@pytest.mark.parametrize("locs,mode", [([1], "full"), ([0, 3], "linear"), ([3], "scalar"), ([1], None)])
def test_taps_step_against_the_python_step(locs, mode):
    """mi_decoder_step_taps against `step_py` from the same folded weights: 1, 8, 9, 64, 65 rows and 2 utterances x 40 hypotheses on shared cross K/V — both sides of the
    8-row limit of the GEMV form and of the 64-row limit of the streaming form — a 3-token prompt at past = 0 and one token at past > 0, tap sets that read the embedding
    output, a middle layer and ln_f (twice: [3] taps what lm_head reads).  Tolerance: what tests/test_gpu_aed.py holds `step` to against `step_py`."""
    eng = _tap_engine(locs, mode)
    assert eng.w["taps"] == list(locs) + [3] and eng.w["head_fold"].shape == (51, (len(locs) + 1) * 128)
    for M, beams in MC.ROWS:
        want = MC.step_case(eng, M, beams, python=True)
        for form in ([0, 2] if beams == 1 else [0]):
            got = MC.step_case(eng, M, beams, form)
            for a, b, what in zip(got, want, ("prompt", "next")):
                assert a.shape == (M, 51) and bool(torch.isfinite(a).all())
                torch.testing.assert_close(a, b, atol=3e-2, rtol=0, msg=lambda m: f"rows {M} beams {beams} form {form} {what}: {m}")
    # the mix is not a no-op: the same weights without it give other logits
    from huggingface_asr_amd.decoder import GPT2DecoderEngine
    plain = GPT2DecoderEngine(dict(eng.cfg, mixing_mode=None, average_logits=False), DEV)
    plain.load_state_dict(MC.decoder_sd(locs))
    assert float((MC.step_case(plain, 9, 1)[1] - MC.step_case(eng, 9, 1)[1]).abs().max()) > 0.1


def _joint_engine(sd, dec_cfg):
    from huggingface_asr_amd.decoder import JointAEDEngine
    eng = JointAEDEngine(ENC, dec_cfg, AED_JCFG, DEV)
    eng.load_state_dict(sd)
    return eng


def _labels():
    lab = synth_labels(GM.CASES["gen_tiny"][0], 2, 9, GM.V - 1, [9, 5])          # ragged; the CTC loss shares them: below the blank / pad id
    lab[0, 8] = GM.V - 2
    return lab


@pytest.mark.parametrize("mode,avg", VARIANTS)
def test_teacher_forced_mixed_logits_and_evaluation_loss(mode, avg):
    """labels absent: the folded multi-tap head against the restatement — the reference's arithmetic (fp32, per-head products mixed) at the tolerance tests/test_gpu_aed.py
    applies to decoder logits against the reference, and the bf16 storage model at its tighter one.  With labels (no grad): the plain shifted cross-entropy of the mixed
    logits over every non-ignored position of B = 2 ragged utterances, per-head logits mixed in fp32, at that file's tolerance for the losses."""
    from huggingface_asr_amd.decoder import shift_tokens_right
    sd, x, am, dec_cfg = MR.mix_case_inputs(mode, avg)
    eng = _joint_engine(sd, dec_cfg)
    lab = _labels()
    fl = am.sum(-1).to(DEV, torch.int32)
    enc_out, enc_bf, T2, key_len = eng.encode(x.to(DEV), fl)
    ids = shift_tokens_right(lab, AED_JCFG["pad_token_id"], AED_JCFG["decoder_start_token_id"]).to(DEV)
    got = eng.dec.forward(ids, enc_bf, T2, key_len)["logits"].cpu().numpy()

    def no_labels(sd_, pre, cfg, ids_, enc, mask, labels=None, q=A._id, dm=None):
        return torch.tensor(0.0), MR.decoder_forward(sd_, pre, cfg, ids_, enc, mask, None, q, dm)[1]
    A.decoder_forward = no_labels
    try:
        with torch.no_grad():
            ref = A.joint_forward(sd, ENC, dec_cfg, AED_JCFG, x, am, lab)["logits"].numpy()
            refq = A.joint_forward(sd, ENC, dec_cfg, AED_JCFG, x, am, lab, q=A.E.bf16_round)["logits"].numpy()
    finally:
        A.decoder_forward = MR._ORIGINAL
    dl, dq = np.abs(got - ref), np.abs(got - refq)
    print(f"{mode} avg={avg}: logits vs fp32 max {dl.max():.4f} mean {dl.mean():.5f}; vs bf16 storage model max {dq.max():.4f} mean {dq.mean():.5f}")
    assert dl.max() < 0.08 and dl.mean() < 0.012, (dl.max(), dl.mean())
    assert dq.max() < 0.04 and dq.mean() < 0.004, (dq.max(), dq.mean())
    # the mix changes the logits: the same weights through lm_head alone are elsewhere
    with torch.no_grad():
        plain = A.joint_forward(sd, ENC, dict(dec_cfg, mixing_mode=None, average_logits=False), AED_JCFG, x, am, lab)["logits"].numpy()
    assert np.abs(plain - ref).max() > 1.0
    # the reference's own numbers (tests/golden/gen_tiny_mix.npz): its mixed logits for the fixture's decoder input at B = 2, its losses at B = 1
    g = load_golden("gen_tiny_mix")
    tag = mode or "average"
    got = eng.dec.forward(torch.from_numpy(g[f"{tag}/ids"]).to(DEV), enc_bf, T2, key_len)["logits"].cpu().numpy()
    df = np.abs(got - g[f"{tag}/logits"])
    print(f"{tag}: logits vs the reference fixture max {df.max():.4f} mean {df.mean():.5f}")
    assert df.max() < 0.08 and df.mean() < 0.012, (df.max(), df.mean())
    if mode is None:
        return                                                      # average_logits only acts with labels absent (multi_head_gpt2.py:129)
    n = int(am[0].sum())
    one = eng.forward(x[:1, :n].to(DEV), fl[:1], torch.from_numpy(g["labels"]).to(DEV))
    for k in ("loss", "enc_loss", "dec_loss"):
        print("B = 1", k, float(one[k]), float(g[f"{tag}/{k}"]))
        assert abs(float(one[k]) - float(g[f"{tag}/{k}"])) < 2e-3 * abs(float(g[f"{tag}/{k}"])), (k, float(one[k]), float(g[f"{tag}/{k}"]))
    out = eng.forward(x.to(DEV), fl, lab.to(DEV))
    with MR.patched(), torch.no_grad():
        want = A.joint_forward(sd, ENC, dec_cfg, AED_JCFG, x, am, lab)
    for k in ("loss", "enc_loss", "dec_loss"):
        print(k, float(out[k]), float(want[k]))
        assert abs(float(out[k]) - float(want[k])) < 2e-3 * abs(float(want[k])), (k, float(out[k]), float(want[k]))
    assert np.abs(out["logits"].cpu().numpy() - want["logits"].numpy()).max() < 0.08


@pytest.mark.parametrize("mode,avg", VARIANTS)
def test_generate_against_the_restated_reference_trajectory(mode, avg):
    """`generate` (greedy, device beam loop) with a mixing decoder through `certified_decode`: the device's bookkeeping exact, its candidate values the restatement's within
    TOL, tokens equal along the reference trajectory up to a certified near tie (a decision outside one fails inside `certified_decode`); and `generate_stepwise` gives the
    same hypotheses.  The trajectory is the reference's: the restatement's decode equals tests/golden/gen_tiny_mix.npz.  A setting whose smallest decision margin in the
    fixture exceeds 2 TOL has no near tie to certify: there every utterance must stay on the trajectory.  The count of exact decodes is printed, not bounded: beam
    search on this model takes decisions with margins down to 0.003 (the fixture's `min_margin`), far inside bf16 noise.  The mix changes decisions: the decode differs
    from the plain decoder's fixture."""
    from test_gpu_generate import TOL, certified_decode
    from huggingface_asr_amd.decoder import generate_stepwise
    torch.set_num_threads(8)
    sd, x, am, dec_cfg = MR.mix_case_inputs(mode, avg)
    eng = _joint_engine(sd, dec_cfg)
    assert eng.dec.w["taps"] == [1, 3]
    base = load_golden("gen_tiny")
    g, tag = load_golden("gen_tiny_mix"), mode or "average"
    fl = am.sum(-1).to(DEV, torch.int32)
    exact = total = changed = 0
    for W, lp, es, ml in (SETTINGS if mode is not None else SETTINGS[:2]):
        with MR.patched():
            got, (ref_seq, ref_sc), diverged, worst = certified_decode(eng, sd, ENC, dec_cfg, AED_JCFG, x, am, W, lp, es, ml, GM.EOS)
        plain = base[GM.setting_key(W, lp, es, ml) + "/sequences"]
        L = max(plain.shape[1], ref_seq.shape[1])
        changed += int((MR.np_pad(plain, L, GM.PAD) != MR.np_pad(ref_seq, L, GM.PAD)).any(1).sum())
        total += len(diverged)
        exact += sum(not d for d in diverged)
        want = g[f"{tag}/" + GM.setting_key(W, lp, es, ml) + "/sequences"]           # the trajectory followed IS the reference's (also asserted on the CPU)
        assert ref_seq.shape == want.shape and (ref_seq == want).all(), (W, ref_seq, want)
        if W > 1:                                                   # the reference's own hypothesis scores, for the utterances that stayed on its trajectory
            want_sc = g[f"{tag}/" + GM.setting_key(W, lp, es, ml) + "/sequences_scores"]
            assert np.abs(ref_sc - want_sc).max() < 1e-4
            for b in range(len(diverged)):
                if not diverged[b]:
                    dev_sc = np.array([s_ for s_, _ in got[b]["hypotheses"]])
                    assert np.abs(dev_sc - want_sc[b * W:(b + 1) * W]).max() < TOL, (W, b, dev_sc, want_sc[b * W:(b + 1) * W])
        if float(g[f"{tag}/" + GM.setting_key(W, lp, es, ml) + "/min_margin"]) > 2 * TOL:
            assert not any(diverged), (W, "every decision of this setting is wider than a certifiable near tie, yet the device left the reference's trajectory")
        step = generate_stepwise(eng, x.to(DEV), fl, num_beams=W, max_length=ml, ctc_weight=0.3, length_penalty=lp, early_stopping=es, eos_token_id=GM.EOS)
        assert [h["hypotheses"] for h in step] == [h["hypotheses"] for h in got], (W, "generate_stepwise differs from generate")
        print(f"{mode} avg={avg} W={W}: worst candidate value error {worst:.4f}, diverged {diverged}")
    print(f"{mode} avg={avg}: {exact} of {total} utterance decodes equal the restated reference token for token; rows changed by the mix: {changed}")
    assert changed > 0, "the mix does not change a decision"


def test_model_surface_swap_rebuilds_the_engine_and_decodes():
    """the statements of model_utils.py:205-217 on a HIP joint model that has already decoded: `model.decoder = new_decoder` rebuilds the engine for the mixing decoder
    (the folded head follows in-place updates of `lm_mixing`), `generate()` returns the engine's tokens and the evaluation forward returns the three losses"""
    from test_mix_cpu import _swap
    from test_surface_cpu import _joint_model
    from huggingface_asr_amd.decoder import generate
    from huggingface_asr_amd.decoding import GenerationConfigCustom
    sd, x, am, dec_cfg = MR.mix_case_inputs("linear")
    model = _joint_model(False)
    missing, unexpected = model.load_state_dict({k: v for k, v in sd.items() if "lm_mixing" not in k}, strict=False)
    assert not missing and not unexpected
    model = model.to(DEV).eval()
    model.generation_config = GenerationConfigCustom(pad_token_id=GM.PAD, eos_token_id=GM.EOS, decoder_start_token_id=GM.START, bos_token_id=GM.START, num_beams=3,
                                                     max_length=14, ctc_weight=0.3, ctc_margin=0, lm_weight=0, lm_model=None, space_token_id=-1,
                                                     apply_eos_space_trick=False, eos_space_trick_weight=1.0, length_penalty=1.0, early_stopping=False)
    before = model.generate(input_values=x.to(DEV), attention_mask=am.to(DEV))
    assert model._get_engine(DEV).dec.w["taps"] is None
    model = _swap(model, "linear").to(DEV)
    uniform = model.generate(input_values=x.to(DEV), attention_mask=am.to(DEV))
    assert model._get_engine(DEV).dec.w["taps"] == [1, 3]
    with torch.no_grad():
        model.decoder.lm_mixing.copy_(sd["decoder.lm_mixing"])
    toks = model.generate(input_values=x.to(DEV), attention_mask=am.to(DEV))
    ref = generate(_joint_engine(sd, dec_cfg), x.to(DEV), am.sum(-1).to(DEV, torch.int32), num_beams=3, max_length=14, ctc_weight=0.3, eos_token_id=GM.EOS)
    for b in range(2):
        n = len(ref[b]["tokens"])
        assert toks[b, :n].tolist() == ref[b]["tokens"] and bool((toks[b, n:] == GM.PAD).all())
    assert before.shape[0] == uniform.shape[0] == 2
    assert before.tolist() != toks.tolist() or uniform.tolist() != toks.tolist()
    lab = _labels()
    with torch.no_grad():
        out = model(input_values=x.to(DEV), attention_mask=am.to(DEV), labels=lab.to(DEV))
    with MR.patched(), torch.no_grad():
        want = A.joint_forward(sd, ENC, dec_cfg, AED_JCFG, x, am, lab)
    for k in ("loss", "enc_loss", "dec_loss"):
        assert abs(float(getattr(out, k)) - float(want[k])) < 2e-3 * abs(float(want[k])), k
