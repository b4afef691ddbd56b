"""Writes tests/golden/gen_tiny_lm.npz: the REFERENCE's own `generate()` with shallow-fusion LM rescoring (`LMRescorerLogitsProcessor`, src/decoding/shallow_fussion.py,
appended behind the CTC processor by src/models/ctc_encoder_plus_autoregressive_decoder.py:398-403) on the `gen_tiny` model of tests/golden/make_golden.py `gen`, with the
structured GPT-2 LM of tests/lm_model.py as `lm_model` and `lm_weight = 0.5`, decoded the way `do_generate` asks (src/utilities/general_utils.py:198-218).

    python tests/golden/make_gen_lm.py          (needs the reference checkout make_golden.py points at; CPU only, a few seconds per setting)

Settings: tests/lm_model.py SETTINGS — greedy and 3 / 5 beams at ctc_weight 0.3, and greedy / 5 beams at ctc_weight 0 (no CTC processor: no pad mask, greedy adds the LM
term to raw logits).  Stored per setting: sequences, sequence scores (beams), the loop's smallest decision margin.  Asserted here, on the reference side alone:
  (a) the LM matters: every setting's output differs from the same call with lm_weight = 0 (which, at ctc_weight 0.3, is gen_tiny.npz's);
  (b) the certification cap of tests/test_gpu_lm_fusion.py: the oracle loop on the fp32 score function + fp32 LM and on the bf16 storage model + bf16-rounded LM matrices
      agree token for token on at least half of the (setting, utterance) decodes."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import _install_generate_adapters, build_reference_aed, load_seeded, synth_feats  # noqa: E402

import gen_model as GM  # noqa: E402
import lm_model as LM  # noqa: E402


def main():
    from decoding.config import GenerationConfigCustom
    from helpers import AED_JCFG, gen_case_inputs
    from huggingface_asr_amd import shapes
    from oracle import aed_ref as A
    from oracle import generate_ref as G
    torch.set_num_threads(8)
    name = "gen_tiny"
    seed, fixed, lengths = GM.CASES[name]
    adapt, rec = _install_generate_adapters()
    model = adapt(build_reference_aed(fixed))
    load_seeded(model, seed)
    missing, unexpected = model.load_state_dict(GM.overrides(seed, fixed), strict=False)
    assert not unexpected, unexpected
    model.eval()
    B, T = len(lengths), 200
    x, am = synth_feats(seed, B, T, lengths)
    lm = LM.tiny_lm()
    base = np.load(os.path.join(HERE, f"{name}.npz"))
    out = dict(seed=seed, lm_seed=LM.SEED, lm_weight=np.float32(LM.LM_WEIGHT), lm_param_sum=np.float64(sum(float(p.double().sum()) for p in lm.parameters())))

    def run(W, lp, es, ml, cw, lm_weight):
        g = GenerationConfigCustom(bos_token_id=GM.START, pad_token_id=GM.PAD, decoder_start_token_id=GM.START, length_penalty=lp, early_stopping=es, eos_token_id=GM.EOS,
                                   max_length=ml, num_beams=W, ctc_weight=cw, ctc_margin=0, lm_weight=lm_weight, lm_model=lm if lm_weight > 0 else None, space_token_id=-1,
                                   apply_eos_space_trick=False, eos_space_trick_weight=1.0)
        model.generation_config = g                                           # train_enc_dec_asr.py:85
        g.num_return_sequences, g.return_dict_in_generate, g.output_scores = W, True, True     # general_utils.py:198-201
        rec["margin"].clear(); rec["stop_gap"].clear()
        with torch.no_grad():
            return model.generate(generation_config=g, input_values=torch.from_numpy(x), attention_mask=torch.from_numpy(am))

    for W, lp, es, ml, cw in LM.SETTINGS:
        key = LM.setting_key(W, lp, es, ml, cw)
        o = run(W, lp, es, ml, cw, LM.LM_WEIGHT)
        seqs = o.sequences.numpy()
        out[key + "/sequences"] = seqs
        if W > 1:
            out[key + "/sequences_scores"] = o.sequences_scores.numpy()
            out[key + "/min_margin"] = np.float32(min(min(m) for m in rec["margin"]))
        else:
            gaps = []
            for t, sc in enumerate(o.scores):
                top2 = sc.topk(2, dim=1).values
                for b in range(B):
                    if t == 0 or (seqs[b, t] != GM.EOS and seqs[b, t] != GM.PAD):
                        gaps.append(float(top2[b, 0] - top2[b, 1]))
            out[key + "/min_margin"] = np.float32(min(gaps))
        # (a) the LM matters
        plain = run(W, lp, es, ml, cw, 0).sequences.numpy()
        if cw == 0.3:
            want = base[GM.setting_key(W, lp, es, ml) + "/sequences"]
            assert plain.shape == want.shape and (plain == want).all(), key
        L = max(plain.shape[1], seqs.shape[1])
        pad_to = lambda a: np.pad(a, ((0, 0), (0, L - a.shape[1])), constant_values=GM.PAD)
        differs = (pad_to(plain) != pad_to(seqs)).any(1)
        assert differs.any(), (key, "the LM does not change this setting's output")
        print(key, "margin", float(out[key + "/min_margin"]), "rows changed by the LM:", int(differs.sum()), "of", len(differs))
        for i, s in enumerate(seqs.tolist()):
            print("    ", s, float(o.sequences_scores[i]) if W > 1 else "")

    # (b) fp32 oracle + fp32 LM against the bf16 storage model + bf16-rounded LM matrices
    _, sd, x_t, am_t, dec_cfg = gen_case_inputs(name)
    enc = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    same = total = 0
    for W, lp, es, ml, cw in LM.SETTINGS:
        res = []
        for q in (None, A.E.bf16_round):
            fn, nb = G.joint_score_fn(sd, enc, dec_cfg, AED_JCFG, x_t, am_t, W, cw, q=q)
            fn = LM.with_lm(fn, lm, LM.LM_WEIGHT, q)
            if W == 1:
                res.append(G.greedy(fn, nb, max_length=ml, eos=GM.EOS, pad=GM.PAD, start=GM.START))
            else:
                res.append(G.beam_search(fn, nb, W, GM.V, max_length=ml, eos=GM.EOS, pad=GM.PAD, start=GM.START, length_penalty=lp, early_stopping=es)[0])
        key = LM.setting_key(W, lp, es, ml, cw)
        a, b = res
        assert a.shape == out[key + "/sequences"].shape and (a == out[key + "/sequences"]).all(), (key, "the fp32 oracle loop does not reproduce the reference")
        L = max(a.shape[1], b.shape[1])
        pad_to = lambda t: np.pad(t, ((0, 0), (0, L - t.shape[1])), constant_values=GM.PAD)
        for u in range(nb):
            total += 1
            same += int((pad_to(a)[u * W:(u + 1) * W] == pad_to(b)[u * W:(u + 1) * W]).all())
    print(f"certification cap: {same} of {total} decodes agree between the fp32 and the bf16 storage model")
    assert 2 * same >= total
    out["certified_same"], out["certified_total"] = np.int64(same), np.int64(total)
    np.savez_compressed(os.path.join(HERE, f"{name}_lm.npz"), **out)
    print("written", f"{name}_lm.npz")


if __name__ == "__main__":
    main()
