"""Writes tests/golden/gen_tiny_mix.npz: the REFERENCE's `GPT2LMMultiHeadModelMixing` (src/models/decoders/multi_head_gpt2_mixing.py) inside its joint model on the
`gen_tiny` model of tests/golden/make_golden.py `gen`, with the structured additional head and the seeded, non-uniform mixing parameters of tests/mix_ref.py.

    python tests/golden/make_gen_mix.py          (needs the reference checkout make_golden.py points at; CPU only)

The decoder is a subclass of the reference's mixing class with the two harness shims make_golden.py `build_reference_aed` applies to the plain decoder (the `tie_weights`
signature, the holder that restores the cross mask).  Stored per mode (`scalar`, `linear`, `full`), for greedy, 3 and 5 beams at ctc_weight 0.3: sequences, sequence
scores, the smallest decision margin; the teacher-forced mixed logits with labels absent at B = 2; `dec_loss` and `loss` at B = 1 (the only batch size at which the
reference's loss is defined: :128 indexes `lm_logits[-1]`) and, for `linear` / `scalar`, autograd's `d lm_mixing` there.  One `average_logits=True` case of the plain
decoder: its logits, its greedy and its 3-beam decode (the greedy one alone is the plain decoder's).  Asserted here, on the reference side alone: (a) every mode's decode differs from the plain decoder's (gen_tiny.npz) in at least
one row; (b) the fp32 restatement tests/mix_ref.py reproduces every stored sequence, and agrees with its bf16 storage model (folded matrix) token for token on at least
half of the (setting, utterance) decodes."""
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
import mix_ref as MR  # noqa: E402

SETTINGS = [(1, 1.0, False, 14), (3, 1.0, False, 14), (5, 1.0, False, 14)]


def _swap_decoder(model, mode, average_logits):
    """the reference's mixing decoder (or, mode None, its plain decoder with `average_logits`) with the harness shims, in the place of the joint model's decoder"""
    import transformers.models.gpt2.modeling_gpt2 as mg
    from models.decoders.multi_head_gpt2 import GPT2LMMultiHeadModel, GPT2MultiHeadConfig
    from models.decoders.multi_head_gpt2_mixing import GPT2LMMultiHeadModelMixing, GPT2MultiHeadMixingConfig
    from transformers.models.gpt2.modeling_gpt2 import GPT2LMHeadModel
    base = GPT2LMMultiHeadModelMixing if mode is not None else GPT2LMMultiHeadModel

    class Dec(base):
        model_parallel = False

        def tie_weights(self, *a, **k):
            return GPT2LMHeadModel.tie_weights(self, *a, **k)

    old = model.decoder.config.to_dict()
    old.pop("model_type", None)
    if mode is not None:
        cfg = GPT2MultiHeadMixingConfig(**old, mixing_mode=mode)
    else:
        old["average_logits"] = average_logits
        cfg = GPT2MultiHeadConfig(**old)
    dec = Dec(cfg).eval()
    dec.load_state_dict(model.decoder.state_dict(), strict=False)
    holder = {}
    orig_forward = dec.forward

    def fwd(*a, **k):
        holder["mask"] = k.get("encoder_attention_mask")
        return orig_forward(*a, **k)

    def bidir(config=None, inputs_embeds=None, attention_mask=None, encoder_hidden_states=None, **kw):
        m = holder.get("mask")
        if m is None:
            return None
        return (1.0 - m[:, None, None, :].to(inputs_embeds.dtype)) * torch.finfo(inputs_embeds.dtype).min

    dec.forward = fwd
    mg.create_bidirectional_mask = bidir
    model.decoder = dec
    return model


def main():
    from decoding.config import GenerationConfigCustom
    from helpers import AED_JCFG
    from huggingface_asr_amd import shapes
    from oracle import aed_ref as A
    from oracle import generate_ref as G
    torch.set_num_threads(8)
    name = "gen_tiny"
    seed, fixed, lengths = GM.CASES[name]
    adapt, rec = _install_generate_adapters()
    B, T = len(lengths), 200
    x, am = synth_feats(seed, B, T, lengths)
    x, am = torch.from_numpy(x), torch.from_numpy(am)
    base = np.load(os.path.join(HERE, f"{name}.npz"))
    enc = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")
    lab = torch.tensor([[5, 17, 30, 9, 22, 41, 12, 1]])
    out = dict(seed=seed, labels=lab.numpy())
    same = total = 0
    for mode, avg in (("scalar", False), ("linear", False), ("full", False), (None, True)):
        model = adapt(build_reference_aed(fixed))
        load_seeded(model, seed)
        model.load_state_dict(GM.overrides(seed, fixed), strict=False)
        model = _swap_decoder(model, mode, avg)
        ov = MR.overrides(seed, mode, fixed)
        missing, unexpected = model.load_state_dict(ov, strict=False)
        assert not unexpected, unexpected
        model.eval()
        tag = mode or "average"
        sd, _, _, dec_cfg = MR.mix_case_inputs(mode, avg)
        # teacher-forced mixed logits, labels absent, B = 2
        ids = torch.tensor([[2, 5, 17, 30, 9, 22], [2, 8, 40, 3, 50, 50]])
        with torch.no_grad():
            eo = model.encoder(x, attention_mask=am, output_hidden_states=True, return_dict=True)
            hid = eo.last_hidden_state if hasattr(eo, "last_hidden_state") and eo.last_hidden_state is not None else eo.hidden_states[-1]
            hid = model.enc_to_dec_proj(hid) if hasattr(model, "enc_to_dec_proj") else hid
            emask = model.encoder._get_feature_vector_attention_mask(hid.shape[1], am)
            lg = model.decoder(input_ids=ids, encoder_hidden_states=hid, encoder_attention_mask=emask).logits
        out[f"{tag}/ids"], out[f"{tag}/logits"] = ids.numpy(), lg.numpy()
        if mode is not None:                                            # loss at B = 1 (+ autograd's gradient of the mix)
            for p in model.parameters():
                p.requires_grad_(False)
            mixp = [p for n, p in model.named_parameters() if "lm_mixing" in n]
            for p in mixp:
                p.requires_grad_(True)
            o = model(input_values=x[:1, :lengths[0]], attention_mask=am[:1, :lengths[0]], labels=lab)
            out[f"{tag}/dec_loss"], out[f"{tag}/loss"], out[f"{tag}/enc_loss"] = np.float32(o.dec_loss.item()), np.float32(o.loss.item()), np.float32(o.enc_loss.item())
            if mode in ("linear", "scalar"):
                o.dec_loss.backward()
                out[f"{tag}/dmix"] = model.decoder.lm_mixing.grad.numpy().copy()
            print(tag, "B = 1: dec_loss", float(o.dec_loss), "loss", float(o.loss))
        changed = 0
        for W, lp, es, ml in (SETTINGS if mode is not None else SETTINGS[:2]):
            g = GenerationConfigCustom(bos_token_id=GM.START, pad_token_id=GM.PAD, decoder_start_token_id=GM.START, length_penalty=lp, early_stopping=es,
                                       eos_token_id=GM.EOS, max_length=ml, num_beams=W, ctc_weight=0.3, ctc_margin=0, lm_weight=0, lm_model=None, space_token_id=-1,
                                       apply_eos_space_trick=False, eos_space_trick_weight=1.0)
            model.generation_config = g
            g.num_return_sequences, g.return_dict_in_generate, g.output_scores = W, True, True
            rec["margin"].clear(); rec["stop_gap"].clear()
            with torch.no_grad():
                o = model.generate(generation_config=g, input_values=x, attention_mask=am)
            key = f"{tag}/" + GM.setting_key(W, lp, es, ml)
            seqs = o.sequences.numpy()
            out[key + "/sequences"] = seqs
            if W > 1:
                out[key + "/sequences_scores"] = o.sequences_scores.numpy()
                out[key + "/min_margin"] = np.float32(min(min(m) for m in rec["margin"]))
            plain = base[GM.setting_key(W, lp, es, ml) + "/sequences"]
            L = max(plain.shape[1], seqs.shape[1])
            differs = (MR.np_pad(plain, L, GM.PAD) != MR.np_pad(seqs, L, GM.PAD)).any(1)
            changed += int(differs.sum())
            assert differs.any() or mode is None, (key, "the mix does not change this setting's output")          # (a); `average_logits`: over its two settings, below
            res = []
            for q in (None, A.E.bf16_round):                                                        # (b)
                with MR.patched():
                    fn, nb = G.joint_score_fn(sd, enc, dec_cfg, AED_JCFG, x, am, W, 0.3, q=q)
                    if W == 1:
                        res.append(G.greedy(fn, nb, max_length=ml, eos=GM.EOS, pad=GM.PAD, start=GM.START))
                    else:
                        res.append(G.beam_search(fn, nb, W, GM.V, max_length=ml, eos=GM.EOS, pad=GM.PAD, start=GM.START, length_penalty=lp, early_stopping=es)[0])
            a, b = res
            if W == 1:                                                                              # the greedy margin, from the restatement that reproduces the decode
                with MR.patched():
                    fn, nb = G.joint_score_fn(sd, enc, dec_cfg, AED_JCFG, x, am, 1, 0.3)
                    tr = {}
                    G.beam_search(fn, nb, 1, GM.V, max_length=ml, eos=GM.EOS, pad=GM.PAD, start=GM.START, trace=tr)
                out[key + "/min_margin"] = np.float32(min(float(m.min()) for m in tr["margin"]))
            assert a.shape == seqs.shape and (a == seqs).all(), (key, "the fp32 restatement does not reproduce the reference", a, seqs)
            L = max(a.shape[1], b.shape[1])
            for u in range(nb):
                total += 1
                same += int((MR.np_pad(a, L, GM.PAD)[u * W:(u + 1) * W] == MR.np_pad(b, L, GM.PAD)[u * W:(u + 1) * W]).all())
            print(key, "rows changed by the mix:", int(differs.sum()), "of", len(differs), "margin", float(out.get(key + "/min_margin", np.float32("nan"))))
        assert changed > 0, (tag, "the heads beside lm_head do not change a decode")
    print(f"certification: {same} of {total} decodes agree between the fp32 restatement and its bf16 storage model")
    assert 2 * same >= total
    out["certified_same"], out["certified_total"] = np.int64(same), np.int64(total)
    np.savez_compressed(os.path.join(HERE, f"{name}_mix.npz"), **out)
    print("written", f"{name}_mix.npz")


if __name__ == "__main__":
    main()
