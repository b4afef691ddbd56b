"""The end-to-end case of two-pass joint decoding shared by tests/test_rescore_cpu.py (which certifies it with the CPU oracle) and tests/test_gpu_rescore.py: the
`gen_tiny` model and inputs (helpers.gen_case_inputs), 5 beams, the 5 best kept.

One entry of the fixture's weights is changed: the CTC head's blank bias.  tests/gen_model.py sets it to 6.0 so that `generate`'s prefix scorer does not veto the
end-of-sequence token; with it the CTC head's 5-best holds the empty hypothesis and four one-token ones, for the fixture's inputs and for every one of 40 other
feature seeds tried (each of the model's ~50 classes alone is likelier than any pair of them) — nothing for a rescoring pass to rank.  At BLANK_BIAS = 2.0 the same
model's 5-best are distinct transcripts of 7 to 12 tokens, which is what a trained CTC head yields."""
import functools

import gen_model as GM
import rescore_ref as RR
from helpers import AED_JCFG, gen_case_inputs
from huggingface_asr_amd import shapes

ENC = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean")
BLANK_BIAS = 2.0
W, NBEST, CTC_WEIGHT, LENGTH_PENALTY, MAX_LENGTH = 5, 5, 0.3, 1.0, 14
SHORT_MAX_LENGTH = 13        # U = 12: the hypotheses of 12 tokens do not fit
# the oracle gap between ranks 1 and 2 above which the device's top-1 must be the oracle's in fp32 precision: twice the 1e-3 per-token bar at length_penalty = 1 (the
# totals are per-token means: each of the two may move by the bar) plus slack for the CTC term (1e-3, tests/test_gpu_ctc_beam.py's score bound, times ctc_weight / length)
TOP1_GAP = 5e-3


@functools.lru_cache(maxsize=None)
def end_to_end_case(max_length=MAX_LENGTH):
    import torch
    g, sd, x, am, dec_cfg = gen_case_inputs("gen_tiny")
    sd = dict(sd)
    sd["encoder.blank_projection.bias"] = torch.full((1,), BLANK_BIAS)
    oracle = RR.two_pass_oracle(sd, ENC, dec_cfg, AED_JCFG, x, am, num_beams=W, nbest=NBEST, ctc_weight=CTC_WEIGHT, length_penalty=LENGTH_PENALTY, max_length=max_length,
                                eos=GM.EOS)
    return dict(sd=sd, x=x, am=am, dec_cfg=dec_cfg, oracle=oracle)
