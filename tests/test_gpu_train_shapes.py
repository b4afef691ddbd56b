"""GPU: training and inference over a sequence of batch shapes, as the length-grouped recipes feed them (`--group_by_length`, `--pad_to_multiples_of=100`:
every batch is padded to its own multiple of 100 frames, so T changes from step to step and shapes come back in no fixed order).

The state the trainers and the engine keep between calls depends on the shape: the sparse-writes attention backward's zero-filled dBD buffers (ops_train._dbd_static,
a three-entry LRU), the LnReduceBatch arena that grows part-way through a backward, the `_dw_ws` scratch, the position tables, TnBatch's overwrite -> accumulate
transition, the engine's resident workspace, its position-projection cache and the LayerNorm-fold switch.  The backward is bit-reproducible, so the yardstick is
strict: a call on an object that has seen other shapes gives the same bits as a fresh object given the same state and batch; and it matches the CPU oracle at the
suite's usual bars.  Before every call the caching allocator's free blocks are filled with NaN bits (`_scribble`), so that a buffer read before it is written shows."""
import numpy as np
import pytest
import torch

from helpers import AED_JCFG, TINY_DEC, aed_case_inputs, compare_grads, load_golden, oracle_ctc_grads, seeded_state_dict, synth_feats, synth_labels
from huggingface_asr_amd import ops_train as OT
from huggingface_asr_amd import shapes
from oracle import ebranchformer_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NO_DROPOUT = dict(hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0, final_dropout=0.0, feat_proj_dropout=0.0,
                  csgu_conv_dropout=0.0, apply_spec_augment=False, layerdrop=0.0)
# head size 64 (the fused attention path); intermediate 1024: the causal CSGU's tap partials, B ceil(T2 / 64) x 512 x 32 floats, outgrow the LayerNorm slots
# (512 x 2 x 256) at B = 6, T2 = 175, so the LnReduceBatch arena is re-allocated part-way through that backward
CFG = dict(shapes.TINY, hidden_size=256, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4, vocab_size=32,
           ctc_zero_infinity=True, ctc_loss_reduction="mean")

# (B, T, frame lengths, label lengths): T a multiple of 100 and every length 1-99 frames short of it, except the 512 / 516 pair (T2 = 128 / 129, a 128 edge)
CTC_SEQ = [
    (4, 300, [299, 287, 262, 231], [6, 5, 6, 4]),                    # T2 75
    (4, 100, [100, 97, 81, 52], [4, 6, 3, 2]),                       # T2 25: less than one 32-row tile
    (3, 512, [512, 470, 430], [6, 5, 6]),                            # T2 128
    (2, 516, [516, 489], [5, 6]),                                    # T2 129
    (6, 700, [700, 688, 671, 650, 633, 602], [6, 6, 5, 4, 6, 3]),    # T2 175: four keys since (4, 75), which the LRU has evicted
    (4, 300, [211, 208, 205, 202], [4, 3, 5, 2]),                    # (4, 75) comes back, much shorter than its last use
    (6, 700, [640, 620, 611, 605, 603, 601], [5, 6, 4, 3, 6, 5]),    # a cached shape, shorter than its last use: the walk re-zeroes what that one wrote
    (1, 400, [377], [5]),                                            # the last batch of an epoch
]
ACC_PAIR = [(3, 200, [200, 180, 121], [5, 4, 6]), (2, 400, [390, 333], [6, 5])]          # two backwards into one gradient, at two shapes
STEP_SEQ = [(2, 516, [500, 455], [6, 4]), (4, 100, [91, 88, 70, 64], [3, 5, 4, 2]), (3, 300, [300, 250, 210], [6, 6, 5])]

CTC_CASES = {"relative": {}, "relative_causal": {"is_causal": True}, "rotary": {"position_embeddings_type": "rotary"}}


def _scribble():
    """Give the allocator back its whole free segments, fill every free block left with 0xFF bytes (NaN in bf16 and fp32), then free them again: memory handed out
    next holds NaN until written, and a buffer dropped part-way through the next call (an LnReduceBatch arena that grows) is what the allocator hands out after it.
    Largest first with exact block sizes: the allocator's best fit then hands out each free block itself."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    keep = torch.empty(512, dtype=torch.uint8, device=DEV)             # a live block and a freed one beside it: there is always at least one free block to find
    probe = torch.empty(512, dtype=torch.uint8, device=DEV)
    del probe
    idx = torch.device(DEV).index or 0
    sizes = sorted((b["size"] for seg in torch.cuda.memory_snapshot() if seg["device"] == idx for b in seg["blocks"] if b["state"] == "inactive"), reverse=True)
    assert sizes, "no free block found in torch.cuda.memory_snapshot(): its layout changed and nothing would be filled"
    held = [torch.empty(s, dtype=torch.uint8, device=DEV).fill_(255) for s in sizes]
    torch.cuda.synchronize()
    del held, keep


def _batch(seed, case, vocab):
    B, T, lens, tl = case
    assert len(lens) == len(tl) == B and max(lens) <= T
    x, am = synth_feats(seed, B, T, lens)
    lab = synth_labels(seed, B, max(tl), vocab, tl)
    return x, am, lab


def _fresh_statics():
    """what a new process starts with: no static dBD buffer, no partial-sum scratch"""
    OT.release_static_buffers()
    OT._DW_WS.clear()


class _AsideStatics:
    """runs a block (a fresh reference trainer) with empty module-level caches and puts the caller's back afterwards, untouched"""
    def __enter__(self):
        self.dbd, self.ws = dict(OT._DBD_CACHE), dict(OT._DW_WS)
        _fresh_statics()

    def __exit__(self, *exc):
        _fresh_statics()
        OT._DBD_CACHE.update(self.dbd)
        OT._DW_WS.update(self.ws)


def _ctc_trainer(cfg, sd, sparse=True):
    from huggingface_asr_amd.train import EncoderCTCTrainer
    tr = EncoderCTCTrainer(dict(cfg, **NO_DROPOUT), DEV, lr=1e-3, weight_decay=1e-2)
    tr.sparse_attn_bwd = sparse
    tr.load_state_dict(sd)
    return tr


def _run(tr, batches):
    """zero_grad, then one forward_backward per batch -> (losses, logits, flat gradient)"""
    _scribble()
    for st in tr.stores():
        st.zero_grad()
    losses, logits = [], []
    for x, am, lab in batches:
        o = tr.forward_backward(x.to(DEV), am.sum(-1).to(DEV), lab.to(DEV))
        losses.append(float(o["loss"]))
        logits.append(o.get("encoder_logits", o.get("logits")).float().clone())
    torch.cuda.synchronize()
    return losses, logits, [st.flat_g.clone() for st in tr.stores()]


def _assert_same(tr, got, want, what):
    (gl, glog, gg), (wl, wlog, wg) = got, want
    assert gl == wl, (what, gl, wl)
    for a, b in zip(glog, wlog):
        assert a.shape == b.shape and torch.equal(a, b), (what, "logits", int((a != b).sum()), float((a - b).abs().nan_to_num(1e30).max()))
    for st, a, b in zip(tr.stores(), gg, wg):
        if not torch.equal(a, b):
            off = [n for n in st.order if not torch.equal(a[slice(*st.range_of([n]))], b[slice(*st.range_of([n]))])]
            raise AssertionError(f"{what}: {int((a != b).sum())} of {a.numel()} gradient elements differ, in {off[:8]}")


def _dbd_keys():
    return [k[2:4] for k in OT._DBD_CACHE]                 # (B, T2) of the static dBD buffers, least recently used first


@pytest.mark.parametrize("case", list(CTC_CASES))
def test_ctc_trainer_over_a_recipe_shape_sequence(case):
    cfg = dict(CFG, **CTC_CASES[case])
    sd = seeded_state_dict(cfg, 61)
    seq = [_batch(100 + i, c, cfg["vocab_size"]) for i, c in enumerate(CTC_SEQ)]
    acc = [_batch(200 + i, c, cfg["vocab_size"]) for i, c in enumerate(ACC_PAIR)]
    steps = [_batch(300 + i, c, cfg["vocab_size"]) for i, c in enumerate(STEP_SEQ)]

    # the fresh references first: a new trainer and empty module caches for every batch, with the sparse-writes dBD walk and with the dense one
    refs = []
    for batches in [[b] for b in seq] + [acc]:
        r = []
        for sparse in (True, False):
            _fresh_statics()
            tr = _ctc_trainer(cfg, sd, sparse)
            r.append(_run(tr, batches))
            del tr
        refs.append(r)
    _fresh_statics()
    if case != "rotary":
        # the dBD buffers as a model of the other kind left them (causal <-> non-causal, one process-wide cache keyed by shape alone): the first three shapes of
        # the sequence start on buffers the other walk wrote
        ocfg = dict(cfg, is_causal=not cfg.get("is_causal", False))
        other = _ctc_trainer(ocfg, seeded_state_dict(ocfg, 62))
        for b in seq[:3]:
            _run(other, [b])
        del other
        assert _dbd_keys() == [(4, 75), (4, 25), (3, 128)], _dbd_keys()

    # one trainer through the whole sequence, nothing cleared in between
    tr = _ctc_trainer(cfg, sd)
    for i, batches in enumerate([[b] for b in seq] + [acc]):
        if i == 5 and case != "rotary":
            assert (4, 75) not in _dbd_keys() and (6, 175) in _dbd_keys(), _dbd_keys()       # the sequence does what it is meant to: (4, 75) was evicted
        got = _run(tr, batches)
        _assert_same(tr, got, refs[i][0], (case, i, "vs a fresh trainer"))
        _assert_same(tr, got, refs[i][1], (case, i, "vs a fresh trainer with dense dBD writes"))
        want_loss, want = 0.0, None
        for k, (x, am, lab) in enumerate(batches):
            loss_ref, g = oracle_ctc_grads(cfg, sd, x, am, lab)
            assert abs(got[0][k] - loss_ref) <= 2e-3 * abs(loss_ref), (case, i, k, got[0][k], loss_ref)
            want = g if want is None else {n: want[n] + g[n] for n in want}
        compare_grads(tr.grad_dict(), want, rel=0.04)

    # optimizer steps at a new shape every step, each against a fresh trainer given the whole pre-step state (parameters, both moments, step counts)
    for i, (x, am, lab) in enumerate(steps):
        pre = [(st.flat_p.clone(), st.flat_m.clone(), st.flat_v.clone(), st.step_count) for st in tr.stores()]
        assert i == 0 or all(st.step_count == i for st in tr.stores())
        with _AsideStatics():
            ref = _ctc_trainer(cfg, sd)
            for st, (p, m, v, n) in zip(ref.stores(), pre):
                st.flat_p.copy_(p); st.flat_m.copy_(m); st.flat_v.copy_(v)
                st.step_count = n
                st.refresh_mirrors(cast=True)
            _scribble()
            ro = ref.train_step(x.to(DEV), am.sum(-1).to(DEV), lab.to(DEV))
            want = (float(ro["loss"]), float(ro["grad_norm"]), ref.last_step_flags.clone(), [(st.flat_p.clone(), st.flat_m.clone(), st.flat_v.clone()) for st in ref.stores()])
            del ref, ro
        _scribble()
        o = tr.train_step(x.to(DEV), am.sum(-1).to(DEV), lab.to(DEV))
        torch.cuda.synchronize()
        assert (float(o["loss"]), float(o["grad_norm"])) == want[:2], (case, "step", i, float(o["loss"]), float(o["grad_norm"]), want[:2])
        assert torch.equal(tr.last_step_flags, want[2]), (case, i, tr.last_step_flags, want[2])
        assert float(want[2][0]) > 0 and float(want[2][2]) == 0.0                     # a real, applied step
        for st, (p, m, v) in zip(tr.stores(), want[3]):
            for a, b, what in ((st.flat_p, p, "parameters"), (st.flat_m, m, "first moments"), (st.flat_v, v, "second moments")):
                assert torch.equal(a, b), (case, "step", i, what, int((a != b).sum()))
    OT.release_static_buffers()


# (B, T, frame lengths, label lengths): the decoder's causal self-attention at a new Tq = U and its cross-attention at a new Tk = T2 every step
AED_SEQ = [
    (3, 300, [300, 280, 251], [12, 9, 7]),          # T2 75 (not a multiple of 32)
    (2, 100, [100, 77], [2, 1]),                    # T2 25, U of 1-2 tokens
    (2, 500, [500, 470], [40, 36]),                 # T2 125, U > 32
    (3, 300, [240, 230, 211], [5, 4, 3]),           # T2 75 again, shorter
]


def test_joint_aed_trainer_over_changing_frame_and_label_lengths():
    from huggingface_asr_amd.train_aed import JointAEDTrainer
    from oracle import aed_ref as A
    sd, _, _, _ = aed_case_inputs(load_golden("grads_aed_tiny"))
    enc_cfg = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean", **NO_DROPOUT)
    dec_cfg = dict(TINY_DEC, pos_emb_fixed=False, tie_word_embeddings=False)
    seq = [_batch(400 + i, c, enc_cfg["vocab_size"]) for i, c in enumerate(AED_SEQ)]

    def trainer():
        tr = JointAEDTrainer(enc_cfg, dec_cfg, AED_JCFG, DEV)
        tr.load_state_dict(sd)
        return tr

    refs = []
    for b in seq:
        _fresh_statics()
        refs.append(_run(trainer(), [b]))
    _fresh_statics()
    tr = trainer()
    for i, (x, am, lab) in enumerate(seq):
        _scribble()
        tr.enc.store.zero_grad(); tr.store.zero_grad()
        o = tr.forward_backward(x.to(DEV), am.sum(-1).to(DEV), lab.to(DEV))
        torch.cuda.synchronize()
        got = ([float(o["loss"])], [o["encoder_logits"].float().clone()], [st.flat_g.clone() for st in tr.stores()])
        _assert_same(tr, got, refs[i], ("aed", i, "vs a fresh trainer"))
        sdr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        w = A.joint_forward(sdr, enc_cfg, dec_cfg, AED_JCFG, x, am, lab)
        w["loss"].backward()
        for key in ("loss", "enc_loss", "dec_loss"):
            want = float(w[key].detach())
            assert abs(float(o[key]) - want) <= 2e-3 * abs(want) + 1e-3, (i, key, float(o[key]), want)
        compare_grads(tr.grad_dict(), {k: v.grad for k, v in sdr.items() if v.grad is not None}, rel=0.04)
    OT.release_static_buffers()


# (B, T) per call.  "head64_fold": B T2 just over / under the LayerNorm-fold threshold of 2048 rows, a short batch, the first shape again (its position projections
# were evicted), then a weight change that load_state_dict records and the same shapes again.  "head16": head size 16 (the attention reads V^T of the
# time-padded layout, whose columns T2 .. Tp only the workspace's zero fill clears) over workspace-key changes onto smaller shapes with T2 = 50, 75, 100.
ENG_CASES = {
    "head64_fold": (CFG, [(16, 516), (16, 508), (2, 300), (16, 516), "reload", (16, 516), (2, 300)], [True, False, False, True, True, False]),
    "head16": (dict(shapes.TINY), [(2, 516), (3, 200), (4, 300), (1, 400), "reload", (3, 200), (2, 300)], [False] * 6),
}


@pytest.mark.parametrize("case", list(ENG_CASES))
def test_engine_forward_over_a_shape_sequence(case):
    from huggingface_asr_amd.engine import EBranchformerEngine
    cfg, seq, want_folds = ENG_CASES[case]
    sds = [seeded_state_dict(cfg, 71), seeded_state_dict(cfg, 72)]
    eng = EBranchformerEngine(cfg, DEV)
    assert eng.ln_fold is None and eng._fold_shapes_ok() == any(want_folds)
    eng.load_state_dict(sds[0])
    w, folds, oracle = 0, [], {}

    def engine(fold=None):
        e = EBranchformerEngine(cfg, DEV)
        e.ln_fold = fold
        e.load_state_dict(sds[w])
        return e

    for i, step in enumerate(seq):
        if step == "reload":
            w = 1
            eng.load_state_dict(sds[1])
            continue
        B, T = step
        rng = np.random.default_rng(500 + i)
        lens = np.sort(T - rng.integers(0, 99, size=B))[::-1].copy()
        lens[0] = T
        x, am = synth_feats(500 + T, B, T, [int(v) for v in lens])
        feats, fl = x.to(DEV), am.sum(-1).to(DEV, torch.int32)
        T2 = eng.out_frames(T)
        folds.append(eng._use_fold(B, T2))
        ref = engine()
        _scribble()
        want = ref.forward(feats, fl)
        want = {k: want[k].clone() for k in ("logits", "last_hidden", "inner_len", "outer_len")}
        del ref
        cs = eng._config_struct(B, T, 80)
        if eng._ws.get("key") not in (None, (cs.B, cs.T, cs.F, cs.ln_fold, cs.wide_tiles)):
            for slot, buf in eng._ws.items():          # what the resident workspace holds from the last shape, made deterministic (NaN / Inf bits): a call at a new
                if slot != "key":                      # key must not depend on it
                    buf.fill_(255)
        _scribble()
        got = eng.forward(feats, fl)
        torch.cuda.synchronize()
        for k, v in want.items():
            assert torch.equal(got[k], v), (case, i, step, k, int((got[k] != v).sum()))
        key = (w, B, T, tuple(int(v) for v in lens))
        if key not in oracle:
            with torch.no_grad():
                oracle[key] = R.ctc_head(sds[w], R.encoder_forward(sds[w], cfg, x, am, q=R.bf16_round), q=R.bf16_round)
        plain = got["logits"]
        if folds[-1]:
            # folded LayerNorms: the plain path of the same engine against the oracle, and the folded path against the plain one at test_gpu_encoder's fold-vs-plain bar
            plain = engine(False).forward(feats, fl)["logits"]
            dd = (got["logits"] - plain).abs()
            assert float(dd.max()) < 0.05 and float(dd.mean()) < 0.006, (case, i, step, float(dd.max()), float(dd.mean()))
        dq = (plain.float().cpu() - oracle[key]).abs()
        assert float(dq.max()) < 0.03 and float(dq.mean()) < 0.003, (case, i, step, float(dq.max()), float(dq.mean()))
    assert folds == want_folds, folds
