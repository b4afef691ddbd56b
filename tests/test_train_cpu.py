"""CPU tests of the training step's host logic (no kernels): the flat parameter store's packed layout <-> the reference's
state-dict names, the weight-decay mask (HF Trainer rule), and the data-parallel gradient all-reduce over gloo, world size 2."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from huggingface_asr_amd import shapes, synth
from huggingface_asr_amd.train import GradSync, ParamStore, _enc_map, encoder_specs


def _sd(cfg, seed=3):
    return {k: torch.from_numpy(v) for k, v in synth.state_dict_numpy(shapes.param_shapes(cfg), seed).items()}


@pytest.mark.parametrize("extra", [{}, {"position_embeddings_type": "rotary"}])
def test_packed_layout_roundtrips_every_reference_parameter(extra):
    """ParamStore's reference-name API on CPU (`pack` is `load` without the bf16 mirror refresh, which runs on the GPU)."""
    cfg = dict(shapes.TINY, **extra)
    sd = _sd(cfg)
    store = ParamStore(encoder_specs(cfg), "cpu", _enc_map(cfg))
    assert set(store.export("p")) == set(sd)                          # before any load nothing is skipped
    store.pack(sd)
    covered = store.export("p")
    assert set(covered) == set(sd), (sorted(set(sd) - set(covered))[:5], sorted(set(covered) - set(sd))[:5])
    for k, v in sd.items():
        assert covered[k].shape == v.shape and torch.equal(covered[k], v), k
    # offsets are 64-element aligned (16-B aligned bf16 rows for the GEMM loads), ranges do not overlap
    offs = sorted((store.off[n], n) for n in store.order)
    for (o, n), (o2, _) in zip(offs, offs[1:]):
        assert o % 64 == 0 and o + torch.Size(store.specs[n].shape).numel() <= o2
    # one piece in / out by reference key, parameters and gradients; a piece of a packed concatenation exports but does not import alone
    wo, wq = "wav2vec2.encoder.layers.0.self_attn.linear_out.weight", "wav2vec2.encoder.layers.0.self_attn.linear_q.weight"
    for which, view in (("p", store.p), ("g", store.g)):
        new = torch.randn_like(sd[wo])
        store.import_piece(wo, new, which)
        assert torch.equal(view("l0.att_wo"), new) and torch.equal(store.export_piece(wo, which), new)
    assert torch.equal(store.export_piece(wq), sd[wq])
    for bad in ("no.such.key", wq):
        with pytest.raises(KeyError):
            store.import_piece(bad, sd[wq])
    with pytest.raises(KeyError):
        store.export_piece("no.such.key")
    # aliasing views: every piece but the front end's re-ordered `out` Linear is a view of the flat store
    fe_out = "wav2vec2.feature_extractor.out.weight"
    for which, flat in (("p", store.flat_p), ("g", store.flat_g)):
        views = store.alias_views(which, prefix="m.")
        assert set(views) == {"m." + k for k in sd} and views["m." + fe_out] is None
        for k, v in views.items():
            assert k == "m." + fe_out or (v.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
                                         and torch.equal(v, store.export_piece(k[2:], which))), k
    # the optional SpecAugment vector: absent from the loaded state dict -> zeros, and neither exported nor aliased
    mse = "wav2vec2.masked_spec_embed"
    store.pack({k: v for k, v in sd.items() if k != mse})
    assert not store.p("masked_spec_embed").any()
    assert set(store.export("p")) == set(sd) - {mse} and set(store.alias_views("g")) == set(sd) - {mse}


def test_weight_decay_mask_follows_hf_trainer_rule():
    """HF Trainer: decay everything except LayerNorm parameters and names containing 'bias' (so pos_bias_u / pos_bias_v are excluded)."""
    cfg = dict(shapes.TINY)
    specs = {s.name: s for s in encoder_specs(cfg)}
    assert specs["l0.ff1_w1"].decay and specs["conv1_w"].decay and specs["l0.csgu_w"].decay and specs["l1.mrg_dw_w"].decay and specs["head_w"].decay
    for n in ("l0.ff1_b1", "l0.att_ln_g", "l0.att_ln_b", "l0.att_u", "l0.att_v", "head_b", "enc_ln_g", "l1.csgu_ln_g", "conv2_b"):
        assert not specs[n].decay, n
    store = ParamStore(list(specs.values()), "cpu")
    o = store.off["l0.ff1_w1"]
    assert int(store.decay[o]) == 1 and int(store.decay[store.off["l0.ff1_b1"]]) == 0


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    from huggingface_asr_amd import parallel as P
    P.init("gloo")
    n = 1000
    for overlap in (False, True):                                     # one merged collective after the backward / one per bucket as it is final
        flat = torch.arange(n, dtype=torch.float32) * (rank + 1)      # stand-in for this rank's flat gradient
        sync = GradSync(flat, overlap=overlap)
        assert sync.on and sync.world == world and sync.overlap == overlap
        for lo, hi in ((768, 1000), (256, 768), (0, 256)):           # head bucket, layer buckets in reverse order, front end
            sync.launch(lo, hi)
        assert len(sync.pending) == (3 if overlap else 0)
        sync.wait()
        assert not sync.pending and sync._span is None
        out[(rank, overlap)] = flat.clone()
    P.barrier()
    torch.distributed.destroy_process_group()


def test_gradsync_gloo_world2_sums_every_bucket():
    world, port = 2, _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    want = torch.arange(1000, dtype=torch.float32) * 3
    for key in ((0, False), (1, False), (0, True), (1, True)):
        assert torch.equal(out[key], want), key


def test_gradsync_single_process_is_a_noop():
    flat = torch.ones(10)
    s = GradSync(flat)
    s.launch(0, 10); s.wait()
    assert not s.on and s.world == 1 and torch.equal(flat, torch.ones(10))


def test_decoder_layout_roundtrips_reference_names():
    """GPT-2 Conv1D weights are stored (in, out) in the reference: packed as (out, in) rows for the GEMM, transposed back on export."""
    from helpers import TINY_DEC
    from huggingface_asr_amd.train_aed import _dec_map, decoder_specs
    for fixed in (False, True):
        c = dict(TINY_DEC, pos_emb_fixed=fixed, tie_word_embeddings=False)
        d, V, L = c["n_embd"], c["vocab_size"], c["n_layer"]
        sd = {"enc_to_dec_proj.weight": torch.randn(d, 64), "enc_to_dec_proj.bias": torch.randn(d), "decoder.lm_head.weight": torch.randn(V, d),
              "decoder.additional_lm_heads.0.weight": torch.randn(V, d), "decoder.transformer.ln_f.weight": torch.randn(d), "decoder.transformer.ln_f.bias": torch.randn(d)}
        if fixed:
            sd["decoder.transformer.wte.emb_layers.0.weight"] = torch.randn(V, d)
        else:
            sd["decoder.transformer.wte.weight"] = torch.randn(V, d); sd["decoder.transformer.wpe.weight"] = torch.randn(c["n_positions"], d)
        for l in range(L):
            r = f"decoder.transformer.h.{l}."
            for n, shp in (("ln_1", None), ("ln_cross_attn", None), ("ln_2", None)):
                sd[r + n + ".weight"] = torch.randn(d); sd[r + n + ".bias"] = torch.randn(d)
            for n, (i, o) in (("attn.c_attn", (d, 3 * d)), ("attn.c_proj", (d, d)), ("crossattention.q_attn", (d, d)), ("crossattention.c_attn", (d, 2 * d)),
                              ("crossattention.c_proj", (d, d)), ("mlp.c_fc", (d, 4 * d)), ("mlp.c_proj", (4 * d, d))):
                sd[r + n + ".weight"] = torch.randn(i, o); sd[r + n + ".bias"] = torch.randn(o)
        store = ParamStore(decoder_specs(c, 64, True), "cpu", _dec_map(c, True))
        store.pack(sd)
        covered = store.export("p")
        assert set(covered) == set(sd)
        for k, v in sd.items():
            assert torch.equal(covered[k], v), k
        assert store.specs["h0.wqkv"].shape == (3 * d, d) and store.specs["h0.wpr"].shape == (d, 4 * d)


def test_dbd_static_buffers_are_a_three_entry_lru_of_zero_filled_buffers():
    """ops_train._dbd_static (the sparse-writes attention backward's dBD buffers) on the host: at most three shapes are held, a shape in use returns the same
    storage, the least recently used goes first, and a buffer made again after its eviction is all zeros.  (Host memory of this size comes from fresh pages, which
    read as zero anyway: a `torch.empty` in place of the zero fill passes here and is caught by tests/test_gpu_train_shapes.py, where freed memory holds NaN bits.)"""
    from huggingface_asr_amd import ops_train as OT
    saved = dict(OT._DBD_CACHE)
    OT.release_static_buffers()
    try:
        cpu = torch.device("cpu")
        a = OT._dbd_static(cpu, 4, 2, 25, 64)
        assert a.shape == (4, 2, 25, 64) and a.dtype == torch.bfloat16 and not bool(a.any())
        b = OT._dbd_static(cpu, 4, 3, 75, 160)
        c = OT._dbd_static(cpu, 4, 2, 128, 288)
        a.fill_(1.0); b.fill_(2.0)                                  # what a launch leaves behind
        assert OT._dbd_static(cpu, 4, 2, 25, 64).data_ptr() == a.data_ptr()     # a is now the most recently used: b is the oldest
        assert len(OT._DBD_CACHE) == 3
        OT._dbd_static(cpu, 4, 2, 129, 288)                         # a fourth shape evicts b
        assert len(OT._DBD_CACHE) == 3
        assert [k[1:] for k in OT._DBD_CACHE] == [(4, 2, 128, 288), (4, 2, 25, 64), (4, 2, 129, 288)]
        assert OT._dbd_static(cpu, 4, 2, 128, 288).data_ptr() == c.data_ptr()
        assert OT._dbd_static(cpu, 4, 2, 25, 64).data_ptr() == a.data_ptr() and bool((a == 1.0).all())    # kept buffers are not cleared
        b2 = OT._dbd_static(cpu, 4, 3, 75, 160)                     # b again: made anew, all zeros; the oldest (129) went
        assert b2.shape == b.shape and not bool(b2.any()) and b2.data_ptr() != b.data_ptr()
        assert [k[1:] for k in OT._DBD_CACHE] == [(4, 2, 128, 288), (4, 2, 25, 64), (4, 3, 75, 160)]
        OT._dbd_static(torch.device("meta"), 4, 2, 25, 64)          # the device is part of the key
        assert [k[1:] for k in OT._DBD_CACHE] == [(4, 2, 25, 64), (4, 3, 75, 160), (4, 2, 25, 64)] and len({k[0] for k in OT._DBD_CACHE}) == 2
    finally:
        OT.release_static_buffers()
        OT._DBD_CACHE.update(saved)
