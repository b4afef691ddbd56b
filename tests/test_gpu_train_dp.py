"""Data-parallel training step on the GPU box: two ranks (two processes sharing the one GPU of the box, gloo process group —
RCCL needs one device per rank) each run forward+backward on HALF the batch with the trainer's per-layer gradient all-reduce;
the synchronised gradients must equal the full-batch gradients of the reference fixture (mean reduction: the average of the
per-rank gradients IS the full-batch gradient), and both ranks must hold identical weights after the optimizer step."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out, name="grads_tiny_rel", overlap=False):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here); sys.path.insert(0, os.path.dirname(here))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0",
                      HFASR_DP_OVERLAP="1" if overlap else "0")
    import torch.distributed as dist
    from helpers import case_inputs, load_golden
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.train import EncoderCTCTrainer
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    g = load_golden(name)
    cfg = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean", hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0,
               final_dropout=0.0, feat_proj_dropout=0.0, csgu_conv_dropout=0.0, apply_spec_augment=False, layerdrop=0.0)
    if "flags" in g.files:          # the CTC fine-tuning head: its gradient ranges (head, additional layer, encoder LayerNorm + mixing weights) are reduced too
        cfg.update(finetune_with_additional_layer=bool(g["flags"][0]), finetune_with_layer_mixing=bool(g["flags"][1]))
    sd, x, am, lab = case_inputs(g, cfg)
    tr = EncoderCTCTrainer(cfg, "cuda:0", lr=1e-3)
    tr.load_state_dict(sd)
    assert tr.sync.on and tr.sync.world == world
    sl = slice(rank, rank + 1)                                   # this rank's shard of the batch
    tr.store.zero_grad()
    o = tr.forward_backward(x[sl].to("cuda:0"), am[sl].sum(-1).to("cuda:0"), lab[sl].to("cuda:0"))
    tr.sync.wait()
    torch.cuda.synchronize()
    grads = {k: v.cpu().numpy() for k, v in tr.grad_dict().items()}
    tr.optimizer_step()
    torch.cuda.synchronize()
    out[rank] = dict(loss=float(o["loss"]), grads=grads, wsum=float(tr.store.flat_p.double().sum()), norm=float(tr._scal[1]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("name,overlap", [("grads_tiny_rel", False), ("finetune_tiny_mix_extra", False), ("finetune_tiny_mix_extra", True)])
def test_two_rank_data_parallel_step_matches_full_batch_fixture(name, overlap):
    from helpers import load_golden
    world, port = 2, _free_port()
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, port, out, name, overlap), nprocs=world, join=True)
    g = load_golden(name)
    r0, r1 = out[0], out[1]
    assert abs(0.5 * (r0["loss"] + r1["loss"]) - float(g["loss"])) <= 1e-3 * float(g["loss"])     # mean of per-rank losses = batch loss
    worst = 0.0
    for k in g.files:
        if not k.startswith("grad:"):
            continue
        want = g[k].reshape(-1)
        a, b = r0["grads"][k[5:]].reshape(-1), r1["grads"][k[5:]].reshape(-1)
        assert np.array_equal(a, b), k                                   # both ranks hold the same reduced gradient
        nw = float(np.linalg.norm(want))
        if nw > 1e-5:
            worst = max(worst, float(np.linalg.norm(a - want)) / nw)
    assert worst < 0.03, worst
    assert r0["wsum"] == r1["wsum"] and r0["norm"] == r1["norm"] and r0["norm"] > 0


def _aed_worker(rank, world, port, out):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, here); sys.path.insert(0, os.path.dirname(here))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK="0", HFASR_DP_OVERLAP="0")
    import torch.distributed as dist
    from helpers import AED_JCFG, TINY_DEC, aed_case_inputs, load_golden
    from huggingface_asr_amd import shapes
    from huggingface_asr_amd.train_aed import JointAEDTrainer
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    g = load_golden("grads_aed_tiny")
    sd, x, am, lab = aed_case_inputs(g)
    enc_cfg = dict(shapes.TINY, ctc_zero_infinity=True, ctc_loss_reduction="mean", hidden_dropout=0.0, activation_dropout=0.0, attention_dropout=0.0,
                   final_dropout=0.0, feat_proj_dropout=0.0, csgu_conv_dropout=0.0, apply_spec_augment=False, layerdrop=0.0)
    tr = JointAEDTrainer(enc_cfg, dict(TINY_DEC, pos_emb_fixed=False, tie_word_embeddings=False), AED_JCFG, "cuda:0", lr=1e-3)
    tr.load_state_dict(sd)
    res = {}
    for shard in ([rank] if world > 1 else [0, 1]):          # world == 1: the per-shard gradients, un-synchronised (the expectation is built from them)
        sl = slice(shard, shard + 1)
        tr.enc.store.zero_grad(); tr.store.zero_grad()
        o = tr.forward_backward(x[sl].to("cuda:0"), am[sl].sum(-1).to("cuda:0"), lab[sl].to("cuda:0"))
        tr.enc.sync.wait(); tr.sync.wait()                    # default schedule: the merged all-reduce of each store runs here (optimizer_step calls the same)
        torch.cuda.synchronize()
        res[shard] = dict(loss=float(o["loss"]), enc_loss=float(o["enc_loss"]), dec_loss=float(o["dec_loss"]), grads={k: v.cpu().numpy() for k, v in tr.grad_dict().items()})
    if world > 1:
        assert tr.sync.on and tr.enc.sync.on and tr.sync.world == world
        tr.optimizer_step()
        torch.cuda.synchronize()
        res[rank]["wsum"] = float(tr.store.flat_p.double().sum()) + float(tr.enc.store.flat_p.double().sum())
        dist.barrier()
        dist.destroy_process_group()
    out[f"{world}:{rank}"] = res


def test_two_rank_data_parallel_joint_aed_step():
    """BASELINE config 3 is 'AED, data parallel': JointAEDTrainer on two ranks, one utterance each.  DDP semantics (what the reference gets from HF Trainer): every rank
    differentiates the mean loss of ITS shard and the gradients are averaged — so the expectation is the average of the two shards' own gradients (a single
    process, no sync), for the encoder's store AND the decoder's; both ranks must hold the same reduced gradients and the same weights after AdamW."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_aed_worker, args=(1, _free_port(), out), nprocs=1, join=True)
    mp.spawn(_aed_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    single, r0, r1 = out["1:0"], out["2:0"][0], out["2:1"][1]
    for key in ("loss", "enc_loss", "dec_loss"):              # a rank reports the loss of its own shard
        assert abs(r0[key] - single[0][key]) <= 1e-6 * abs(single[0][key]) and abs(r1[key] - single[1][key]) <= 1e-6 * abs(single[1][key]), key
    worst, n = 0.0, 0
    for k, g0 in single[0]["grads"].items():
        want = 0.5 * (g0.astype(np.float64) + single[1]["grads"][k].astype(np.float64)).reshape(-1)
        a, b = r0["grads"][k].reshape(-1), r1["grads"][k].reshape(-1)
        assert np.array_equal(a, b), k
        nw = float(np.linalg.norm(want))
        if nw > 1e-6:
            worst = max(worst, float(np.linalg.norm(a - want)) / nw)
            n += 1
    assert n > 100 and worst < 1e-4, (n, worst)          # 1 / world = 0.5 scales exactly; what is left is the summation order (batch of two vs two batches of one)
    assert r0["wsum"] == r1["wsum"]


def test_bench_train_entry_point_both_schedules_identical_weights():
    """`bench.py --train --overlap {0,1}` through bench.py's OWN entry point (it starts its ranks itself), two ranks sharing the box's one GPU over
    gloo: both gradient all-reduce schedules — one collective per parameter store after the backward, and one async all-reduce per layer range overlapped with the
    backward — must leave bit-identical replicas AND the same weights as each other after the same steps; the line names the schedule and carries per-rank step times."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    recs = {}
    for ov in (0, 1):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--train", "--gpus", "2", "--backend", "gloo", "--share-gpu", "--overlap", str(ov),
                            "--steps", "2", "--warmup", "1", "--batch", "4"], capture_output=True, text=True, timeout=900,
                           env=dict(os.environ, HFASR_DP_OVERLAP="0"))
        assert r.returncode == 0, r.stderr[-2000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        recs[ov] = json.loads(line)
    for ov, rec in recs.items():
        assert rec["n_gpus"] == 2 and rec["rccl_ranks"] == 2 and rec["backend"] == "gloo"
        assert rec["replicas_identical"] is True and len(rec["ms_per_step_by_rank"]) == 2 and rec["all_reduce_ms"] is not None
        assert ("overlap" in rec["schedule"]) == bool(ov)
    # Same seeded weights, same shards, and (round 4) no float atomics left in the backward: the two schedules reduce the SAME gradient bits (a two-rank sum is
    # commutative, so the bucket partition does not matter) — the first step's global gradient norm and the weights after the steps are EQUAL, not close.  This is what
    # makes `--overlap 1` on real RCCL a yes / no question: any co-residency corruption of a gradient, however small, shows as an inequality here.
    assert recs[0]["first_step_grad_norm"] == recs[1]["first_step_grad_norm"], (recs[0]["first_step_grad_norm"], recs[1]["first_step_grad_norm"])
    assert recs[0]["weights_checksum_by_rank"] == recs[1]["weights_checksum_by_rank"], (recs[0]["weights_checksum_by_rank"], recs[1]["weights_checksum_by_rank"])


def test_full_bench_command_carries_train_dp_when_it_runs_on_more_than_one_rank():
    """the forward replica bench with --full (`bench.py --gpus N --full`) also runs, at N > 1, the config-3 training step
    under BOTH gradient all-reduce schedules and reports it as `train_dp` — so one multi-GPU run exercises the gradient all-reduce without a second invocation.  Here:
    two ranks sharing the box's one GPU over gloo, small batches.  The schedules must agree bit for bit (no float atomics in the backward), replicas must be identical."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--streams", "1", "--train-dp-batch", "4", "--train-dp-steps", "2", "--no-kernel-events", "--full"], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, HFASR_DP_OVERLAP="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["rccl_ranks"] == 2 and rec["value"] > 0
    assert rec["one_step_ms"] > 0 and rec["one_step_value"] > 0 and rec["steps_in_flight"] == 1          # flat keys beside `value`
    dp = rec["train_dp"]
    assert dp is not None and "error" not in dp, dp
    assert len(dp["ms_per_step"]) == 2 and all(v > 0 for v in dp["ms_per_step"]) and dp["all_reduce_ms"] is not None
    assert dp["replicas_identical"] == [True, True] and dp["schedules_agree"] is True, dp
    assert dp["first_step_grad_norm"][0] == dp["first_step_grad_norm"][1] > 0
    assert rec["secondary"] is None                            # configs 3-5 ride the single-GPU line only


def test_a_rank_failing_in_train_dp_cannot_take_the_forward_line_down():
    """VERDICT r4 item 5 / ADVICE r4: with --full at more than one rank the forward headline is printed before the training collectives start; a rank that fails inside `train_dp`
    (here: injected on rank 1 while rank 0 is already inside the first schedule's collectives) exits non-zero at once, the launcher ends the run, and stdout still carries a
    parseable forward line — the run neither hangs until the driver's limit nor loses its headline."""
    import json
    import subprocess
    import sys
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--share-gpu", "--steps", "2", "--warmup", "1", "--batch", "4",
                        "--streams", "1", "--train-dp-batch", "4", "--train-dp-steps", "2", "--no-kernel-events", "--full"], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, HFASR_DP_OVERLAP="0", HFASR_BENCH_FAIL_RANK="1"))
    assert r.returncode != 0
    assert time.time() - t0 < 400
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, r.stderr[-2000:]
    rec = json.loads(lines[-1])
    assert rec["n_gpus"] == 2 and rec["value"] > 0 and rec["train_dp"] is None and rec["roofline"] is None or rec["value"] > 0
    assert "injected failure" in r.stderr
