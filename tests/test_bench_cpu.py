"""CPU: bench.py's argument checks and its --dump-outputs writer (the arrays two builds are compared by, output for output).  No GPU calls."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        spec.loader.exec_module(mod)
    finally:
        sys.argv = argv
    return mod


def test_steps_is_the_number_of_timed_steps_and_at_least_one():
    B = _bench()
    assert B.parse_args(["--steps", "7", "--warmup", "2"]).steps == 7
    for bad in (["--steps", "0"], ["--steps", "-1"], ["--dump-outputs", "d", "--train"], ["--dump-outputs", "d", "--secondary", "decode"]):
        with pytest.raises(SystemExit):
            B.parse_args(bad)


def test_full_is_off_by_default_and_keep_profile_needs_it():
    B = _bench()
    assert B.parse_args([]).full is False and B.parse_args(["--full"]).full is True
    assert B.parse_args(["--full", "--keep-profile", "d"]).keep_profile == "d"
    with pytest.raises(SystemExit):
        B.parse_args(["--keep-profile", "d"])          # the roofline leg it keeps a file of runs with --full only


def _last_step(B_, T2, V1, seed):
    g = torch.Generator().manual_seed(seed)
    lbuf = torch.randn((B_, T2, (V1 + 7) // 8 * 8), generator=g)        # the engine's padded row stride; callers get the (B, T2, V+1) view
    outer = torch.tensor([T2 - 3 * b for b in range(B_)], dtype=torch.int32)
    return {"out": {"logits": lbuf[..., :V1], "outer_len": outer, "lse": None}, "loss": torch.tensor(1.25)}


def test_dump_outputs_is_a_fixed_sample_of_valid_rows_within_the_size_limit(tmp_path):
    B = _bench()
    B_, T2, V1 = 32, 250, 5001                                           # the headline's shape: 160 MB of fp32 logits
    last = _last_step(B_, T2, V1, 0)
    B.dump_outputs(str(tmp_path / "a"), last)
    B.dump_outputs(str(tmp_path / "b"), _last_step(B_, T2, V1, 0))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["ctc_loss.npy", "logits_row_index.npy", "logits_rows.npy", "outer_len.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), n
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    idx = np.load(tmp_path / "a" / "logits_row_index.npy").astype(np.int64)
    rows = np.load(tmp_path / "a" / "logits_rows.npy")
    outer = last["out"]["outer_len"].numpy()
    assert len(idx) > 1000 and np.all(np.diff(idx) > 0) and np.all(idx % T2 < outer[idx // T2])       # distinct rows, none in a clip's padding
    np.testing.assert_array_equal(rows, last["out"]["logits"].reshape(B_ * T2, V1)[torch.from_numpy(idx)].numpy())
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "outer_len.npy"), outer)
    assert float(np.load(tmp_path / "a" / "ctc_loss.npy")[0]) == 1.25
