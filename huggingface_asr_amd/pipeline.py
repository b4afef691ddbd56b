"""Independent forward steps in flight together (serving / throughput mode).

One forward of the encoder is a chain of ~240 dependent launches, most of them one tile per CU: each has a fill and a drain that nothing in the SAME step can
cover.  A second, independent step can: `ForwardPipeline` keeps `lanes` engines (each with its own workspace; the same weights) on `lanes` HIP streams and hands
consecutive submissions to consecutive lanes.  A submission's results are the bits the engine gives alone (tests/test_gpu_encoder.py).  Measured on the headline
config (base encoder, 32 x 10 s per step): 4.97 -> 4.24 ms per step with two lanes, 4.16 with three (tools/two_stream_bench.py).

The library's own kernels contain no packed-f32 arithmetic (csrc/build.py enforces it), which is what made co-resident kernels from two streams safe
("Concurrent kernels"); the training path stays single-stream (RCCL's kernels are not ours to rebuild)."""
from __future__ import annotations

import os

import torch

from .engine import EBranchformerEngine


DEFAULT_HW_QUEUES = 4          # the HIP runtime's own GPU_MAX_HW_QUEUES


def reserve_hw_queues(lanes: int) -> int:
    """The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and reads that variable once, when it initialises:
    with four lanes next to the default stream two of them take turns on one queue (measured, base encoder, wide tiles: 4.61 ms per step; with 8 queues 3.85).
    Call this BEFORE the first HIP call of the process (torch.cuda.is_available() is one).  Four or more lanes need 8 queues: the variable is raised to 8 when it is
    absent or holds the runtime's default of 4 — an environment that spells the default out (a job wrapper exporting GPU_MAX_HW_QUEUES=4 for every command) expresses no
    choice about lanes.  It is never lowered and never set above 8 here; a value above the need stays, and so does one BELOW the runtime's default (1-3: a restriction
    somebody chose).  HFASR_HW_QUEUES=<n> pins the count whatever the lanes need.
    -> the queue count the runtime will see."""
    want = 8 if lanes > 3 else DEFAULT_HW_QUEUES
    have = os.environ.get("GPU_MAX_HW_QUEUES")
    pin = os.environ.get("HFASR_HW_QUEUES")
    if pin is not None:
        want = int(pin)
        if not 1 <= want <= 32:
            raise ValueError(f"HFASR_HW_QUEUES={pin!r}: a queue count from 1 to 32")
    elif have is None:
        if want == DEFAULT_HW_QUEUES:
            return want                              # nothing to raise: the variable stays absent
    elif not DEFAULT_HW_QUEUES <= int(have) < want:
        return int(have)                             # enough already, or a restriction below the default
    if have is not None and int(have) == want:
        return want
    if torch.cuda.is_initialized():
        raise RuntimeError(f"reserve_hw_queues: the HIP runtime is already initialised; export GPU_MAX_HW_QUEUES={want} before starting the process")
    os.environ["GPU_MAX_HW_QUEUES"] = str(want)
    return want


class ForwardPipeline:
    def __init__(self, cfg: dict, device, state_dict: dict, lanes: int = 2, wide_tiles: bool = False, precision: str = "bf16"):
        if lanes < 1:
            raise ValueError("lanes >= 1")
        if precision != "bf16":      # the lanes share one bf16 weight table and run the folded / wide-tile kernels: the fp32 mode (engine.py) has neither
            raise NotImplementedError(f"ForwardPipeline lanes run in precision='bf16' only, got {precision!r}")
        self.device = torch.device(device)
        if lanes > 3 and int(os.environ.get("GPU_MAX_HW_QUEUES", "4")) < 8:
            import warnings
            warnings.warn("ForwardPipeline: more than 3 lanes on fewer than 8 hardware queues — lanes will take turns on one queue (measured on 4 queues: 4.6 instead of "
                          "3.8 ms per step); call pipeline.reserve_hw_queues(lanes) before the first HIP call of the process (it raises an absent or default "
                          "GPU_MAX_HW_QUEUES to 8; HFASR_HW_QUEUES pins another count), or export GPU_MAX_HW_QUEUES=8", RuntimeWarning)
        self.engines = []
        for i in range(lanes):
            e = EBranchformerEngine(cfg, self.device)
            e.wide_tiles = bool(wide_tiles)          # mi_ebf_config.wide_tiles: fewer, fatter GEMM blocks per launch — pays with >= 3 lanes
            if i == 0:
                e.load_state_dict(state_dict)
            else:
                e.share_weights_from(self.engines[0])        # one packed weight table for every lane; a lane owns its workspace and position cache only
            self.engines.append(e)
        self.streams = [torch.cuda.Stream(device=self.device) for _ in range(lanes)] if lanes > 1 else [None]
        self.events = [None] * lanes                 # the event recorded behind each lane's latest submission (wait on it before reading that lane's results on another stream)
        self._next = 0

    @property
    def lanes(self) -> int:
        return len(self.engines)

    def submit(self, fn):
        """fn(engine, lane) is enqueued on the next lane's stream (behind that lane's earlier work only) -> (lane, fn's return value).
        `self.events[lane]` is recorded behind it: wait on that event (or torch.cuda.synchronize()) before reading the results on another stream."""
        lane = self._next
        self._next = (lane + 1) % len(self.engines)
        st = self.streams[lane]
        if st is None:
            return lane, fn(self.engines[lane], lane)
        with torch.cuda.stream(st):
            out = fn(self.engines[lane], lane)
            ev = torch.cuda.Event()
            ev.record(st)
            self.events[lane] = ev
            return lane, out

    def reset(self):
        self._next = 0
