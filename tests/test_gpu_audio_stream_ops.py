"""GPU: the stateful log-mel front end (fbank.FbankStream; csrc/fbank_stream.hip).  Audio pushed in irregular pieces must give, bit for bit, the frames the one-shot
extractor gives for the whole clip (`fbank_gpu` with normalize=None / "global") — torch.equal: both kernels run one frame body (fbank_body.hpp) —, whatever the other
slots do, and the reference's recorded features within the one-shot kernel's own bar (atol 2e-5, tests/test_gpu_ops.py test_fbank_golden)."""
import random

import numpy as np
import pytest
import torch

from helpers import load_golden
from huggingface_asr_amd import _lib
from huggingface_asr_amd import fbank as FB
from huggingface_asr_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGES = [0, 1, 159, 160, 161, 399, 400, 401]


def pieces(seed, total, most):
    """sizes that sum to `total`: the sizes around the hop and the frame, each once, among random ones up to `most`"""
    rng = random.Random(seed)
    sizes = list(EDGES)
    left = total - sum(sizes)
    while left > 0:
        n = min(left, rng.choice([rng.randrange(0, 50), rng.randrange(100, 700), rng.randrange(100, most + 1)]))
        sizes.append(n)
        left -= n
    rng.shuffle(sizes)
    assert sum(sizes) == total
    return sizes


def drain(fb, got, slots, final):
    """pop whole chunks while a slot holds one (final: everything), checking the zero rows -> pops made"""
    pops = 0
    while True:
        takes = [(s, min(fb.W, fb.ready(s))) for s in slots if fb.ready(s) >= (1 if final else fb.W)]
        if not takes:
            return pops
        out = fb.pop(takes)
        assert out.shape == (len(takes), fb.W, fb.nmel)
        for i, (s, n) in enumerate(takes):
            assert not bool(out[i, n:].any()), "rows behind a slot's frames are zero"
            got[s].append(out[i, :n].clone())
        pops += 1


def run(fb, sessions, whole_chunks=True):
    """sessions {slot: (wave (N), sizes)}: call i pushes piece i of every session that still has one -> {slot: frames (T, nmel)}"""
    got, pos = {s: [] for s in sessions}, {s: 0 for s in sessions}
    for s in sessions:
        fb.open(s)
    for i in range(max(len(sz) for _, sz in sessions.values())):
        call = {}
        for s, (w, sz) in sessions.items():
            if i < len(sz):
                call[s] = w[pos[s]: pos[s] + sz[i]]
                pos[s] += sz[i]
        fb.push(call)
        drain(fb, got, list(call), final=not whole_chunks)
    drain(fb, got, list(sessions), final=True)
    return {s: torch.cat(v) if v else torch.zeros((0, fb.nmel), device=DEV) for s, v in got.items()}


@pytest.fixture(scope="module")
def clips():
    tb = FB.FbankTables(80)
    g = load_golden("fbank")
    means, stds = (torch.from_numpy(np.asarray(g[k], dtype=np.float32)).to(DEV) for k in ("global_means", "global_stds"))
    w = torch.from_numpy(synth.waveforms(21, 3, 24000)).to(DEV)
    raw, _ = FB.fbank_gpu(w, tb, normalize=None)
    glob, _ = FB.fbank_gpu(w, tb, normalize="global", global_means=means, global_stds=stds)
    assert raw.shape == (3, 148, 80)
    return dict(tb=tb, w=w, raw=raw, glob=glob, means=means, stds=stds, g=g)


# ------------------------------------------------------------------ bit equality with the one-shot extractor
def test_three_schedules_idle_slot_reuse_and_a_wrapping_ring(clips):
    """ring of 16 + 5 frames for clips of 148: every slot wraps it seven times; slot 3 is open and idle, slot 4 never opened, slot 0 takes a second session"""
    tb, w, raw = clips["tb"], clips["w"], clips["raw"]
    fb = FB.FbankStream(5, 16, 700, tb, device=DEV)
    assert fb.R == 21
    fb.open(3)
    a = run(fb, {0: (w[0], pieces(1, 24000, 700)), 1: (w[1], pieces(2, 24000, 700)), 2: (w[2], pieces(3, 24000, 300))})
    for s in range(3):
        assert torch.equal(a[s], raw[s]), f"slot {s}: differs from the one-shot frames by {float((a[s] - raw[s]).abs().max())}"
    assert fb.ready(3) == 0 and fb.n[3] == 0
    b = run(fb, {0: (w[2], pieces(4, 24000, 700)), 2: (w[0][:9000], pieces(5, 9000, 650))})          # second sessions: stale carry and ring rows are never read
    assert torch.equal(b[0], raw[2]) and torch.equal(b[2], raw[0][: FB.num_frames(9000)])
    torch.cuda.synchronize()


def test_global_normalisation_and_long_pushes(clips):
    """normalize="global" fused into the store == fbank_gpu(normalize="global"); pushes of up to 4000 samples are split into launches of at most 1000"""
    tb, w = clips["tb"], clips["w"]
    fb = FB.FbankStream(3, 64, 1000, tb, normalize="global", global_means=clips["means"], global_stds=clips["stds"], device=DEV)
    got = run(fb, {0: (w[0], pieces(6, 24000, 4000)), 2: (w[1], pieces(7, 24000, 4000)), 1: (w[2].cpu(), pieces(8, 24000, 2500))}, whole_chunks=False)
    for s, b in ((0, 0), (2, 1), (1, 2)):                                 # slot 1 was pushed host tensors
        assert torch.equal(got[s], clips["glob"][b]), f"slot {s}"


def test_int16_push_is_the_float_push(clips):
    tb = clips["tb"]
    pcm = (clips["w"][0] * 32768.0).round().clamp(-32768, 32767).to(torch.int16)
    flt = pcm.to(torch.float32) / 32768.0
    fb = FB.FbankStream(2, 16, 700, tb, device=DEV)
    sz = pieces(9, 24000, 700)
    a = run(fb, {0: (pcm, sz)})[0]
    b = run(fb, {1: (flt, sz)})[1]
    want, _ = FB.fbank_gpu(flt[None], tb, normalize=None)
    assert torch.equal(a, b) and torch.equal(a, want[0])
    with pytest.raises(ValueError, match="float32"):
        fb.push({0: flt.double()})


def test_short_session_yields_no_frame(clips):
    tb, w = clips["tb"], clips["w"]
    fb = FB.FbankStream(2, 16, 700, tb, device=DEV)
    got = run(fb, {1: (w[0][:399], [0, 160, 1, 238])})
    assert got[1].shape == (0, 80) and fb.ready(1) == 0 and fb.n[1] == 399
    got = run(fb, {1: (w[1][:400], [399, 1])})                            # the slot again: exactly one frame, of the new session's samples alone
    assert torch.equal(got[1], clips["raw"][1][:1])


def test_bit_identical_runs_and_independence_of_the_other_slots(clips):
    tb, w, raw = clips["tb"], clips["w"], clips["raw"]
    sz = [pieces(10 + b, 24000, 700) for b in range(3)]
    both = lambda: run(FB.FbankStream(4, 16, 700, tb, device=DEV), {0: (w[0], sz[0]), 1: (w[1], sz[1]), 3: (w[2], sz[2])})
    a, b = both(), both()
    alone = run(FB.FbankStream(4, 16, 700, tb, device=DEV), {2: (w[1], sz[1])})                          # the same session without neighbours, in another slot
    assert all(torch.equal(a[s], b[s]) for s in a)
    assert torch.equal(alone[2], a[1]) and torch.equal(a[1], raw[1])


# ------------------------------------------------------------------ the reference's recorded features
@pytest.mark.parametrize("wave", ["sweep", "noise", "silence_padded"])
def test_streamed_pieces_match_the_reference_golden(clips, wave):
    g, tb = clips["g"], clips["tb"]
    x = torch.from_numpy(g[f"{wave}_wave"]).to(DEV)
    N = int(x.numel())
    sz = pieces(11, N, 700) if N > sum(EDGES) + 700 else [N // 3, N - N // 3]
    raw = run(FB.FbankStream(1, 16, 700, tb, device=DEV), {0: (x, sz)})[0]
    assert raw.shape == g[f"{wave}_raw"].shape
    d = float(np.abs(raw.cpu().numpy() - g[f"{wave}_raw"]).max())
    print(f"{wave}: streamed vs the reference's recorded features, max abs {d:.3g}")
    np.testing.assert_allclose(raw.cpu().numpy(), g[f"{wave}_raw"], atol=2e-5, rtol=0)
    if wave == "noise":
        fb = FB.FbankStream(1, 16, 700, tb, normalize="global", global_means=g["global_means"], global_stds=g["global_stds"], device=DEV)
        glob = run(fb, {0: (x, sz)})[0]
        np.testing.assert_allclose(glob.cpu().numpy(), g["noise_global"], atol=2e-5, rtol=0)


# ------------------------------------------------------------------ argument errors: MI_ERR_ARG, nothing launched
def test_argument_errors_launch_nothing(clips):
    tb = clips["tb"].device(DEV)
    L = _lib.lib()
    S, R, F = 3, 21, 80
    state = torch.full((L.mi_fbank_stream_state_bytes(S, R, F) // 4,), 7.0, device=DEV)
    big = torch.full((3 * (800 + R * 128),), 7.0, device=DEV)
    samples = torch.zeros(4000, device=DEV)
    out = torch.full((S, 16, F), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def push(recs, state=state, nmel=F, normalize=0, means=None, n_samples=4000, dtype=0, A=None):
        h = torch.tensor(recs, dtype=torch.int32)
        d = h.to(DEV)
        return L.mi_fbank_stream_push(state.data_ptr(), state.numel() * 4, S, R, nmel, samples.data_ptr(), n_samples, dtype, h.data_ptr(), d.data_ptr(),
                                      len(recs) if A is None else A, tb["window"].data_ptr(), tb["twiddle"].data_ptr(), tb["mel_t"].data_ptr(), tb["lo"].data_ptr(),
                                      tb["hi"].data_ptr(), means, means, normalize, FB.MEL_FLOOR, FB.PREEMPH, st)

    def pop(recs, rows=16):
        h = torch.tensor(recs, dtype=torch.int32)
        d = h.to(DEV)
        return L.mi_fbank_stream_pop(state.data_ptr(), state.numel() * 4, S, R, F, h.data_ptr(), d.data_ptr(), len(recs), out.data_ptr(), rows, st)

    ok = [0, 0, 1000, 0, 0, 0, 0, 0]
    E = _lib.ERR_ARG
    assert push([[3] + ok[1:]]) == E and push([[-1] + ok[1:]]) == E                         # a slot out of range
    assert push([ok, [1] + ok[1:], ok]) == E                                                 # a slot named twice
    assert push([[0, 0, 3900, 0, 0, 0, 0, 0]]) == E                                          # 22 frames into a ring of 21
    assert push([[0, 0, 1000, 0, 0, 18, 0, 0]]) == E                                         # 18 held + 4 new > 21
    assert push([[0, 0, 1000, 3001, 0, 0, 0, 0]]) == E                                       # samples outside the buffer
    assert push([ok], n_samples=999) == E
    assert push([[0, 0, 1000, 0, 21, 0, 0, 0]]) == E and push([[0, 0, 1000, 0, 0, 0, 2, 0]]) == E      # a write position outside the ring, a third carry buffer
    assert push([[0, -1, 1000, 0, 0, 0, 0, 0]]) == E and push([[0, 0, -1, 0, 0, 0, 0, 0]]) == E
    assert push([ok], state=big, nmel=128) == E                                              # nmel > 127
    assert push([ok], normalize=1, means=None) == E                                          # a normalisation without its tables
    assert push([ok], dtype=2) == E
    assert push([ok], state=state[:-1]) == E                                                 # a state too small
    assert pop([[3, 0, 4]]) == E and pop([[0, 0, 4], [0, 4, 4]]) == E and pop([[0, 21, 4]]) == E and pop([[0, 0, 17]]) == E and pop([[0, 0, -1]]) == E
    torch.cuda.synchronize()
    assert bool((state == 7.0).all()) and bool((big == 7.0).all()) and bool((out == 7.0).all())       # nothing ran
    assert push([ok]) == 0 and pop([[0, 0, 4]]) == 0                                         # the same calls with good records do
    torch.cuda.synchronize()
    assert bool((out[0, 4:] == 0).all()) and not bool((out[0, :4] == 7.0).any()) and bool((out[1:] == 7.0).all())
