"""Host side of the log-mel front end: float64 tables + the two execution paths.

* `FbankTables` builds the povey window, FFT twiddles and Kaldi mel filterbank exactly as transformers'
  `window_function` / `mel_filter_bank` do (audio_utils.py:638-731, :745-806) for the settings hard-wired in
  `Speech2TextFeatureExtractor.__init__` (feature_extraction_speech_to_text.py:86-102).
* `fbank_gpu` runs the HIP kernels (csrc/fbank.hip) on device waveforms — the GPU pre-stage of `forward`.
* `fbank_numpy` is the fork-safe, GPU-free implementation used by `CustomFeatureExtractor` inside dataloader
  workers (reference src/utilities/callbacks.py:100-118 runs the extractor there); vectorised numpy float64.
* `FbankStream` is the stateful form for live audio (csrc/fbank_stream.hip): samples in pieces of any size in, feature frames
  in chunks out, bit for bit `fbank_gpu`'s frames of the whole audio with normalize=None / "global".
"""
from __future__ import annotations

import numpy as np

FRAME, HOP, NFFT, NBINS = 400, 160, 512, 257
MEL_FLOOR = 1.192092955078125e-07
PREEMPH = 0.97


class FbankTables:
    def __init__(self, num_mel: int = 80, sr: int = 16000, fmin: float = 20.0, fmax: float | None = None):
        fmax = float(sr // 2) if fmax is None else fmax
        self.num_mel = num_mel
        self.window = np.power(np.hanning(FRAME), 0.85)                      # "povey", periodic=False
        k = np.arange(NFFT // 2)
        self.twiddle = np.stack([np.cos(2 * np.pi * k / NFFT), -np.sin(2 * np.pi * k / NFFT)], 1)   # exp(-2 pi i k/512)
        mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
        mel_freqs = np.linspace(mel(fmin), mel(fmax), num_mel + 2)
        fft_mels = mel((sr / ((NBINS - 1) * 2)) * np.arange(NBINS))
        diff = np.diff(mel_freqs)
        slopes = mel_freqs[None, :] - fft_mels[:, None]
        self.filters = np.maximum(0.0, np.minimum(-slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]))   # (257, nmel)
        nz = self.filters > 0
        self.lo = np.array([int(np.argmax(nz[:, f])) if nz[:, f].any() else 0 for f in range(num_mel)], np.int32)
        self.hi = np.array([int(NBINS - np.argmax(nz[::-1, f])) if nz[:, f].any() else 0 for f in range(num_mel)], np.int32)
        self._dev = {}

    def device(self, device):
        import torch
        key = str(device)
        if key not in self._dev:
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._dev[key] = dict(window=t(self.window), twiddle=t(self.twiddle), mel_t=t(self.filters.T.copy()),
                                  lo=t(self.lo), hi=t(self.hi))
        return self._dev[key]


def num_frames(num_samples: int) -> int:
    return 1 + (num_samples - FRAME) // HOP if num_samples >= FRAME else 0


def fbank_numpy(waveform: np.ndarray, tables: FbankTables) -> np.ndarray:
    """(N,) float32 -> (T, nmel) float32, numerically the numpy branch of the reference extractor."""
    x = (np.asarray(waveform, dtype=np.float32) * np.float32(2 ** 15)).astype(np.float64)
    T = num_frames(x.size)
    idx = np.arange(FRAME)[None, :] + HOP * np.arange(T)[:, None]
    fr = x[idx]
    fr = fr - fr.mean(axis=1, keepdims=True)
    pre = fr.copy()
    pre[:, 1:] -= PREEMPH * fr[:, :-1]
    pre[:, 0] *= 1.0 - PREEMPH
    pre *= tables.window[None, :]
    spec = np.fft.rfft(pre, n=NFFT, axis=1).astype(np.complex64)
    power = np.abs(spec, dtype=np.float64) ** 2.0
    return np.log(np.maximum(MEL_FLOOR, power @ tables.filters)).astype(np.float32)


def fbank_gpu(wave, tables: FbankTables, num_samples=None, pad_frames_to: int | None = None, *, normalize="utterance",
              normalize_means=True, normalize_vars=True, global_means=None, global_stds=None, padding_value=0.0):
    """wave (B,N) float32 device tensor -> (features (B,T,nmel) float32, frames (B,) int32).

    T = frames of the longest clip, optionally rounded up (`pad_frames_to` = collator's pad_to_multiple_of);
    frames beyond a clip's own count hold `padding_value` (the collator's right padding)."""
    import torch

    from . import _lib
    B, N = wave.shape
    tb = tables.device(wave.device)
    if num_samples is None:
        key = ("frames", str(wave.device), B, N)             # the same full-length batch every step: one fill kernel less per call
        frames = tb.get(key)
        if frames is None:
            frames = tb[key] = torch.full((B,), num_frames(N), dtype=torch.int32, device=wave.device)
        T = num_frames(N)
    else:
        frames = torch.clamp((num_samples.to(torch.int32) - FRAME) // HOP + 1, min=0)
        T = num_frames(N)
    if pad_frames_to:
        T = (T + pad_frames_to - 1) // pad_frames_to * pad_frames_to
    # utterance CMVN rewrites every element of the buffer, padding rows included (csrc/fbank.hip cmvn kernels): no fill pass in front of it
    out = (torch.empty((B, T, tables.num_mel), dtype=torch.float32, device=wave.device) if normalize == "utterance"
           else torch.full((B, T, tables.num_mel), float(padding_value), dtype=torch.float32, device=wave.device))
    st = torch.cuda.current_stream().cuda_stream
    L = _lib.lib()
    _lib.check(L.mi_fbank_f64(wave.data_ptr(), wave.stride(0), 0 if num_samples is None else num_samples.to(torch.int32).data_ptr(),
                              N, tb["window"].data_ptr(), tb["twiddle"].data_ptr(), tb["mel_t"].data_ptr(), tb["lo"].data_ptr(),
                              tb["hi"].data_ptr(), out.data_ptr(), T, B, tables.num_mel, MEL_FLOOR, PREEMPH, st), "mi_fbank_f64")
    if normalize == "utterance":
        _lib.check(L.mi_cmvn_utterance(out.data_ptr(), frames.data_ptr(), B, T, tables.num_mel, int(normalize_means),
                                       int(normalize_vars), float(padding_value), st), "mi_cmvn_utterance")
    elif normalize == "global":
        _lib.check(L.mi_cmvn_global(out.data_ptr(), out.numel(), tables.num_mel, global_means.data_ptr(), global_stds.data_ptr(), st),
                   "mi_cmvn_global")
    return out, frames


def strip_zeros_pad_gpu(wave, num_samples=None, min_len: int = 8000):
    """The array handling of the reference's `default_transform` (callbacks.py:108-118) for a device batch: every clip stripped of leading / trailing
    zero samples (`np.trim_zeros`, data_utils.py:173-177) and zero-padded to at least `min_len` samples.
    wave (B,N) float32 device tensor -> (stripped (B, max(N, min_len)) float32, eff_len (B,) int32 = samples the feature extractor sees)."""
    import torch

    from . import _lib
    B, N = wave.shape
    n_out = max(N, int(min_len))
    out = torch.empty((B, n_out), dtype=torch.float32, device=wave.device)
    meta = torch.empty((3, B), dtype=torch.int32, device=wave.device)
    ns = None if num_samples is None else num_samples.to(device=wave.device, dtype=torch.int32).contiguous()
    _lib.check(_lib.lib().mi_trim_zeros_pad_f32(wave.data_ptr(), wave.stride(0), 0 if ns is None else ns.data_ptr(), N, B, int(min_len), out.data_ptr(), out.stride(0),
                                                n_out, meta[0].data_ptr(), meta[1].data_ptr(), meta[2].data_ptr(), torch.cuda.current_stream().cuda_stream),
               "mi_trim_zeros_pad_f32")
    return out, meta[2]


# ---------------------------------------------------------------------------------------------------- streaming: audio in pieces -> feature frames in chunks
def frames_added(n: int) -> int:
    """the most frames that n more samples can complete, whatever came before: ceil(n / 160)"""
    return (n + HOP - 1) // HOP


def check_samples(x, what="samples"):
    """sample tensors are fp32 in [-1, 1] (what the extractor takes) or int16 PCM, on the host or the device -> 0 / 1 (mi_fbank_stream_push's sample_dtype)"""
    import torch
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.int16):
        raise ValueError(f"{what}: audio is a float32 tensor in [-1, 1] or an int16 PCM tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    return 0 if x.dtype == torch.float32 else 1


class FbankStream:
    """Stateful log-mel front end over `slots` sessions (csrc/fbank_stream.hip, whose header states the semantics): audio goes in in pieces of any size, feature frames
    come out in pieces of up to `chunk_feature_frames` — bit for bit the frames `fbank_gpu` gives for the session's whole audio with normalize=None / "global".

        fb = FbankStream(slots, 4 * C, max_push_samples, tables, normalize="global", global_means=m, global_stds=s, device="cuda")
        fb.open(slot); fb.push({slot: samples}); fb.ready(slot) -> frames held; fb.pop([(slot, n)]) -> (A, 4 * C, nmel) fp32, rows n .. zero

    Holds host bookkeeping (per slot: samples so far, the carry's ping-pong side, the ring's read position and count) and the state tensor; the device reports nothing
    back.  The ring holds chunk_feature_frames + frames_added(max_push_samples) frames: a caller that pops whole chunks as they become ready never overruns it."""

    def __init__(self, slots, chunk_feature_frames, max_push_samples, tables: FbankTables, *, normalize=None, global_means=None, global_stds=None, device):
        import torch
        if normalize == "utterance":
            raise NotImplementedError("FbankStream: utterance CMVN needs the whole utterance (its mean and variance run over every frame), so it cannot stream; "
                                      "global statistics (normalize='global') or no normalisation (normalize=None) stream exactly")
        if normalize not in (None, "global"):
            raise ValueError(f"FbankStream: normalize is None or 'global', got {normalize!r}")
        if slots < 1 or chunk_feature_frames < 1 or max_push_samples < 1:
            raise ValueError("FbankStream: slots, chunk_feature_frames and max_push_samples >= 1")
        if tables.num_mel > 127:
            raise ValueError(f"FbankStream: {tables.num_mel} mel bins (the kernels take up to 127)")
        self.S, self.W, self.max_push, self.tables, self.normalize, self.device = int(slots), int(chunk_feature_frames), int(max_push_samples), tables, normalize, device
        self.R = self.W + frames_added(self.max_push)
        self.nmel = tables.num_mel
        self._means = self._stds = None
        if normalize == "global":
            if global_means is None or global_stds is None:
                raise ValueError("FbankStream: normalize='global' needs global_means and global_stds")
            self._means, self._stds = ((v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(torch.float32).reshape(-1).contiguous()
                                       for v in (global_means, global_stds))
            if self._means.numel() != self.nmel or self._stds.numel() != self.nmel:
                raise ValueError(f"FbankStream: global_means / global_stds hold {self._means.numel()} / {self._stds.numel()} values for {self.nmel} mel bins (feature_size)")
        self.n = [0] * self.S           # samples the slot's session has had
        self.sel = [0] * self.S         # the carry buffer that is current
        self.r = [0] * self.S           # the ring's read position
        self.count = [0] * self.S       # frames the ring holds
        self._state = None

    def state_bytes(self) -> int:
        from . import _lib
        return int(_lib.lib().mi_fbank_stream_state_bytes(self.S, self.R, self.nmel))

    def open(self, slot: int):
        """a new session in `slot`: host bookkeeping alone — nothing of the slot's old carry or ring is ever read"""
        self._slot(slot)
        self.n[slot] = self.count[slot] = self.r[slot] = self.sel[slot] = 0

    def ready(self, slot: int) -> int:
        return self.count[self._slot(slot)]

    def frames(self, slot: int) -> int:
        """frames the slot's session has produced so far"""
        return num_frames(self.n[self._slot(slot)])

    def _slot(self, slot):
        if not isinstance(slot, int) or not 0 <= slot < self.S:
            raise ValueError(f"FbankStream: slot {slot!r} outside 0..{self.S - 1}")
        return slot

    def _ensure_state(self):
        import torch
        if self._state is None:
            if torch.device(self.device).type != "cuda":
                raise RuntimeError("FbankStream needs a GPU device (no CPU fallback)")
            self._state = torch.empty(self.state_bytes(), dtype=torch.uint8, device=self.device)          # never read before written: the host knows every count
            if self._means is not None:
                self._means, self._stds = self._means.to(self.device), self._stds.to(self.device)
        return self._state

    def _upload(self, records):
        import torch
        host = torch.tensor(records, dtype=torch.int32).pin_memory()
        return host, host.to(self.device, non_blocking=True)

    def flatten(self, samples: dict, what="FbankStream.push"):
        """{slot: samples (n)} -> (one 1-D tensor, spans {slot: (offset, n)}); one dtype per call; pieces on the device stay there, host pieces are copied once, as one"""
        import torch
        kinds = {check_samples(x, what) for x in samples.values()}
        if len(kinds) > 1:
            raise ValueError(f"{what}: the audio of one call has one dtype (float32 or int16)")
        if any(x.dim() != 1 for x in samples.values()):
            raise ValueError(f"{what}: a session's audio is a 1-D tensor of samples")
        spans, off = {}, 0
        for s, x in samples.items():
            spans[self._slot(s)] = (off, int(x.numel()))
            off += int(x.numel())
        xs = list(samples.values())
        if any(x.is_cuda for x in xs):
            xs = [x.to(self.device) for x in xs]
        return torch.cat(xs), spans

    def push(self, samples: dict):
        """{slot: samples (n) fp32 / int16, n >= 0}: one launch for all named slots (several when a piece is longer than max_push_samples)"""
        if samples:
            self.push_flat(*self.flatten(dict(sorted(samples.items()))))

    def push_flat(self, flat, spans: dict):
        """the same with the pieces already in one 1-D tensor: spans {slot: (offset, n)}"""
        check_samples(flat, "FbankStream.push")
        if flat.dim() != 1 or any(off < 0 or n < 0 or off + n > flat.numel() for off, n in spans.values()):
            raise ValueError("FbankStream.push: spans outside the sample buffer")
        done = {self._slot(s): 0 for s in spans}
        count = dict((s, self.count[s]) for s in spans)
        for s, (_, n) in spans.items():                 # the whole call is checked before its first launch
            if count[s] + num_frames(self.n[s] + n) - num_frames(self.n[s]) > self.R:
                raise RuntimeError(f"FbankStream.push: slot {s} would hold more than the ring's {self.R} frames: pop before pushing more")
        flat = flat.to(self.device).contiguous()        # a host tensor is copied by torch
        while True:
            piece = {s: (off + done[s], min(self.max_push, n - done[s])) for s, (off, n) in spans.items() if n > done[s]}
            if not piece:
                return
            self._push_piece(flat, piece)
            for s, (_, n) in piece.items():
                done[s] += n

    def _push_piece(self, flat, piece):
        import torch

        from . import _lib
        state = self._ensure_state()
        recs = []
        for s, (off, n) in sorted(piece.items()):
            if n <= 0:
                continue
            recs.append([s, self.n[s], n, off, (self.r[s] + self.count[s]) % self.R, self.count[s], self.sel[s], 0])
        if not recs:
            return
        host, dev = self._upload(recs)
        tb = self.tables.device(self.device)
        p = lambda t: None if t is None else t.data_ptr()
        rc = _lib.lib().mi_fbank_stream_push(state.data_ptr(), state.numel(), self.S, self.R, self.nmel, flat.data_ptr(), flat.numel(), check_samples(flat),
                                             host.data_ptr(), dev.data_ptr(), len(recs), tb["window"].data_ptr(), tb["twiddle"].data_ptr(), tb["mel_t"].data_ptr(),
                                             tb["lo"].data_ptr(), tb["hi"].data_ptr(), p(self._means), p(self._stds), int(self.normalize == "global"), MEL_FLOOR, PREEMPH,
                                             torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mi_fbank_stream_push")
        for s, n_prev, n, *_ in recs:
            self.count[s] += num_frames(n_prev + n) - num_frames(n_prev)
            self.n[s] = n_prev + n
            self.sel[s] ^= 1

    def pop(self, takes):
        """[(slot, n)], n <= min(ready(slot), chunk_feature_frames): -> (A, chunk_feature_frames, nmel) fp32, entry i = the slot's next n frames then zero rows; one launch"""
        import torch

        from . import _lib
        takes = [(self._slot(s), int(n)) for s, n in takes]
        if not takes or len({s for s, _ in takes}) != len(takes):
            raise ValueError("FbankStream.pop: one (slot, n) per slot, at least one")
        for s, n in takes:
            if not 0 <= n <= min(self.count[s], self.W):
                raise ValueError(f"FbankStream.pop: slot {s} holds {self.count[s]} frames and a chunk is {self.W}, asked for {n}")
        state = self._ensure_state()
        host, dev = self._upload([[s, self.r[s], n] for s, n in takes])
        out = torch.empty((len(takes), self.W, self.nmel), dtype=torch.float32, device=self.device)
        rc = _lib.lib().mi_fbank_stream_pop(state.data_ptr(), state.numel(), self.S, self.R, self.nmel, host.data_ptr(), dev.data_ptr(), len(takes), out.data_ptr(),
                                            self.W, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, "mi_fbank_stream_pop")
        for s, n in takes:
            self.r[s] = (self.r[s] + n) % self.R
            self.count[s] -= n
        return out
