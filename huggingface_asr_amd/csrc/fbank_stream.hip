// Stateful log-mel front end for the streaming encoder: audio samples in, in pieces of any size, feature frames out, in the chunks the stream step takes — bit for bit
// the frames of the one-shot extractor (fbank.hip) on the whole utterance.  That is possible because the extractor snips edges: frame t reads samples [160 t, 160 t + 400)
// and nothing else, and because global normalisation works per element.  The frame body is fbank.hip's (fbank_body.hpp); only the way a sample is fetched differs.
//
// Semantics (normative)
//  * T(N) = 0 for N < 400, else 1 + (N - 400) / 160: the frames of N samples.
//  * State of S slots, mi_fbank_stream_state_bytes(S, R, nmel) = S * (2 * 400 + R * nmel) * 4 bytes: [carry (S, 2, 400) fp32 | fifo (S, R, nmel) fp32].  A slot's carry
//    holds the at most 399 samples that its next frame still needs, in one of two buffers (a ping-pong the host chooses: a push reads buffer `sel` and writes the
//    other); its fifo is a ring of R feature frames, R >= 4 * C + the frames one push can add (ceil(n / 160) for a push of n samples).
//  * Sample counts, frame counts, the ping-pong choice and the ring positions are the caller's host arithmetic (huggingface_asr_amd/fbank.py FbankStream).  The device
//    never reports a count back, no call synchronises with the host or reads device memory from it.  As the host knows every count, stale carry or ring contents of a
//    reused slot are never read: opening a session is host bookkeeping alone (N = 0), there is no reset.
//  * Push, one launch for all A records of a call.  Record i (8 ints): slot, N_prev = the samples the slot's session has had, n_new >= 0, src = the offset of its new
//    samples in `samples` (fp32 in [-1, 1], or int16 PCM converted as (float)s / 32768.0f, which is exact: an int16 push gives the bits of the same samples pushed as
//    fp32), w = the ring's write position, count = the frames the ring holds, sel = the carry buffer that is current, 0.
//    The call computes frames T(N_prev) .. T(N_prev + n_new) - 1 of the slot: sample s of the session comes from the carry when s < N_prev (carry[s - 160 T(N_prev)]),
//    else from the new samples.  Frame T(N_prev) + j goes to ring row (w + j) % R, normalised — not at all, or "global": (x - mean) / std, global_norm_kernel's fp32
//    subtraction and division — in the store.  The carry afterwards, written to buffer 1 - sel, is samples [160 T(N), N) of the session, N = N_prev + n_new: 240 .. 399
//    samples once a frame exists, else all N.  n_new = 0 leaves the slot untouched (the host does not flip its sel).
//  * Pop, one launch: record i (3 ints) = slot, r = the ring's read position, n <= rows: out (A, rows, nmel) fp32, row j < n of entry i = ring row (r + j) % R of the
//    slot, rows n .. rows - 1 zero — the (A, 4 * C, F) buffer of mi_ebf_stream_step / mi_ebf_stream_step_slots, a finish tail zero-padded.
//  * Records come twice, as the pool's tables do: rec_host is checked, rec_dev holds the same words on the device and is what the kernel reads.  MI_ERR_ARG before any
//    launch: a slot out of range or named twice, a ring overrun (count + the new frames > R), positions outside the ring, samples outside the buffer, nmel > 127, a
//    normalisation asked for without tables, a state too small.
//  * No atomics; a slot's result does not depend on the other slots of the call, on its slot index or on how the samples were cut into pushes.
#include "fbank_body.hpp"

namespace {

using namespace fbank_body;

constexpr int CARRY = 400;          // floats per carry buffer (399 used at most)
constexpr int PUW = 8;              // push record: slot, N_prev, n_new, src, w, count, sel, 0
constexpr int POW = 3;              // pop record: slot, r, n

struct PushArgs {
    float* carry;                   // (S, 2, CARRY)
    float* fifo;                    // (S, R, nmel)
    const void* samples;
    const int* rec;                 // (A, PUW) on the device
    const float* means; const float* stds;   // (nmel) or both null
    Tables tb;
    int R;
};

template <typename T> __device__ __forceinline__ float to_sample(T v);
template <> __device__ __forceinline__ float to_sample<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_sample<short>(short v) { return (float)v / 32768.0f; }

// grid (X, A): blocks x < X - 1 of record y compute its frames, four per block, one per wave; block X - 1 writes its new carry.  Both read carry buffer `sel`, the
// carry block writes the other one: no order between the blocks is needed.
template <typename T>
__global__ __launch_bounds__(256) void fbank_push_kernel(PushArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int* e = p.rec + (long)blockIdx.y * PUW;
    const int slot = e[0], n_prev = e[1], n_new = e[2], src = e[3], w0 = e[4], sel = e[6];
    if (n_new <= 0) return;
    const int t0 = num_frames(n_prev), t1 = num_frames(n_prev + n_new);
    const int c0 = t0 * HOP;                                           // the session's sample at carry[0]
    const float* carry = p.carry + ((long)slot * 2 + sel) * CARRY;
    const T* fresh = reinterpret_cast<const T*>(p.samples) + src;
    auto sample = [&](int s) { return s < n_prev ? carry[s - c0] : to_sample<T>(fresh[s - n_prev]); };      // s: index within the session
    if (blockIdx.x == gridDim.x - 1) {
        float* next = p.carry + ((long)slot * 2 + (1 - sel)) * CARRY;
        const int c1 = t1 * HOP, n = n_prev + n_new - c1;              // <= 399
        for (int i = threadIdx.x; i < n; i += 256) next[i] = sample(c1 + i);
        return;
    }
    if (t0 + (int)blockIdx.x * 4 >= t1) return;                        // block-uniform: no frame left for this block
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Lds L = setup(smem, p.tb);
    const int j = blockIdx.x * 4 + wave;
    if (t0 + j >= t1) return;                                          // wave-uniform, after the block's barriers
    const int base = (t0 + j) * HOP;
    float* o = p.fifo + ((long)slot * p.R + (w0 + j) % p.R) * p.tb.nmel;
    frame(p.tb, L, lane, [&](int n) { return sample(base + n); }, o, p.means, p.stds);
}

// grid (blocks, A): entry y's `rows` rows of out
__global__ __launch_bounds__(256) void fbank_pop_kernel(const float* __restrict__ fifo, int R, int nmel, const int* __restrict__ rec, float* __restrict__ out, int rows) {
    const int* e = rec + (long)blockIdx.y * POW;
    const int slot = e[0], r0 = e[1], n = e[2];
    const float* ring = fifo + (long)slot * R * nmel;
    float* o = out + (long)blockIdx.y * rows * nmel;
    const int total = rows * nmel;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int j = i / nmel, f = i - j * nmel;
        o[i] = j < n ? ring[(long)((r0 + j) % R) * nmel + f] : 0.f;
    }
}

bool geometry_ok(int slots, int R, int nmel) { return slots > 0 && R > 0 && nmel > 0 && nmel <= 127; }

size_t state_bytes(int slots, int R, int nmel) { return (size_t)slots * (2 * (size_t)CARRY + (size_t)R * nmel) * sizeof(float); }

// a slot named twice among the first i records (w words each)?
bool named_before(const int* rec, int w, int i) {
    for (int j = 0; j < i; ++j)
        if (rec[(long)j * w] == rec[(long)i * w]) return true;
    return false;
}

}  // namespace

// bytes of the state of `slots` slots with a ring of fifo_frames frames of nmel values each (header: the layout); 0: refused (a count < 1, nmel > 127).  Host only.
extern "C" size_t mi_fbank_stream_state_bytes(int slots, int fifo_frames, int nmel) {
    return geometry_ok(slots, fifo_frames, nmel) ? state_bytes(slots, fifo_frames, nmel) : 0;
}

// samples: n_samples values, fp32 (sample_dtype 0) or int16 (1); rec_host / rec_dev: A push records (header); window / twiddle / mel_t / mel_lo / mel_hi / mel_floor /
// preemph as mi_fbank_f64's; normalize 0: none, 1: global with means / stds (nmel) fp32.
extern "C" int mi_fbank_stream_push(void* state, size_t state_bytes_, int slots, int fifo_frames, int nmel, const void* samples, long n_samples, int sample_dtype,
                                    const int* rec_host, const int* rec_dev, int A, const double* window, const double* twiddle, const double* mel_t, const int* mel_lo,
                                    const int* mel_hi, const float* means, const float* stds, int normalize, double mel_floor, double preemph, hipStream_t stream) {
    MI_ENTER();
    if (!geometry_ok(slots, fifo_frames, nmel) || !state || state_bytes_ < state_bytes(slots, fifo_frames, nmel)) return MI_ERR_ARG;
    if (!rec_host || !rec_dev || A <= 0 || A > slots || A > 65535 || !window || !twiddle || !mel_t || !mel_lo || !mel_hi) return MI_ERR_ARG;
    if (sample_dtype < 0 || sample_dtype > 1 || n_samples < 0 || normalize < 0 || normalize > 1 || (normalize == 1 && (!means || !stds))) return MI_ERR_ARG;
    const int R = fifo_frames;
    int most = 0;
    for (int i = 0; i < A; ++i) {
        const int* e = rec_host + (long)i * PUW;
        const int slot = e[0], n_prev = e[1], n_new = e[2], src = e[3], w = e[4], count = e[5], sel = e[6];
        if (slot < 0 || slot >= slots || named_before(rec_host, PUW, i)) return MI_ERR_ARG;
        if (n_prev < 0 || n_new < 0 || (long)n_prev + n_new > 0x7fffffffL - FRAME || src < 0 || (long)src + n_new > n_samples) return MI_ERR_ARG;
        if (w < 0 || w >= R || count < 0 || count > R || (sel != 0 && sel != 1)) return MI_ERR_ARG;
        const int fresh = num_frames(n_prev + n_new) - num_frames(n_prev);
        if (count + fresh > R) return MI_ERR_ARG;                          // the ring would overrun frames not yet popped
        most = fresh > most ? fresh : most;
        if (n_new > 0 && !samples) return MI_ERR_ARG;
    }
    float* carry = (float*)state;
    PushArgs a{carry, carry + (size_t)slots * 2 * CARRY, samples, rec_dev, normalize ? means : nullptr, normalize ? stds : nullptr,
               Tables{window, twiddle, mel_t, mel_lo, mel_hi, nmel, mel_floor, preemph}, R};
    const dim3 grid(cdiv(most, 4) + 1, A);
    if (sample_dtype == 0) hipLaunchKernelGGL(fbank_push_kernel<float>, grid, dim3(256), LDS_BYTES, stream, a);
    else hipLaunchKernelGGL(fbank_push_kernel<short>, grid, dim3(256), LDS_BYTES, stream, a);
    MI_CHECK_LAUNCH();
    return MI_OK;
}

// rec_host / rec_dev: A pop records (header); out (A, rows, nmel) fp32, every element written.
extern "C" int mi_fbank_stream_pop(const void* state, size_t state_bytes_, int slots, int fifo_frames, int nmel, const int* rec_host, const int* rec_dev, int A, float* out,
                                   int rows, hipStream_t stream) {
    MI_ENTER();
    if (!geometry_ok(slots, fifo_frames, nmel) || !state || state_bytes_ < state_bytes(slots, fifo_frames, nmel)) return MI_ERR_ARG;
    if (!rec_host || !rec_dev || !out || A <= 0 || A > slots || A > 65535 || rows <= 0 || (long)rows * nmel > 0x7fffffffL) return MI_ERR_ARG;
    for (int i = 0; i < A; ++i) {
        const int* e = rec_host + (long)i * POW;
        if (e[0] < 0 || e[0] >= slots || named_before(rec_host, POW, i)) return MI_ERR_ARG;
        if (e[1] < 0 || e[1] >= fifo_frames || e[2] < 0 || e[2] > rows || e[2] > fifo_frames) return MI_ERR_ARG;
    }
    const float* fifo = (const float*)state + (size_t)slots * 2 * CARRY;
    const int gx = cdiv((long)rows * nmel, 256) < 64 ? cdiv((long)rows * nmel, 256) : 64;
    hipLaunchKernelGGL(fbank_pop_kernel, dim3(gx, A), dim3(256), 0, stream, fifo, fifo_frames, nmel, rec_dev, out, rows);
    MI_CHECK_LAUNCH();
    return MI_OK;
}
