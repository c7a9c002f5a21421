// Look-ahead limiter and true-peak meter of the delivery stage, over the packed ragged sequences of pcm_kernels.hip.
//   pcm_truepeak_seq_kernel   per-sequence max |u|, u = the sequence oversampled 1 -> 4 by the resampler's own polyphase chain; no 4N buffer
//   pcm_limiter_seq_kernel    z[n] = clamp(x[n] g0 G[n], -c, c), G the smoothed look-ahead minimum of the required gain; one-shot and streaming
// Every output sample is a pure function of its own stream's samples within +-R (R = La, + 24 in true-peak mode): the bits depend on neither
// the tile, the batch, the piece boundaries of a stream nor the sequence's place in the buffer.
#include "../../include/indextts_hip.h"
#include "common.h"

namespace {

constexpr int LIM_TILE = ITTS_PCM_LIMITER_TILE;
constexpr int LIM_THREADS = 256;
constexpr int LIM_PER_THREAD = LIM_TILE / LIM_THREADS;
constexpr int TP_L = 4, TP_H = 96, TP_Z = 24;        // resample_params(1, 4): L = 4, M = 1, H = 96, K = 49

__device__ __forceinline__ long long ceil_div4(long long a) { return a >= 0 ? (a + 3) / 4 : -((-a) / 4); }

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// u[q], 0 <= q < 4 n_in: output q of pcm_resample_seq_kernel for the rate pair (1, 4) -- the same table, the same ascending fmaf chain from 0.f
// over the inputs that exist, i in [lo_ok, hi_ok].  xv[i - base] is the stream's sample i.  The meter and the limiter both come here.
__device__ __forceinline__ float truepeak_u(const float* xv, long long base, long long lo_ok, long long hi_ok, const float* __restrict__ table4,
                                            long long q) {
    const long long i_lo = ceil_div4(q - TP_H);
    long long lo = i_lo, hi = (q + TP_H) / TP_L;
    if (lo < lo_ok) lo = lo_ok;
    if (hi > hi_ok) hi = hi_ok;
    const int cnt = hi >= lo ? (int)(hi - lo + 1) : 0;
    const float* tp = table4 + (lo - i_lo) * TP_L + (int)(q & 3);
    const float* xp = xv + (lo - base);
    float acc = 0.f;
    for (int k = 0; k < cnt; ++k) acc = fmaf(tp[k * TP_L], xp[k], acc);
    return acc;
}

// seq row: { x_start, n }.  A block serves LIM_TILE consecutive q of one sequence; its inputs, at most LIM_TILE / 4 + 2 Z + 1, are staged in LDS.
// fmaxf drops a NaN operand; the maximum is an integer atomicMax on the bits, as in pcm_peak_seq_kernel.  peak[] is zeroed by the entry.
constexpr int TP_STAGE = LIM_TILE / TP_L + 2 * TP_Z + 1;
__global__ __launch_bounds__(LIM_THREADS) void pcm_truepeak_seq_kernel(const float* __restrict__ x, float* __restrict__ peak,
                                                                       const float* __restrict__ table4, const long long* __restrict__ seq) {
    __shared__ float xs[TP_STAGE];
    const long long n = seq[(size_t)blockIdx.y * 2 + 1];
    const long long q0 = (long long)blockIdx.x * LIM_TILE;
    if (q0 >= 4 * n) return;
    const float* xp = x + seq[(size_t)blockIdx.y * 2];
    const long long q1 = (q0 + LIM_TILE < 4 * n ? q0 + LIM_TILE : 4 * n) - 1;
    long long s_lo = ceil_div4(q0 - TP_H), s_hi = (q1 + TP_H) / TP_L;
    if (s_lo < 0) s_lo = 0;
    if (s_hi > n - 1) s_hi = n - 1;
    for (int j = threadIdx.x; j < (int)(s_hi - s_lo + 1); j += LIM_THREADS) xs[j] = xp[s_lo + j];
    __syncthreads();
    float v = 0.f;
    for (long long q = q0 + threadIdx.x; q <= q1; q += LIM_THREADS) v = fmaxf(v, fabsf(truepeak_u(xs, s_lo, 0, n - 1, table4, q)));
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0 && v > 0.f) atomicMax((unsigned int*)(peak + blockIdx.y), __float_as_uint(v));
}

// seq row: the resampler's, { x_start, n_buf, in_offset, y_start, out_offset, n_out, final, 0 }.  A block serves up to LIM_TILE consecutive
// outputs n0 .. n0 + T of one sequence.  LDS, in floats:
//   xs [T + 2R]    the stream's samples n0 - R ..            (0 where the stream has none)
//   rs [T + 2La]   required gain r[n0 - La ..]               (1 outside [0, n_in))
//   ms [T + La]    m[j] = min r[j .. j + La], j = n0 - La ..  (exact: any order gives the same bits)
//   ws [La + 1]    the smoothing window
// then per output ONE fmaf chain over k ascending of w[k] (1 - m[n - k]) from 0.f.  At La = 1024 in true-peak mode: 9265 floats, under 40 KiB.
// A non-final sequence leaves unwritten any output with n + R >= n_in; the host never asks for one.
__global__ __launch_bounds__(LIM_THREADS) void pcm_limiter_stats_init_kernel(float* stats, int n_seq) {
    const int i = blockIdx.x * LIM_THREADS + threadIdx.x;
    if (i < n_seq) { stats[2 * i] = 1.f; stats[2 * i + 1] = 0.f; }
}

template <bool TP>
__global__ __launch_bounds__(LIM_THREADS) void pcm_limiter_seq_kernel(const float* __restrict__ x, float* __restrict__ z,
                                                                      const float* __restrict__ window, const float* __restrict__ table4,
                                                                      const long long* __restrict__ seq, int La, const float* __restrict__ gain,
                                                                      float c, float* __restrict__ stats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const long long* row = seq + (size_t)blockIdx.y * 8;
    const long long n_out = row[5];
    const long long t0 = (long long)blockIdx.x * LIM_TILE;
    if (t0 >= n_out) return;
    const long long x_start = row[0], n_buf = row[1], in_off = row[2], y_start = row[3], out_off = row[4];
    const bool final = row[6] != 0;
    const long long n_in = in_off + n_buf;
    const long long lo_ok = in_off > 0 ? in_off : 0, hi_ok = n_in - 1;
    const int T = (int)(n_out - t0 < LIM_TILE ? n_out - t0 : LIM_TILE);
    const int R = La + (TP ? TP_Z : 0);
    const long long n0 = out_off + t0;
    float* xs = lds;
    float* rs = xs + LIM_TILE + 2 * R;
    float* ms = rs + LIM_TILE + 2 * La;
    float* ws = ms + LIM_TILE + La;
    const float* xg = x + x_start - in_off;                              // xg[i]: the stream's sample i
    const float g0 = gain[blockIdx.y];

    for (int j = threadIdx.x; j < T + 2 * R; j += LIM_THREADS) {
        const long long i = n0 - R + j;
        xs[j] = (i >= lo_ok && i <= hi_ok) ? xg[i] : 0.f;
    }
    for (int k = threadIdx.x; k <= La; k += LIM_THREADS) ws[k] = window[k];
    __syncthreads();

    for (int j = threadIdx.x; j < T + 2 * La; j += LIM_THREADS) {
        const long long i = n0 - La + j;
        float r = 1.f;
        if (i >= 0 && i < n_in) {
            float a;
            if (TP) {
                float v = 0.f;
#pragma unroll 1
                for (int p = -3; p <= 3; ++p) {
                    const long long q = 4 * i + p;
                    if (q >= 0 && q < 4 * n_in) v = fmaxf(v, fabsf(truepeak_u(xs, n0 - R, lo_ok, hi_ok, table4, q)));
                }
                a = v * fabsf(g0);
            } else {
                a = fabsf(xs[j] * g0);                                   // R == La: xs and rs share their origin
            }
            if (a > c) r = c / a;                                        // a NaN compares false: it asks for nothing
        }
        rs[j] = r;
    }
    __syncthreads();

    for (int j = threadIdx.x; j < T + La; j += LIM_THREADS) {
        float m = rs[j];
        for (int k = 1; k <= La; ++k) m = fminf(m, rs[j + k]);
        ms[j] = m;
    }
    __syncthreads();

    float g_min = 1.f, z_max = 0.f;
#pragma unroll 1
    for (int u = 0; u < LIM_PER_THREAD; ++u) {
        const int t = u * LIM_THREADS + threadIdx.x;
        if (t >= T) break;
        const long long n = n0 + t;
        if (!final && n + R >= n_in) continue;
        const float* mp = ms + t + La;                                   // mp[-k] = m[n - k]
        float acc = 0.f;
        for (int k = 0; k <= La; ++k) acc = fmaf(ws[k], 1.f - mp[-k], acc);
        const float G = 1.f - acc;
        float v = (xs[t + R] * g0) * G;
        if (v != v) v = 0.f;
        v = fminf(fmaxf(v, -c), c);
        z[y_start + t0 + t] = v;
        g_min = fminf(g_min, fmaxf(G, 0.f));
        z_max = fmaxf(z_max, fabsf(v));
    }
    if (stats) {
        g_min = wave_min(g_min);
        z_max = wave_max(z_max);
        if ((threadIdx.x & 63) == 0) {
            if (g_min < 1.f) atomicMin((unsigned int*)(stats + 2 * blockIdx.y), __float_as_uint(g_min));
            if (z_max > 0.f) atomicMax((unsigned int*)(stats + 2 * blockIdx.y + 1), __float_as_uint(z_max));
        }
    }
}

}  // namespace

extern "C" int itts_pcm_limiter_lookahead(int rate) {
    if (rate < 1) return 0;
    const long long la = ((long long)rate * 5 + 500) / 1000;
    return la > 0x7fffffffLL ? 0x7fffffff : (int)la;
}

extern "C" int itts_pcm_truepeak_seq_forward(const float* x, float* peak, const float* table4, const int64_t* seq, int n_seq, int64_t max_n,
                                             void* stream) {
    if (!x || !peak || !table4 || !seq || n_seq < 1 || n_seq > 65535 || max_n < 0 || max_n > (int64_t)(LIM_TILE / TP_L) * 0x7fffffffLL) {
        itts_set_error("pcm_truepeak_seq: bad args (non-null tensors, 1 <= n_seq <= 65535, max_n >= 0)");
        return ITTS_ERR_ARG;
    }
    HIP_TRY(hipMemsetAsync(peak, 0, (size_t)n_seq * 4, (hipStream_t)stream));
    if (max_n == 0) return ITTS_OK;
    const dim3 grid((unsigned)((max_n * TP_L + LIM_TILE - 1) / LIM_TILE), n_seq);
    hipLaunchKernelGGL(pcm_truepeak_seq_kernel, grid, dim3(LIM_THREADS), 0, (hipStream_t)stream, x, peak, table4, (const long long*)seq);
    HIP_TRY(hipGetLastError());
    return ITTS_OK;
}

extern "C" int itts_pcm_limiter_seq_forward(const float* x, float* z, const float* window, const float* table4, const int64_t* seq, int n_seq,
                                            int64_t max_n_out, int lookahead, const float* gain, float ceiling, float* stats, void* stream) {
    if (!x || !z || !window || !seq || !gain || n_seq < 1 || n_seq > 65535 || max_n_out < 0 || max_n_out > (int64_t)LIM_TILE * 0x7fffffffLL ||
        lookahead < 1 || lookahead > ITTS_PCM_LIMITER_MAX_LOOKAHEAD || !(ceiling > 0.f) || !(ceiling <= 1.f)) {
        itts_set_error("pcm_limiter_seq: bad args (non-null tensors, 1 <= n_seq <= 65535, max_n_out >= 0, 1 <= lookahead <= %d, 0 < ceiling <= 1)",
                       ITTS_PCM_LIMITER_MAX_LOOKAHEAD);
        return ITTS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    if (stats) {
        hipLaunchKernelGGL(pcm_limiter_stats_init_kernel, dim3((n_seq + LIM_THREADS - 1) / LIM_THREADS), dim3(LIM_THREADS), 0, st, stats, n_seq);
        HIP_TRY(hipGetLastError());
    }
    if (max_n_out == 0) return ITTS_OK;
    const int R = lookahead + (table4 ? TP_Z : 0);
    const size_t lds = (size_t)(3 * LIM_TILE + 2 * R + 4 * lookahead + 1) * sizeof(float);
    const dim3 grid((unsigned)((max_n_out + LIM_TILE - 1) / LIM_TILE), n_seq);
    const long long* sq = (const long long*)seq;
    if (table4)
        hipLaunchKernelGGL(pcm_limiter_seq_kernel<true>, grid, dim3(LIM_THREADS), lds, st, x, z, window, table4, sq, lookahead, gain, ceiling, stats);
    else
        hipLaunchKernelGGL(pcm_limiter_seq_kernel<false>, grid, dim3(LIM_THREADS), lds, st, x, z, window, table4, sq, lookahead, gain, ceiling, stats);
    HIP_TRY(hipGetLastError());
    return ITTS_OK;
}
