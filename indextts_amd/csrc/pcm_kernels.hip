// Delivery formats: what turns the vocoder's 22.05 kHz f32 rows into the audio a request asked for, on the device.
//   pcm_resample_seq_kernel      rational polyphase resampler over packed ragged sequences, one-shot and streaming in one kernel
//   pcm_peak_seq_kernel          per-sequence max |x| (NaN ignored)
//   pcm_encode_seq_kernel        per-sequence gain, then pcm_s16le / mulaw / alaw / pcm_f32le
//   pcm_stream_piece_seq_kernel  RowStream.push / flush for all jobs of a render: Hann cross-fade, held-back tail, 512-sample fade-out
// Sequences are addressed through DEVICE int64 tables (one row per sequence), as the _seq_ entries of codec_kernels.hip address theirs
// through int32 ones; 64 bits because a stream's global sample index outgrows 31 bits within a day of audio.
#include "../../include/indextts_hip.h"
#include "common.h"

namespace {

// ---- (a) resampler ------------------------------------------------------------------------------------------------------------------
// y[m] = sum over i of h[m*M - i*L] * x[i], i ascending over |m*M - i*L| <= H inside the sequence: ONE f32 fmaf chain from 0.f per output, so
// the bits of y[m] depend on neither the tile, the block, the staging nor the neighbours in the packed buffer.  The prototype arrives laid
// out by output residue: table[k*L + (m mod L)] is the coefficient of the k-th input of output m's support (i = ceil((m*M - H)/L) + k); the
// lanes of a wave serve consecutive m, so they read consecutive coefficients.  A block serves PCM_TILE consecutive outputs of one sequence
// (grid.x tiles, grid.y sequences), 256 threads x 4 outputs; the tile's input span is staged in LDS when it fits the launch's LDS budget and
// read from global memory otherwise -- the same chain either way.
// seq row: { x_start, n_buf, in_offset, y_start, out_offset, n_out, final, 0 }: the buffer x[x_start .. x_start + n_buf) holds the stream's
// samples in_offset .. in_offset + n_buf (carried history + new piece); outputs out_offset .. out_offset + n_out go to y[y_start ..).  A
// non-final sequence leaves unwritten any output whose support reaches past the samples received so far (m*M + H >= n_in*L): the host never
// asks for one, and the kernel does not invent samples if it did.
constexpr int PCM_TILE = ITTS_PCM_RESAMPLE_TILE;
constexpr int PCM_THREADS = 256;
constexpr int PCM_PER_THREAD = PCM_TILE / PCM_THREADS;

__device__ __forceinline__ long long ceil_div_ll(long long a, long long b) {      // b > 0
    return a >= 0 ? (a + b - 1) / b : -((-a) / b);
}

__global__ __launch_bounds__(PCM_THREADS) void pcm_resample_seq_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                       const float* __restrict__ table, const long long* __restrict__ seq,
                                                                       int L, int M, int H, int lds_floats) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    const long long* row = seq + (size_t)blockIdx.y * 8;
    const long long n_out = row[5];
    const long long t0 = (long long)blockIdx.x * PCM_TILE;
    if (t0 >= n_out) return;
    const long long x_start = row[0], n_buf = row[1], in_off = row[2], y_start = row[3], out_off = row[4];
    const bool final = row[6] != 0;
    const long long n_in = in_off + n_buf;                               // samples of the stream received so far
    const long long lo_ok = in_off > 0 ? in_off : 0, hi_ok = n_in - 1;   // global input indices that exist in the buffer
    const long long t1 = (t0 + PCM_TILE < n_out ? t0 + PCM_TILE : n_out) - 1;
    // the tile's input span: supports are monotone in m, so [first output's low end, last output's high end] covers them all
    long long s_lo = ceil_div_ll((out_off + t0) * M - H, L), s_hi = ((out_off + t1) * M + H) / L;
    if (s_lo < lo_ok) s_lo = lo_ok;
    if (s_hi > hi_ok) s_hi = hi_ok;
    const long long span = s_hi - s_lo + 1;
    const bool staged = span <= (long long)lds_floats;
    const float* xg = x + x_start - in_off;                              // xg[i]: the stream's sample i
    if (staged) {
        for (int j = threadIdx.x; j < (int)span; j += PCM_THREADS) xs[j] = xg[s_lo + j];
        __syncthreads();
    }
#pragma unroll 1
    for (int u = 0; u < PCM_PER_THREAD; ++u) {
        const long long t = t0 + u * PCM_THREADS + threadIdx.x;
        if (t > t1) break;
        const long long m = out_off + t, c = m * M;
        if (!final && c + H >= n_in * L) continue;
        const long long i_lo = ceil_div_ll(c - H, L);
        long long lo = i_lo, hi = (c + H) / L;
        if (lo < lo_ok) lo = lo_ok;
        if (hi > hi_ok) hi = hi_ok;
        const int cnt = hi >= lo ? (int)(hi - lo + 1) : 0;
        const float* tp = table + (size_t)(lo - i_lo) * L + (int)(m % L);
        float acc = 0.f;
        if (staged) {
            const float* xp = xs + (lo - s_lo);
            for (int k = 0; k < cnt; ++k) acc = fmaf(tp[(size_t)k * L], xp[k], acc);
        } else {
            const float* xp = xg + lo;
            for (int k = 0; k < cnt; ++k) acc = fmaf(tp[(size_t)k * L], xp[k], acc);
        }
        y[y_start + t] = acc;
    }
}

// ---- (b) peak -----------------------------------------------------------------------------------------------------------------------
// seq row: { x_start, n }.  |x| of a non-NaN float orders as its bit pattern does, so the maximum is an integer atomicMax on the bits: exact
// and independent of the order.  fmaxf drops a NaN operand.  peak[] is zeroed by the entry on the same stream.
__global__ __launch_bounds__(256) void pcm_peak_seq_kernel(const float* __restrict__ x, float* __restrict__ peak, const long long* __restrict__ seq) {
    const long long n = seq[(size_t)blockIdx.y * 2 + 1];
    const float* xp = x + seq[(size_t)blockIdx.y * 2];
    float v = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) v = fmaxf(v, fabsf(xp[i]));
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0 && v > 0.f) atomicMax((unsigned int*)(peak + blockIdx.y), __float_as_uint(v));
}

// ---- (c) encode ---------------------------------------------------------------------------------------------------------------------
// G.711 of a 16-bit sample, table-free: the segment is found by comparing against the eight segment ends, as CPython's audioop does.
__device__ __forceinline__ int g711_segment(int v, int first_end) {          // first index whose end (first_end, then 2e+1, ...) holds v; 8: none
    int seg = 0, end = first_end;
    while (seg < 8 && v > end) { end = (end << 1) | 1; ++seg; }
    return seg;
}
__device__ __forceinline__ unsigned char g711_ulaw(int q) {                   // audioop.lin2ulaw(q, 2): the 14-bit coder on q >> 2
    int v = q >> 2, mask = 0xFF;
    if (v < 0) { v = -v; mask = 0x7F; }
    if (v > 8159) v = 8159;
    v += 0x84 >> 2;
    const int seg = g711_segment(v, 0x3F);
    if (seg >= 8) return (unsigned char)(0x7F ^ mask);
    return (unsigned char)(((seg << 4) | ((v >> (seg + 1)) & 0xF)) ^ mask);
}
__device__ __forceinline__ unsigned char g711_alaw(int q) {                   // audioop.lin2alaw(q, 2): the 13-bit coder on q >> 3
    int v = q >> 3, mask = 0xD5;
    if (v < 0) { mask = 0x55; v = -v - 1; }
    const int seg = g711_segment(v, 0x1F);
    if (seg >= 8) return (unsigned char)(0x7F ^ mask);
    const int low = seg < 2 ? (v >> 1) & 0xF : (v >> seg) & 0xF;
    return (unsigned char)(((seg << 4) | low) ^ mask);
}

// seq row: { x_start, n, y_start, 0 } (y_start in samples).  s = x * g with ONE f32 multiply, NaN -> 0; g = gain[seq], or gain[seq] / peak[seq]
// (an f32 division; a peak of 0 gives 1) when a peak table is given.
template <int ENC>
__global__ __launch_bounds__(256) void pcm_encode_seq_kernel(const float* __restrict__ x, void* __restrict__ y, const long long* __restrict__ seq,
                                                             const float* __restrict__ gain, const float* __restrict__ peak) {
    const long long* row = seq + (size_t)blockIdx.y * 4;
    const long long n = row[1];
    const float* xp = x + row[0];
    float g = gain[blockIdx.y];
    if (peak) { const float p = peak[blockIdx.y]; g = p == 0.f ? 1.f : g / p; }
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        float s = xp[i] * g;
        if (s != s) s = 0.f;
        if (ENC == ITTS_PCM_F32LE) {
            ((float*)y)[row[2] + i] = fminf(fmaxf(s, -1.f), 1.f);
        } else {
            const int q = (int)rintf(fminf(fmaxf(s * 32767.f, -32767.f), 32767.f));
            if (ENC == ITTS_PCM_S16LE) ((short*)y)[row[2] + i] = (short)q;
            else if (ENC == ITTS_PCM_MULAW) ((unsigned char*)y)[row[2] + i] = g711_ulaw(q);
            else ((unsigned char*)y)[row[2] + i] = g711_alaw(q);
        }
    }
}

// ---- (d) stream pieces ----------------------------------------------------------------------------------------------------------------
// job row (12 x int64): { tail_start, audio_start, piece_start, keep_start, n_blend, piece_len, keep_len, rest_src, keep_src, win_off, flags, 0 }
//   piece[j] = tail[j] * win[win_off + n_blend + j] + audio[j] * win[win_off + j]      for j < n_blend   (np.hanning(2 n_blend): falling | rising)
//            = src[rest_src + j - n_blend]                                              otherwise; src is the tail row when flags & 2 (a flush)
//   flags & 1: the last 512 samples of the piece are scaled by fade[0..512) (np.linspace(1, 0, 512))
//   keep[j]  = audio[keep_src + j]: the samples held back for the next chunk's head
// The window and fade tables are f32; each sample is formed in f64 from exact products and rounded to f32 once.
__global__ __launch_bounds__(256) void pcm_stream_piece_seq_kernel(const float* __restrict__ tails, const float* __restrict__ audio,
                                                                   float* __restrict__ piece, float* __restrict__ keep,
                                                                   const float* __restrict__ win, const float* __restrict__ fade,
                                                                   const long long* __restrict__ jobs) {
    const long long* r = jobs + (size_t)blockIdx.y * 12;
    const long long n_blend = r[4], piece_len = r[5], keep_len = r[6], flags = r[10];
    const float* tp = tails + r[0];
    const float* ap = audio + r[1];
    const float* rest = (flags & 2) ? tp : ap;
    const float* wp = win + r[9];
    const long long fade_from = (flags & 1) ? piece_len - ITTS_PCM_TAIL_FADE : piece_len;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < piece_len + keep_len; j += (long long)gridDim.x * 256) {
        if (j >= piece_len) { keep[r[3] + (j - piece_len)] = ap[r[8] + (j - piece_len)]; continue; }
        double v = j < n_blend ? (double)tp[j] * (double)wp[n_blend + j] + (double)ap[j] * (double)wp[j] : (double)rest[r[7] + (j - n_blend)];
        if (j >= fade_from) v *= (double)fade[j - fade_from];
        piece[r[2] + j] = (float)v;
    }
}

inline int blocks_for(long long n, int per_block, int cap) {
    long long b = (n + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

}  // namespace

extern "C" int itts_pcm_resample_tile(void) { return PCM_TILE; }

extern "C" int itts_pcm_resample_seq_forward(const float* x, float* y, const float* table, const int64_t* seq, int n_seq, int64_t max_n_out, int L,
                                             int M, int H, int K, void* stream) {
    if (!x || !y || !table || !seq || n_seq < 1 || n_seq > 65535 || L < 1 || M < 1 || H < 1 || K != (2 * (long long)H + L) / L ||
        (long long)K * L * 4 > ITTS_PCM_TABLE_MAX_BYTES || max_n_out < 0 || max_n_out > (int64_t)PCM_TILE * 0x7fffffffLL) {
        itts_set_error("pcm_resample_seq: bad args (non-null tensors, 1 <= n_seq <= 65535, L, M, H >= 1, K = ceil((2H + 1) / L), K * L * 4 <= %d, "
                       "max_n_out >= 0)", ITTS_PCM_TABLE_MAX_BYTES);
        return ITTS_ERR_ARG;
    }
    if (max_n_out == 0) return ITTS_OK;
    // LDS for a full tile's span, ((TILE - 1) * M + 2H) / L + 2 samples, when that fits 48 KiB; a wider span is read from global memory
    long long need = ((long long)(PCM_TILE - 1) * M + 2LL * H) / L + 2;
    const int lds_floats = need <= 12288 ? (int)need : 0;
    const dim3 grid((unsigned)((max_n_out + PCM_TILE - 1) / PCM_TILE), n_seq);
    hipLaunchKernelGGL(pcm_resample_seq_kernel, grid, dim3(PCM_THREADS), (size_t)lds_floats * 4, (hipStream_t)stream, x, y, table,
                       (const long long*)seq, L, M, H, lds_floats);
    HIP_TRY(hipGetLastError());
    return ITTS_OK;
}

extern "C" int itts_pcm_peak_seq_forward(const float* x, float* peak, const int64_t* seq, int n_seq, int64_t max_n, void* stream) {
    if (!x || !peak || !seq || n_seq < 1 || n_seq > 65535 || max_n < 0) {
        itts_set_error("pcm_peak_seq: bad args (non-null tensors, 1 <= n_seq <= 65535, max_n >= 0)");
        return ITTS_ERR_ARG;
    }
    HIP_TRY(hipMemsetAsync(peak, 0, (size_t)n_seq * 4, (hipStream_t)stream));
    if (max_n == 0) return ITTS_OK;
    hipLaunchKernelGGL(pcm_peak_seq_kernel, dim3(blocks_for(max_n, 256 * 8, 1024), n_seq), dim3(256), 0, (hipStream_t)stream, x, peak,
                       (const long long*)seq);
    HIP_TRY(hipGetLastError());
    return ITTS_OK;
}

extern "C" int itts_pcm_encode_seq_forward(const float* x, void* y, const int64_t* seq, int n_seq, int64_t max_n, int encoding, const float* gain,
                                           const float* peak, void* stream) {
    if (!x || !y || !seq || !gain || n_seq < 1 || n_seq > 65535 || max_n < 0 || encoding < ITTS_PCM_S16LE || encoding > ITTS_PCM_F32LE) {
        itts_set_error("pcm_encode_seq: bad args (non-null tensors, 1 <= n_seq <= 65535, max_n >= 0, encoding one of ITTS_PCM_*)");
        return ITTS_ERR_ARG;
    }
    if (max_n == 0) return ITTS_OK;
    const dim3 grid(blocks_for(max_n, 256 * 4, 1024), n_seq);
    const long long* sq = (const long long*)seq;
    hipStream_t st = (hipStream_t)stream;
    switch (encoding) {
        case ITTS_PCM_S16LE: hipLaunchKernelGGL(pcm_encode_seq_kernel<ITTS_PCM_S16LE>, grid, dim3(256), 0, st, x, y, sq, gain, peak); break;
        case ITTS_PCM_MULAW: hipLaunchKernelGGL(pcm_encode_seq_kernel<ITTS_PCM_MULAW>, grid, dim3(256), 0, st, x, y, sq, gain, peak); break;
        case ITTS_PCM_ALAW: hipLaunchKernelGGL(pcm_encode_seq_kernel<ITTS_PCM_ALAW>, grid, dim3(256), 0, st, x, y, sq, gain, peak); break;
        default: hipLaunchKernelGGL(pcm_encode_seq_kernel<ITTS_PCM_F32LE>, grid, dim3(256), 0, st, x, y, sq, gain, peak); break;
    }
    HIP_TRY(hipGetLastError());
    return ITTS_OK;
}

extern "C" int itts_pcm_stream_piece_seq_forward(const float* tails, const float* audio, float* piece, float* keep, const float* win,
                                                 const float* fade, const int64_t* jobs, int n_jobs, int64_t max_len, void* stream) {
    if (!tails || !audio || !piece || !keep || !win || !fade || !jobs || n_jobs < 1 || n_jobs > 65535 || max_len < 0) {
        itts_set_error("pcm_stream_piece_seq: bad args (non-null tensors, 1 <= n_jobs <= 65535, max_len >= 0)");
        return ITTS_ERR_ARG;
    }
    if (max_len == 0) return ITTS_OK;
    hipLaunchKernelGGL(pcm_stream_piece_seq_kernel, dim3(blocks_for(max_len, 256 * 4, 1024), n_jobs), dim3(256), 0, (hipStream_t)stream, tails,
                       audio, piece, keep, win, fade, (const long long*)jobs);
    HIP_TRY(hipGetLastError());
    return ITTS_OK;
}
