// Loudness normalisation of the delivery formats: integrated loudness after ITU-R BS.1770-4 / EBU R 128 of packed ragged
// f32 sequences, measured on the device, and the per-sequence gain that brings a sequence to a target.
//   loud_chunk_kernel<false>   (a) every 100 ms sub-block filtered from ZERO output state with its true input history: its four end-state values
//   loud_chain_kernel          (b) per sequence, the true state at every sub-block boundary: s[k+1] = e[k] + Phi s[k], Phi the hop-step transition
//   loud_chunk_kernel<true>    (c) every sub-block filtered again from its true state, y^2 summed into S[k]; the sequence's max |x| on the way
//   loud_gate_kernel           (d) per sequence the 400 ms blocks, the absolute and the relative gate, L in LUFS
//   loud_gain_kernel           (L, peak, target, ceiling) -> the f32 gain pcm_encode_seq_kernel multiplies by
// The K-weighting is a 4th-order IIR (a shelf and a high-pass biquad, direct form 1); it is linear, so the state a sub-block starts from is the
// state it would reach from zero plus what the earlier state decays to -- which is what lets every sub-block run on a lane of its own.  State
// and sums are f64; every sum has one order, counted from the sequence's own start, so a sequence's bits depend on neither its batch nor its
// place in the buffer.
#include <math.h>

#include "../../include/indextts_hip.h"
#include "common.h"

namespace {

constexpr int LOUD_LANES = 64;            // sub-blocks a block of (a) / (c) serves: one per lane
constexpr int LOUD_TILE = 64;             // samples of every sub-block staged per round
constexpr int LOUD_PITCH = LOUD_TILE + 1; // LDS row pitch in floats: odd, so the lanes' column reads fall on distinct banks
constexpr int LOUD_GATE_THREADS = 1024;

struct LoudCoef {
    double b0, b1, b2, a1, a2;            // stage 1 (shelf)
    double c1, c2;                        // stage 2 (high-pass, b = [1, -2, 1])
    double phi[16];                       // the hop-step transition of (y1[-1], y1[-2], y2[-1], y2[-2]) under zero input, row-major
};

// seq row: { x_start, n, sub_start, 0 }: the sequence's floor(n / hop) sub-blocks own the workspace rows sub_start .. (the host lays them out).
// A row whose sub-blocks would leave the workspace is not served at all (its L is NaN): nothing is written outside the workspace.
__device__ __forceinline__ bool loud_row(const long long* seq, int s, int hop, long long total_sub, long long& x_start, long long& n,
                                         long long& sub_start, long long& n_sub) {
    const long long* r = seq + (size_t)s * 4;
    x_start = r[0], n = r[1], sub_start = r[2];
    n_sub = n / hop;
    return n >= 0 && sub_start >= 0 && sub_start + n_sub <= total_sub;
}

// (a) and (c).  Lane l of block bx serves sub-block k = bx * 64 + l: samples [k hop, (k + 1) hop) of its sequence.  The lanes' samples lie `hop`
// floats apart, so each round stages 64 samples of all 64 sub-blocks through LDS: a row of the tile is one coalesced 256-byte read, and the
// lanes then walk their own rows (pitch 65: conflict-free).  SUM = false: from zero output state, the end state goes to ends[k].  SUM = true:
// from starts[k], the sum of y2^2 in sample order goes to sums[k]; the chunk after the last whole sub-block takes part for the peak only.
template <bool SUM>
__global__ __launch_bounds__(LOUD_LANES) void loud_chunk_kernel(const float* __restrict__ x, const long long* __restrict__ seq, int hop,
                                                                 long long total_sub, LoudCoef cf, double* __restrict__ ends,
                                                                 const double* __restrict__ starts, double* __restrict__ sums,
                                                                 float* __restrict__ peak) {
    __shared__ float xs[LOUD_LANES * LOUD_PITCH];
    long long x_start, n, sub_start, n_sub;
    if (!loud_row(seq, blockIdx.y, hop, total_sub, x_start, n, sub_start, n_sub)) return;
    const long long k0 = (long long)blockIdx.x * LOUD_LANES;
    const long long n_chunks = SUM && peak ? (n + hop - 1) / hop : (SUM ? n_sub : n_sub - 1);      // (a) needs no end state of the last sub-block
    if (k0 >= n_chunks) return;
    const float* xp = x + x_start;
    const int lane = threadIdx.x;
    const long long k = k0 + lane;
    const bool filt = k < (SUM ? n_sub : n_sub - 1);
    const long long base = k * hop;
    // input history: the two samples before the sub-block (zero before the sequence's start); a NaN sample counts as 0
    double x1 = 0.0, x2 = 0.0, p1 = 0.0, p2 = 0.0, q1 = 0.0, q2 = 0.0, acc = 0.0;
    if (filt) {
        if (base >= 1) { const float v = xp[base - 1]; x1 = v != v ? 0.0 : (double)v; }
        if (base >= 2) { const float v = xp[base - 2]; x2 = v != v ? 0.0 : (double)v; }
        if (SUM) {
            const double* s = starts + (size_t)(sub_start + k) * 4;
            p1 = s[0], p2 = s[1], q1 = s[2], q2 = s[3];
        }
    }
    float pk = 0.f;
    // The tile of round t0 + 64 is fetched into registers while round t0 is filtered out of LDS, so the memory latency of a round hides behind
    // the arithmetic of the one before.  The loads are unconditional (the index is clamped into the sequence, the value selected afterwards):
    // all 64 of a round are in flight together.
    float next[LOUD_LANES];
    const long long last = n - 1;                                    // n >= 1: this block has a chunk to serve
#pragma unroll
    for (int r = 0; r < LOUD_LANES; ++r) {                           // row r: sub-block k0 + r, its samples 0 .. 64; lane = column
        const long long i = (k0 + r) * hop + lane;
        const float v = xp[i < last ? i : last];
        next[r] = (lane < hop && i <= last) ? v : 0.f;
    }
    const double na1 = -cf.a1, na2 = -cf.a2, nc1 = -cf.c1, nc2 = -cf.c2;
    for (int t0 = 0; t0 < hop; t0 += LOUD_TILE) {
        const int cols = hop - t0 < LOUD_TILE ? hop - t0 : LOUD_TILE;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < LOUD_LANES; ++r) xs[r * LOUD_PITCH + lane] = next[r];
        __syncthreads();
        if (t0 + LOUD_TILE < hop) {
#pragma unroll
            for (int r = 0; r < LOUD_LANES; ++r) {
                const long long i = (k0 + r) * hop + t0 + LOUD_TILE + lane;
                const float v = xp[i < last ? i : last];
                next[r] = (t0 + LOUD_TILE + lane < hop && i <= last) ? v : 0.f;
            }
        }
        const float* mine = xs + lane * LOUD_PITCH;
        if (SUM && peak)
            for (int t = 0; t < cols; ++t) pk = fmaxf(pk, fabsf(mine[t]));                         // fmaxf drops a NaN operand
        if (filt) {
            // direct form 1, every product an fma in one fixed order; only the last fma of each stage waits for the sample before
            for (int t = 0; t < cols; ++t) {
                const float v = mine[t];
                const double x0 = v != v ? 0.0 : (double)v;
                const double f1 = fma(cf.b0, x0, fma(cf.b1, x1, fma(cf.b2, x2, na2 * p2)));
                const double y1 = fma(na1, p1, f1);
                const double f2 = fma(nc2, q2, fma(-2.0, p1, p2));
                const double y2 = fma(nc1, q1, y1 + f2);
                x2 = x1, x1 = x0, p2 = p1, p1 = y1, q2 = q1, q1 = y2;
                if (SUM) acc = fma(y2, y2, acc);
            }
        }
    }
    if (filt) {
        if (SUM) {
            sums[sub_start + k] = acc;
        } else {
            double* e = ends + (size_t)(sub_start + k) * 4;
            e[0] = p1, e[1] = p2, e[2] = q1, e[3] = q2;
        }
    }
    if (SUM && peak) {
        pk = wave_max(pk);
        if (lane == 0 && pk > 0.f) atomicMax((unsigned int*)(peak + blockIdx.y), __float_as_uint(pk));      // exact and order-free, as pcm_peak_seq
    }
}

// (b) one wave per sequence.  The chain is the one serial part: 16 fmas per sub-block on lane 0.  The end states arrive, and the start states
// leave, 64 sub-blocks at a time through LDS, so the memory latency is paid once per 64 steps and not once per step.
__global__ __launch_bounds__(LOUD_LANES) void loud_chain_kernel(const long long* __restrict__ seq, int hop, long long total_sub, LoudCoef cf,
                                                                 const double* __restrict__ ends, double* __restrict__ starts) {
    __shared__ double es[LOUD_LANES][4], ss[LOUD_LANES][4];
    long long x_start, n, sub_start, n_sub;
    if (!loud_row(seq, blockIdx.x, hop, total_sub, x_start, n, sub_start, n_sub)) return;
    const int lane = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;                   // lane 0's: the state at the boundary before sub-block k
    for (long long k0 = 0; k0 < n_sub; k0 += LOUD_LANES) {
        const int cnt = n_sub - k0 < LOUD_LANES ? (int)(n_sub - k0) : LOUD_LANES;
        __syncthreads();
        if (lane < cnt && k0 + lane < n_sub - 1) {                   // the last sub-block has no end state: nothing follows it
            const double* e = ends + (size_t)(sub_start + k0 + lane) * 4;
            es[lane][0] = e[0], es[lane][1] = e[1], es[lane][2] = e[2], es[lane][3] = e[3];
        }
        __syncthreads();
        if (lane == 0) {
            for (int j = 0; j < cnt; ++j) {
                ss[j][0] = s0, ss[j][1] = s1, ss[j][2] = s2, ss[j][3] = s3;
                if (k0 + j >= n_sub - 1) break;
                const double* p = cf.phi;
                const double t0 = es[j][0] + (p[0] * s0 + p[1] * s1 + p[2] * s2 + p[3] * s3);
                const double t1 = es[j][1] + (p[4] * s0 + p[5] * s1 + p[6] * s2 + p[7] * s3);
                const double t2 = es[j][2] + (p[8] * s0 + p[9] * s1 + p[10] * s2 + p[11] * s3);
                const double t3 = es[j][3] + (p[12] * s0 + p[13] * s1 + p[14] * s2 + p[15] * s3);
                s0 = t0, s1 = t1, s2 = t2, s3 = t3;
            }
        }
        __syncthreads();
        if (lane < cnt) {
            double* s = starts + (size_t)(sub_start + k0 + lane) * 4;
            s[0] = ss[lane][0], s[1] = ss[lane][1], s[2] = ss[lane][2], s[3] = ss[lane][3];
        }
    }
}

// a block-wide sum of (value, count) with one order: thread t's own terms in ascending j, then the halving tree over the 1024 slots
__device__ __forceinline__ void loud_block_sum(double* vs, int* cs, double& v, int& c) {
    const int t = threadIdx.x;
    __syncthreads();
    vs[t] = v, cs[t] = c;
    __syncthreads();
    for (int s = LOUD_GATE_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) vs[t] += vs[t + s], cs[t] += cs[t + s];
        __syncthreads();
    }
    v = vs[0], c = cs[0];
}

// (d) one block per sequence: z_j = (S_j + S_j+1 + S_j+2 + S_j+3) / (4 hop) for the n_sub - 3 blocks; keep l_j > -70, then l_j > (the loudness
// of the kept) - 10, compared as mean squares (l = -0.691 + 10 log10 z is monotone); L = -0.691 + 10 log10 mean(z over the kept), -inf when
// fewer than four sub-blocks or nothing passes.
__global__ __launch_bounds__(LOUD_GATE_THREADS) void loud_gate_kernel(const long long* __restrict__ seq, int hop, long long total_sub,
                                                                       const double* __restrict__ sums, double* __restrict__ lufs) {
    __shared__ double vs[LOUD_GATE_THREADS];
    __shared__ int cs[LOUD_GATE_THREADS];
    long long x_start, n, sub_start, n_sub;
    if (!loud_row(seq, blockIdx.x, hop, total_sub, x_start, n, sub_start, n_sub)) {
        if (threadIdx.x == 0) lufs[blockIdx.x] = __builtin_nan("");
        return;
    }
    const long long n_blk = n_sub - 3;
    const double* S = sums + sub_start;
    const double inv = 1.0 / (4.0 * (double)hop);
    const double z_abs = pow(10.0, (-70.0 + 0.691) / 10.0);          // the mean square whose loudness is -70
    double v = 0.0;
    int c = 0;
    for (long long j = threadIdx.x; j < n_blk; j += LOUD_GATE_THREADS) {
        const double z = (((S[j] + S[j + 1]) + S[j + 2]) + S[j + 3]) * inv;
        if (z > z_abs) v += z, ++c;
    }
    loud_block_sum(vs, cs, v, c);
    double out = -INFINITY;
    if (c > 0) {                                                     // uniform: every thread holds the same totals
        const double z_rel = 0.1 * (v / (double)c);                  // 10 LU under the loudness of the abs-gated blocks
        v = 0.0, c = 0;
        for (long long j = threadIdx.x; j < n_blk; j += LOUD_GATE_THREADS) {
            const double z = (((S[j] + S[j + 1]) + S[j + 2]) + S[j + 3]) * inv;
            if (z > z_abs && z > z_rel) v += z, ++c;
        }
        loud_block_sum(vs, cs, v, c);
        if (c > 0) out = -0.691 + 10.0 * log10(v / (double)c);
    }
    if (threadIdx.x == 0) lufs[blockIdx.x] = out;
}

// g = f32(10^((target - L) / 20)) formed in f64 and rounded once, 1 when nothing was measurable; under a ceiling, at most ceiling / peak (the
// f32 division of pcm_encode_seq_kernel).  report (optional) [n][3] = { L, 20 log10 g, 20 log10 of the delivered peak min(peak * g, 1) }.
__global__ __launch_bounds__(256) void loud_gain_kernel(const double* __restrict__ lufs, const float* __restrict__ peak, float* __restrict__ gain,
                                                         double* __restrict__ report, int n, double target, int has_ceiling, float ceiling) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double L = lufs[i];
    float g = L > -INFINITY ? (float)pow(10.0, (target - L) / 20.0) : 1.f;                        // NaN compares false: g = 1
    const float p = peak ? peak[i] : 0.f;
    if (has_ceiling && p > 0.f) g = fminf(g, ceiling / p);
    gain[i] = g;
    if (report) {
        report[(size_t)i * 3 + 0] = L;
        report[(size_t)i * 3 + 1] = 20.0 * log10((double)g);
        report[(size_t)i * 3 + 2] = peak ? 20.0 * log10((double)fminf(p * g, 1.f)) : __builtin_nan("");
    }
}

void mat4_mul(const double* a, const double* b, double* out) {
    double t[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            double s = 0.0;
            for (int k = 0; k < 4; ++k) s += a[i * 4 + k] * b[k * 4 + j];
            t[i * 4 + j] = s;
        }
    for (int i = 0; i < 16; ++i) out[i] = t[i];
}

bool loud_coefficients(int rate, double* out) {
    if (rate < ITTS_PCM_LOUDNESS_MIN_RATE || rate > ITTS_PCM_LOUDNESS_MAX_RATE) return false;
    const double pi = 3.14159265358979323846, fs = (double)rate;
    {   // stage 1: the high shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
        out[0] = (Vh + Vb * K / Q + K * K) / a0;
        out[1] = 2.0 * (K * K - Vh) / a0;
        out[2] = (Vh - Vb * K / Q + K * K) / a0;
        out[3] = 2.0 * (K * K - 1.0) / a0;
        out[4] = (1.0 - K / Q + K * K) / a0;
    }
    {   // stage 2: the high-pass, b = [1, -2, 1]
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        out[5] = 2.0 * (K * K - 1.0) / a0;
        out[6] = (1.0 - K / Q + K * K) / a0;
    }
    // one zero-input step of s = (y1[-1], y1[-2], y2[-1], y2[-2]): y1 = -a1 p1 - a2 p2, y2 = y1 - 2 p1 + p2 - c1 q1 - c2 q2; Phi = A^hop by squaring
    const double a1 = out[3], a2 = out[4], c1 = out[5], c2 = out[6];
    double A[16] = {-a1, -a2, 0, 0, 1, 0, 0, 0, -a1 - 2.0, 1.0 - a2, -c1, -c2, 0, 0, 1, 0};
    double P[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int e = (rate + 5) / 10; e > 0; e >>= 1) {
        if (e & 1) mat4_mul(P, A, P);
        mat4_mul(A, A, A);
    }
    for (int i = 0; i < 16; ++i) out[7 + i] = P[i];
    return true;
}

}  // namespace

extern "C" int itts_pcm_loudness_hop(int rate) { return rate < 1 ? 0 : (int)(((long long)rate + 5) / 10); }

extern "C" int itts_pcm_loudness_coefficients(int rate, double* out) {
    if (!out || !loud_coefficients(rate, out)) {
        itts_set_error("pcm_loudness_coefficients: bad args (non-null out, %d <= rate <= %d)", ITTS_PCM_LOUDNESS_MIN_RATE, ITTS_PCM_LOUDNESS_MAX_RATE);
        return ITTS_ERR_ARG;
    }
    return ITTS_OK;
}

extern "C" size_t itts_pcm_loudness_workspace_bytes(int64_t total_sub) {
    return total_sub < 0 ? 0 : (size_t)(total_sub > 0 ? total_sub : 1) * ITTS_PCM_LOUDNESS_WS_DOUBLES * sizeof(double);
}

extern "C" int itts_pcm_loudness_seq_forward(const float* x, double* lufs, float* peak, const int64_t* seq, int n_seq, int64_t max_n, int rate,
                                             int64_t total_sub, void* workspace, size_t workspace_bytes, void* stream) {
    LoudCoef cf;
    if (!x || !lufs || !seq || !workspace || n_seq < 1 || n_seq > 65535 || max_n < 0 || total_sub < 0 || !loud_coefficients(rate, &cf.b0) ||
        workspace_bytes < itts_pcm_loudness_workspace_bytes(total_sub) || ((uintptr_t)workspace & 7) ||
        max_n / itts_pcm_loudness_hop(rate) / LOUD_LANES >= 0x7fffffffLL) {
        itts_set_error("pcm_loudness_seq: bad args (non-null tensors, 1 <= n_seq <= 65535, max_n >= 0, %d <= rate <= %d, total_sub >= 0, an 8-byte "
                       "aligned workspace of itts_pcm_loudness_workspace_bytes(total_sub))", ITTS_PCM_LOUDNESS_MIN_RATE, ITTS_PCM_LOUDNESS_MAX_RATE);
        return ITTS_ERR_ARG;
    }
    static_assert(sizeof(LoudCoef) == 23 * sizeof(double), "LoudCoef is the 23 doubles of itts_pcm_loudness_coefficients");
    const int hop = itts_pcm_loudness_hop(rate);
    hipStream_t st = (hipStream_t)stream;
    const size_t rows = (size_t)(total_sub > 0 ? total_sub : 1);
    double* ends = (double*)workspace;
    double* starts = ends + rows * 4;
    double* sums = starts + rows * 4;
    const long long* sq = (const long long*)seq;
    if (peak) HIP_TRY(hipMemsetAsync(peak, 0, (size_t)n_seq * 4, st));
    const long long max_sub = max_n / hop, max_chunks = (max_n + hop - 1) / hop;
    if (max_sub > 1)
        hipLaunchKernelGGL(loud_chunk_kernel<false>, dim3((unsigned)((max_sub - 1 + LOUD_LANES - 1) / LOUD_LANES), n_seq), dim3(LOUD_LANES), 0, st, x,
                           sq, hop, (long long)total_sub, cf, ends, (const double*)nullptr, (double*)nullptr, (float*)nullptr);
    if (max_sub > 0)
        hipLaunchKernelGGL(loud_chain_kernel, dim3(n_seq), dim3(LOUD_LANES), 0, st, sq, hop, (long long)total_sub, cf, (const double*)ends, starts);
    const long long c_chunks = peak ? max_chunks : max_sub;
    if (c_chunks > 0)
        hipLaunchKernelGGL(loud_chunk_kernel<true>, dim3((unsigned)((c_chunks + LOUD_LANES - 1) / LOUD_LANES), n_seq), dim3(LOUD_LANES), 0, st, x, sq,
                           hop, (long long)total_sub, cf, (double*)nullptr, (const double*)starts, sums, peak);
    hipLaunchKernelGGL(loud_gate_kernel, dim3(n_seq), dim3(LOUD_GATE_THREADS), 0, st, sq, hop, (long long)total_sub, (const double*)sums, lufs);
    HIP_TRY(hipGetLastError());
    return ITTS_OK;
}

extern "C" int itts_pcm_loudness_gain_forward(const double* lufs, const float* peak, float* gain, double* report, int n_seq, double target_lufs,
                                              int has_ceiling, double ceiling_dbfs, void* stream) {
    if (!lufs || !gain || n_seq < 1 || n_seq > 65535 || !(target_lufs >= -70.0 && target_lufs <= 0.0) ||
        (has_ceiling && (!peak || !(ceiling_dbfs <= 0.0) || !(ceiling_dbfs > -INFINITY)))) {
        itts_set_error("pcm_loudness_gain: bad args (non-null lufs and gain, 1 <= n_seq <= 65535, -70 <= target_lufs <= 0; a ceiling needs a peak "
                       "table and a finite ceiling_dbfs <= 0)");
        return ITTS_ERR_ARG;
    }
    const float ceiling = has_ceiling ? (float)pow(10.0, ceiling_dbfs / 20.0) : 1.f;
    hipLaunchKernelGGL(loud_gain_kernel, dim3((n_seq + 255) / 256), dim3(256), 0, (hipStream_t)stream, lufs, peak, gain, report, n_seq, target_lufs,
                       has_ceiling ? 1 : 0, ceiling);
    HIP_TRY(hipGetLastError());
    return ITTS_OK;
}
