// Launcher prototypes for the GPT decoder kernels (gpt_kernels.hip), shared with capi_gpt.hip.
#pragma once
#include "common.h"

enum { PREC_F32 = 0, PREC_BF16 = 1,
       PREC_F32X3 = 2 };   // f32 activations; GEMMs on the bf16 matrix pipe with every f32 operand carried exactly as three bf16 planes
                           // (gpt_kernels.hip::gemm_x3_kernel).  Everything that is not a GEMM runs its f32 code.

// ---- LayerNorm with fused split-K reduce / bias / residual update ---------------------------------------------
struct LnArgs {
    float* x;                // [rows_in][D] residual stream (updated in place when partial/bias_prev given)
    const float* partial;    // [nsplit][rows][D] f32 partial GEMM outputs or null
    int nsplit;
    const float* bias_prev;  // [D] bias of the GEMM whose partials are being reduced, or null
    const float* g1; const float* b1;   // first LayerNorm affine
    const float* g2; const float* b2;   // optional second LayerNorm (ln_f -> final_norm), null to skip
    void* out;               // [rows][D] act dtype (bf16 / f32) or f32 when out_f32 != 0
    int out_f32;
    int rows, D;
    int in_row_mul, in_row_add;   // input row of output row r = r*mul + add (gather of last rows); 1,0 = identity
    float eps;
};
int launch_ln(const LnArgs& a, int prec, hipStream_t st);

// ---- GEMM  C[M,N] = A[M,K] * W[K,N]  on MFMA ------------------------------------------------------------------
enum { EPI_STORE_F32 = 0, EPI_GELU_ACT = 1, EPI_PARTIAL = 2, EPI_RESIDUAL = 3, EPI_QKV = 4,
       // bf16 prefill-tile kernel only (the s2mel DiT, gpt_kernels.hip::pf_epilogue_pair / pf_epilogue):
       EPI_SWIGLU = 5,      // W packed with n-tiles interleaved (2j: w1 columns 16j.., 2j+1: w3 columns 16j..): out_act[m][n] = silu(a) * b
       EPI_GATE = 6,        // same interleave of the WaveNet in_layer halves: out_act[m][n] = tanh(a + bias + g) * sigmoid(b + bias' + g')
       EPI_QKV_ROPE = 7,    // fused wqkv: RoPE on q / k, Q -> out_act [m][D], K -> kcache [seq][H][Tmax][64], V^T -> vcache [seq][H][64][Tmax]
       EPI_WN_RS = 8,       // WaveNet res_skip: n < D: out_f32[m][n] = (out_f32[m][n] + v) * mask(m); n >= D: out2[m][n - D] (=|+=) v
       // f32x3 tile kernel only (gemm_x3.hip):
       EPI_RESIDUAL_SRC = 9 };   // out-of-place residual: out_f32[m][n] = res_src[res_map ? res_map[m] : m][n] + v (res_src rows of ldo floats, != out_f32)
struct GemmArgs {
    const void* A; int lda;          // act dtype [M][lda]
    const void* Wp;                  // packed weights (itts_pack_gemm_weight)
    const float* bias;               // [N] or null
    int M, N, K;
    int nsplit;                      // K slices (EPI_PARTIAL), else 1
    int epi;
    float* out_f32; int ldo;         // EPI_STORE_F32 / EPI_RESIDUAL (in-place add)
    void* out_act;                   // EPI_GELU_ACT: act dtype [M][ldo]
    float* partial;                  // EPI_PARTIAL: [nsplit][M][N]
    // EPI_QKV: n < D -> qbuf[m][n]; D <= n < 2D -> K cache; else V cache, at cache position *pos_ptr + (m % S) [- pos_shift[cache row]]
    float* qbuf; void* kcache; void* vcache;
    const int* pos_ptr; int S, H, Tmax, D;
    const int* pos_shift;            // [cache rows] or null: the batch's position counter runs ahead of cache row r's OWN position by pos_shift[r] -- a
                                     // row admitted into a running batch (itts_gpt_admit_rows) keeps its keys at its own positions; honoured by the decode
                                     // AND the S > 1 tile epilogues (the latent session appends many positions per row at ragged prefix lengths)
    size_t a_planes;                 // f32x3 tile GEMM: when non-zero, A is THREE bf16 planes (plane p at (u16*)A + p * a_planes, rows of lda elements, each
                                     // 32-column group stored in fragment order: ada_rmsnorm_planes_kernel) instead of f32 rows -- no in-register split
    int kb_slice;                    // filled by the decode-GEMM launcher: 32-wide k-blocks per K slice
    int dma_rot;                     // per-block rotation of the slab DMA issue order (ITTS_DECODE_ROT=0 turns it off: A/B switch)
    // LayerNorm fused into a decode GEMM's operand staging (gemm_decode_ln_kernel: at most 4 rows, K == model_dim, bf16): when ln_x is set the
    // A operand is LayerNorm(ln_x [+ the 4 split-K partials ln_partial + ln_bias_prev]) computed by every block (one wave per row, ln_kernel's
    // arithmetic) straight into the LDS slab; block 0 also stores the updated residual rows to ln_x_out (a DIFFERENT buffer: the other
    // blocks still read ln_x).  A / lda are unused then.
    const float* ln_x; float* ln_x_out; const float* ln_partial; const float* ln_bias_prev; const float* ln_g; const float* ln_b; float ln_eps;
    // s2mel epilogues (packed token rows): sequence / frame of a row, valid frames per sequence, RoPE table [t][32][2],
    // per-step conditioning vector (EPI_GATE), second f32 output (EPI_WN_RS) with its overwrite / last-layer switches
    const int* tok_seq; const int* tok_t; const int* seq_len; const float* rope; const float* gvec;
    float* out2; int wn_first, wn_last;
    // tap mode of the bf16 tile kernel (conv_taps > 0): the A operand is an IMPLICIT im2col of a [n_tok][conv_W] matrix -- K
    // index j * conv_W + c reads row src(m, j) = the frame t + j * conv_dil - left of m's sequence, reflect-padded at the
    // sequence ends (SConv1d, encodec.py:212-228); a source outside the sequence (zero extension of very short inputs) reads
    // `zero_row`.  K = conv_taps * conv_W, lda = conv_W.
    int conv_taps, conv_dil, conv_W;
    const int* seq_start; const int* seq_T; const void* zero_row;
    void* out_act2;                  // EPI_WN_RS / EPI_STORE_F32 / EPI_RESIDUAL (bf16 tile kernels): bf16 shadow copy [M][ldo] of the f32
                                     // output (the next GEMM's A operand; for EPI_WN_RS the next layer's tap-mode operand, stride D)
    int seq_mul;                     // EPI_QKV: cache row of sequence b is b * seq_mul (0/1 = identity); beam prefill writes only row b*nb
    const int* seq_map;              // EPI_QKV (decode): when non-null, the cache row of dense row b is seq_map[b] (row compaction of a
                                     // ragged batch: finished rows leave the running batch, the survivors keep their cache rows)
    size_t kv_planes;                // EPI_QKV_ROPE, f32 / f32x3 kernels: when non-zero, K and V^T are written as THREE bf16 planes (h, m, l with
                                     // h + m + l == the f32 value exactly; plane p at element offset p * kv_planes of kcache / vcache, each plane in
                                     // the bf16 mode's image) -- the operands of flash_attn_x3_kernel (s2mel_kernels.hip)
    const float* res_src;            // EPI_RESIDUAL_SRC: the residual's source matrix (rows of ldo floats; must not overlap out_f32) ...
    const int* res_map;              // ... and, when non-null, the source row of output row m (a gather of the residual stream inside the epilogue)
};
int launch_gemm(const GemmArgs& a, int prec, bool prefill, hipStream_t st);
int launch_gemm_x3(const GemmArgs& a, hipStream_t st);      // gemm_x3.hip: the fp32x3 tile kernel (its own translation unit, built without SLP vectorisation)
int gemm_x3_occupancy(int* blocks);
bool gemm_decode_ln_ok(int M, int K, int epi);                 // shapes of the LayerNorm-fused decode GEMM (bf16, 1-4 rows)
int launch_gemm_decode_ln(const GemmArgs& a, hipStream_t st);  // A = LayerNorm(ln_x [+ ln_partial + ln_bias_prev]) built inside the kernel
int gemm_tile_occupancy(int prec, int* blocks);      // diagnostics: predicted resident blocks per CU of the 128 x 128 tile kernel

// Which kernel and geometry a GEMM launcher took: written on the host, per thread, just before the launch (itts_gemm_last_path in
// include/indextts_hip.h: the tests assert the path a shape is meant for, so a changed dispatch threshold cannot drop a kernel out of coverage).
// Order == kGemmPathNames in gpt_kernels.hip.
enum GemmPath {
    GP_NONE = -1,
    GP_BF16_TILE128, GP_BF16_TILE128_NOVEC, GP_BF16_TILE256, GP_BF16_TILE256X128, GP_BF16_REG_PREFILL,
    GP_BF16_SLAB_MT1, GP_BF16_SLAB_MT2, GP_BF16_SLAB_MT4_NT1, GP_BF16_SLAB_MT4_NT2, GP_BF16_SLAB_MT4_NT4,
    GP_BF16_REG_DECODE_MT1, GP_BF16_REG_DECODE_MT2, GP_BF16_REG_DECODE_MT4,
    GP_F32_TILE, GP_F32_REG_PREFILL, GP_F32_REG_DECODE_MT1, GP_F32_REG_DECODE_MT2, GP_F32_REG_DECODE_MT4,
    GP_X3_4W_P6, GP_X3_4W_P8, GP_X3_4W_APLANES, GP_X3_8W,
    GP_BF16_LN_DECODE_4W, GP_BF16_LN_DECODE_WIDE_NT2, GP_BF16_LN_DECODE_WIDE_NT4,
    GP_COUNT
};
void gemm_note_path(int path);
int gemm_last_path();
const char* gemm_path_name(int path);             // nullptr outside 0 .. GP_COUNT - 1

// ---- attention over the KV cache ------------------------------------------------------------------------------
struct AttnArgs {
    const float* qbuf;       // [nseq*nq][D]
    const void* kcache; const void* vcache;   // [nseq][H][Tmax][64] cache dtype
    const int* pad;          // [nseq] first valid key (left padding), or null
    const int* row_map;      // [nseq][Tmax] physical row holding position t of sequence b (beam indirection) or null
    const int* row_map_alt;  // second buffer: the map in use is (*step_ptr & 1) ? row_map_alt : row_map
    const int* step_ptr;
    const int* pos_ptr;      // cache index of query 0
    const int* pos_shift;    // [cache rows] or null: query 0 of cache row r sits at *pos_ptr - pos_shift[r] (GemmArgs::pos_shift), in attn_kernel
                             // and in attn_prefill_mfma_kernel
    void* out;               // [nseq*nq][D] act dtype
    int nseq, H, nq, Tmax, D;
    int seq_mul;             // sequence b reads cache row / pad entry b * seq_mul when no row map is given (0/1 = identity)
    const int* seq_map;      // when non-null (compacted decode batch): dense row b reads cache row / pad entry seq_map[b]
};
int launch_attention(const AttnArgs& a, int prec, hipStream_t st);

// Which kernel and geometry launch_attention took: written on the host, per thread, just before the launch (itts_attention_last_path in
// include/indextts_hip.h; the same purpose as GemmPath).  Order == kAttnPathNames in gpt_kernels.hip: attn_kernel by precision, waves per block
// (4 / 8 / 16) and row map, then attn_prefill_mfma_kernel by precision.
enum AttnPath {
    AP_NONE = -1,
    AP_STREAMS_F32_W4, AP_STREAMS_F32_W4_RMAP, AP_STREAMS_F32_W8, AP_STREAMS_F32_W8_RMAP, AP_STREAMS_F32_W16, AP_STREAMS_F32_W16_RMAP,
    AP_STREAMS_BF16_W4, AP_STREAMS_BF16_W4_RMAP, AP_STREAMS_BF16_W8, AP_STREAMS_BF16_W8_RMAP, AP_STREAMS_BF16_W16, AP_STREAMS_BF16_W16_RMAP,
    AP_PREFILL_MFMA_F32, AP_PREFILL_MFMA_BF16,
    AP_COUNT
};
int attention_last_path();
const char* attention_path_name(int path);        // nullptr outside 0 .. AP_COUNT - 1

// ---- alignment export: the decode query's attention over a span of its keys (itts_gpt_set_alignment) ------------------------------
// attn_align_kernel (gpt_kernels.hip), one block per (dense row b, selected head): with pb / first / last exactly as attn_kernel finds them
// (seq_map / seq_mul, pad[pb], *pos_ptr - pos_shift[pb] clamped to Tmax - 1) and s_t = q . K_t / 8 over keys first .. last,
//     out[u][rstep][kidx][j] = exp(s_t - max) / sum_u exp(s_u - max),  t = first + off + j,  j < len,   0 where t > last
// with (off, len) = span[u], u = row_slot ? row_slot[b] : b, rstep = *step_ptr - row_step0[u] (the column this step's sample_kernel stores
// the token in).  Columns len .. text_cap - 1 are never written.  The whole block leaves when finished[u], rstep < 0, rstep >= max_new or
// rstep >= row_limit[u]: that step's token is forced, and a finished row of a long session keeps stepping.
// Reduction order: the maximum is exact (f32 max of f32 scores, every score kept in LDS); e_t = expf(s_t - max) in f32, computed once and
// kept in LDS (the normalising pass and the output pass read the same number); the sum in F64: thread i adds keys i, i + 1024, ... ascending,
// an xor-shuffle tree inside the wave, the sixteen wave partials in index order; p = (float)((double)e_t / sum).  A score depends
// on q and the key's row alone (one fma chain per lane, one shuffle tree), so a row's BITS do not depend on the batch, the dense row,
// compaction, the fused-LayerNorm path or the step at which the row joined.
struct AlignArgs {
    const float* qbuf;       // [nseq][D] the step's queries (the QKV epilogue has just written them)
    const void* kcache;      // [cache rows][H][Tmax][64] cache dtype, the layer's keys
    const int* pad; const int* pos_ptr; const int* pos_shift; const int* seq_map; int seq_mul;   // as AttnArgs
    const int* row_slot;     // [nseq] dense row -> utterance, or null (identity)
    const int* step_ptr;     // the batch's step counter
    const int* row_step0;    // [utterances] or null (0)
    const int* row_limit;    // [utterances] or null
    const unsigned char* finished;   // [utterances] or null
    const int* span;         // [utterances][2] (off, len) relative to `first`
    float* out;              // [utterances][max_new][n_pairs][text_cap]
    int head[8], kidx[8];    // the launch's heads and each one's index in the installed pair list
    int n_heads;             // grid.y
    int nseq, H, Tmax, D, max_new, n_pairs, text_cap;
};
#define ALIGN_MAX_PAIRS 8
#define ALIGN_MAX_TEXT 1024
#define ALIGN_MAX_KEYS 12288          // Tmax whose score row (one f32 per cache position, dynamic LDS) fits in 48 KiB
int launch_attention_align(const AlignArgs& a, int prec, hipStream_t st);

// ---- alignment export of a many-query pass (itts_gpt_rescore) -----------------------------------------------------------------------
// attn_align_mq_kernel (gpt_kernels.hip): attn_align_kernel for the nq consecutive queries a teacher-forced pass appends per sequence.  For
// sequence b, the i-th listed head and query qi < (q_len ? q_len[b] : nq), with pb / first as attn_align_kernel finds them and
// last = min(*pos_ptr + qi - pos_shift[pb], Tmax - 1):
//     out[b][row0 + qi][kidx][j] = softmax_{first..last}(q[b][qi] . K / 8)[first + off + j],  j < min(len, text_cap),  0 where past `last`
// with (off, len) = span[b].  Queries from q_len[b] on write nothing.  Per (query, key) the arithmetic is attn_align_kernel's, operation for
// operation (lane split of the dot, ascending fmaf, xor-shuffle over the key's lanes, * 0.125f, exact f32 max, expf once into LDS, the f64 sum
// per thread ascending keys / xor tree / wave partials in index order, (float)(e / sum)): a query's row has the BITS the single-query kernel
// gives for the same q, cache and window.  New is the reuse: a block serves a tile of `qt` consecutive queries of one (sequence, head), so each
// 16-byte key load feeds every query of the tile.
struct AlignMqArgs {
    const float* qbuf;       // query (b, qi) = qbuf + ((size_t)b * q_stride + qi) * D
    int q_stride;            // rows of qbuf per sequence (>= nq)
    const void* kcache;      // [cache rows][H][Tmax][64] cache dtype, the layer's keys
    const int* pad; const int* pos_ptr; const int* pos_shift; const int* seq_map; int seq_mul;   // as AttnArgs (pos_ptr: cache index of query 0)
    const int* q_len;        // [nseq] valid queries per sequence, or null (nq)
    const int* span;         // [nseq][2] (off, len) relative to `first`
    float* out;              // [nseq][out_rows][n_pairs][text_cap]
    int head[8], kidx[8];
    int n_heads;             // grid.y
    int nseq, nq, row0, out_rows, H, Tmax, D, n_pairs, text_cap;
    int qt;                  // filled by the launcher: queries per block, clamp(ALIGN_MQ_LDS_FLOATS / Tmax, 1, ALIGN_MQ_QT)
};
#define ALIGN_MQ_QT 8                 // queries per block at most: their query registers (8 x 8 dims) fit beside four key loads in flight
#define ALIGN_MQ_LDS_FLOATS 15872     // score rows of a block: 62 KiB, which leaves the reduction scratch inside the 64 KiB a kernel gets unasked
int launch_attention_align_mq(const AlignMqArgs& a, int prec, hipStream_t st);

// ---- log-probability of given tokens under rows of logits (itts_gpt_rescore) -----------------------------------------------------------
// logp_gather_kernel (gpt_kernels.hip), one block of 256 threads per row: out[r] = (float)(((double)row[tok] - max) - log sum_i exp(row[i] - max)),
// tok = targets[r], over the V valid columns of row r of logits [rows][ldl]; 0.0f when tok lies outside 0 .. V - 1 or the row's max is -inf.
// The normaliser is row_logsumexp, i.e. the arithmetic and reduction order of sample_kernel's logp_model (SampleArgs): the same bits for the
// same row.  Never log(e_tok / sum): a token whose expf underflows keeps its finite log-probability.
struct LogpGatherArgs {
    const float* logits; int ldl;
    const long long* targets;   // [rows]
    float* out;                 // [rows]
    int rows, V;
};
int launch_logp_gather(const LogpGatherArgs& a, hipStream_t st);

// ---- code prefix (itts_gpt_set_code_prefix) ---------------------------------------------------------------------------------------------
// prefix_embed_kernel (gpt_kernels.hip), grid (n, nseq): the ragged embed-and-seed pass of one ingest chunk.  Prefix code j = j0 + qi of row b
// (j < lens[b]: live; past it a dead query, embedded as code 0 so that the stack runs on finite numbers):
//     x[b][qi] = mel_emb[codes[b][j]] + mel_pos[min(j + pos_offset, n_mel_pos - 1)]
// and for a live code, with u = slots ? slots[b] : b the row's utterance slot: tokens[u][j] = the code, seen[u][code] = 1, both score arrays'
// entry [u][j] = 0.0 (a prefix code was given, not selected: it is scored like a forced token).  The chunk with j0 == 0 also sets the row's own
// step and position under the shared counters: row_step0[u] = step0 - lens[b], row_shift[u] = shift - lens[b] -- the selection kernel and the
// decode step's QKV epilogue / attention then see own step = step + lens[b] and own position = pos + lens[b] (SampleArgs, AttnArgs.pos_shift):
// the row HAS taken lens[b] steps.
struct PrefixEmbedArgs {
    const long long* codes; int width;      // [nseq][width]
    const int* lens;                        // [nseq] device
    const int* slots;                       // [nseq] row -> utterance slot, or null (identity)
    int j0, n, nseq, pos_offset, V, n_mel_pos, D;
    const float* mel_emb; const float* mel_pos;
    float* x;                               // [nseq][n][D]
    long long* tokens; int max_new;         // [utterances][max_new]
    unsigned char* seen;                    // [utterances][V]
    int* row_step0; int* row_shift;         // [utterances]
    int step0, shift;                       // what a row without a prefix gets (0, 0 on a first call; the admission's values)
    float* logp_model; float* logp_sampled; // [utterances][max_new] or null
};
int launch_prefix_embed(const PrefixEmbedArgs& a, hipStream_t st);
// prefix_gather_kernel, grid nseq: the last-query gather.  Row b's last valid query of this chunk's x [nseq][n][D] -- q = lens[b] - 1 - j0 when
// 0 <= q < n, or q = force_q for every row when force_q >= 0 (the prompt's last position) -- is copied to out[b]; other rows keep what they hold.
struct PrefixGatherArgs {
    const float* x; int n, j0, force_q, nseq, D;
    const int* lens;                        // [nseq] device (unused with force_q >= 0)
    float* out;                             // [nseq][D]
};
int launch_prefix_gather(const PrefixGatherArgs& a, hipStream_t st);

// ---- token selection ------------------------------------------------------------------------------------------
// One utterance slot's sampling settings: the device image of itts_row_sampling (include/indextts_hip.h; layout asserted in capi_gpt.hip)
struct RowSampling {
    int do_sample, top_k, min_keep;
    float top_p, temperature, rep_penalty, typical_mass;
    int stream;
    unsigned long long seed;
};
// The installed logits filters (itts_gpt_set_logits_filters): ONE device record per engine handle, at an address that never changes.  The
// selection kernels take its address (null: nothing installed) and load the record at entry, so a captured step graph bakes in nothing of
// its contents -- another min_new_tokens replays the same graph.  `mask` / `decay` are handle-owned device buffers.
// The same record is the element of the per-slot table (itts_gpt_set_row_filters; SampleArgs::filt_table / BeamArgs::filt_table).
struct LogitsFilters {
    int min_new_tokens, min_length;   // 0 = off: the stop token is -inf while own step < min_new_tokens / prompt length + own step < min_length
    int ngram;                        // 0 = off: no_repeat_ngram_size (num_beams = 1)
    int decay_start;                  // exponential_decay_length_penalty[0]; -1 = off
    int n_decay;                      // entries of `decay`
    int has_mask;                     // any bit set in `mask`
    int prompt_len;                   // S of the running call (written by the generate entries; a session row's own prompt length is
                                      // prompt_len + row_step0 - row_shift)
    int start_mel;                    // last id of the fake prompt HF sees: [1] * (S - 1) + [start_mel]
    float min_p;                      // < 0 = off
    float epsilon, eta;               // 0 = off
    const unsigned char* mask;        // [V] bit 0: -inf always (suppress_tokens, single-token bad words); bit 1: -inf at own step 0 (begin_suppress_tokens)
    const float* decay;               // [n_decay] f32(factor^(step - decay_start) - 1) by own step, 0 up to decay_start
};
struct SampleArgs {
    const float* logits;     // [B][V]
    unsigned char* seen;     // [B][V] ids already in input_ids (repetition penalty set)
    unsigned char* finished; // [B]
    long long* tokens;       // [B][max_new]
    const int* step_ptr;     // generated-token index of this step
    const double* uniforms;  // [max_new][B] or null (then an internal counter RNG with `seed` is used)
    unsigned long long seed;
    int B, V, max_new;
    int do_sample, top_k, min_keep;
    float top_p, temperature, rep_penalty;
    float typical_mass;      // 0 = off, else TypicalLogitsWarper(mass) between the repetition penalty and the warpers
    int stop_token;
    // next-step embedding: x_next[b] = mel_emb[tok] + mel_pos[step + pos_offset]
    const float* mel_emb; const float* mel_pos; float* x_next; int D; int pos_offset; int n_mel_pos;
    int* adv_state;          // {step, pos, ticket}: when non-null the last block to finish advances step and pos (decode steps)
    const unsigned long long* seed_ptr;   // when non-null the RNG seed is read from device memory (keeps a captured step seed-free)
    // compacted decode batch: dense row b is utterance row_slot[b] -- its seen-set, finished flag, token row, uniform / RNG stream and
    // token limit are indexed by the utterance, logits and x_next by the dense row.  uniforms_stride = utterances of the call.
    const int* row_slot; int uniforms_stride;
    int radix_select;        // filled by the launcher (ITTS_SAMPLE_RADIX=1): the 4-pass radix-select top-k instead of the ballot bisection (A/B switch)
    unsigned long long* stamps;   // microbench builds only (-DITTS_SAMPLE_STAMPS): [B][8] phase time stamps, else null
    const int* row_limit;    // [utterances] or null: per-utterance cap on generated tokens (a batch merges requests with their own
                             // max_mel_tokens): from token index row_limit[u] on, the row emits the stop token
    const int* row_step0;    // [utterances] or null: the step at which utterance u joined the running batch (itts_gpt_admit_rows; 0 for the rows of
                             // the first call).  The row's own step (step - row_step0[u]) indexes its token column, its mel position embedding,
                             // its uniform / RNG stream and its token limit -- what the row would see decoded alone; from its own step max_new
                             // on a row emits the stop token and stores nothing (a session's step counter may run past max_new).
    const RowSampling* row_table;   // [utterances] or null: per-slot sampling settings (itts_gpt_set_row_sampling).  When set, entry u replaces the
                             // scalars do_sample / top_k / min_keep / top_p / temperature / rep_penalty / typical_mass above and the RNG draw is
                             // rng_uniform(entry.seed, row step, entry.stream) -- `stream` where the scalar path keys the slot index u, `seed`
                             // instead of *seed_ptr; `uniforms`, when given, still replace the RNG.  The seen set and the finished flag are kept
                             // whatever the penalty is, so nothing else depends on the scalars.
    const LogitsFilters* filt;      // null: no filter installed (the kernel then computes what it always did)
    const int* row_shift;           // [utterances] as BeamArgs::row_shift; read with `filt` only (a session row's own prompt length)
    const LogitsFilters* filt_table;   // [utterances] or null: per-slot filter records (itts_gpt_set_row_filters).  When set, the row loads entry u -- the index
                             // of row_table -- instead of *filt; each entry's mask / decay point into the slot's own rows of handle-owned arrays.  An
                             // "off" entry (counts 0, decay_start -1, min_p -1, epsilon = eta = 0, has_mask 0) makes filter_score, ngram_ban and
                             // filter_warp_lo identities: the row gets the bits of the unfiltered branch.
    // Token scores (itts_gpt_set_token_scores), both set or both null; [utterances][max_new] f32 laid out like `tokens` (row u, column = the
    // row's own step).  Set: the launcher takes the sample_kernel<true> instantiation, which writes next to the token it stores
    // log_softmax(raw logits row)[tok] (logp_model) and the log-probability the token was selected with (logp_sampled), 0.0f in both for a
    // forced token.  Accumulation: f32 max, f32 exponentials summed in F64 in one fixed order (per thread ascending i, xor-shuffle tree, the
    // four wave partials in index order by one thread), f64 log, one rounding to f32: batch-invariant bits.  Null: the kernel as it always was.
    float* logp_model; float* logp_sampled;
};
int launch_sample(const SampleArgs& a, hipStream_t st);
int launch_advance(int* step_ptr, int* pos_ptr, hipStream_t st);

// ---- beam search / beam-sample step (GenerationMixin._beam_search + BeamSearchScorer.process) ------------------
#define BEAM_MAX 4
struct BeamHyp { float score; int step; int row; int pad; };
// One beam group's sampling settings: the device image of itts_group_sampling (include/indextts_hip.h; layout asserted in capi_gpt.hip)
struct GroupSampling {
    int do_sample, top_k, min_keep;
    float top_p, temperature, rep_penalty, typical_mass, length_penalty;
    int stream;
    unsigned long long seed;
};
struct BeamArgs {
    const float* logits;          // [B*nb][V]
    unsigned char* seen[2];       // [B*nb][V], parity = step & 1 (read), 1 - parity (written by apply)
    int* row_map[2];              // [B*nb][Tmax]
    float* beam_scores;           // [B*nb]
    float* next_scores; int* next_tokens; int* next_indices;   // [B*nb]
    int* surv_idx; float* surv_val; int* surv_n;                // [B*nb][64], [B*nb]: per-row survivors (phase 1 -> phase 2)
    BeamHyp* hyps;                // [B][BEAM_MAX]
    int* n_hyps;                  // [B]
    float* worst;                 // [B]
    unsigned char* done;          // [B]
    int* hist_tok; int* hist_par; // [max_new][B*nb]
    const int* step_ptr;
    int logits_shared;            // 1: logits hold ONE row per utterance (first step after the shared-prompt prefill)
    const double* uniforms;       // [max_new][B][2*nb] or null
    unsigned long long seed;
    int B, nb, V, max_new, Tmax, S;
    int do_sample, top_k, min_keep;
    float top_p, temperature, rep_penalty, length_penalty;
    float typical_mass;
    int stop_token;
    const float* mel_emb; const float* mel_pos; float* x_next; int D; int pos_offset; int n_mel_pos;
    int* adv_state;               // as SampleArgs::adv_state, honoured by the apply kernel (the step's last launch)
    const unsigned long long* seed_ptr;   // as SampleArgs::seed_ptr
    int radix_select;             // as SampleArgs::radix_select (filled by the launcher)
    // Beam sessions (itts_gpt_generate_beam_chunk / itts_gpt_admit_beam_groups): a group = the nb adjacent rows of one utterance.  All null / 0 =
    // one batch decoded from step 0 (itts_gpt_generate_beam: the code below then computes what it always did).
    const int* row_step0;         // [B*nb] the session step of the group's own step 0 (entry b*nb is read): own step = *step_ptr - row_step0[b*nb] indexes the
                                  // history row, gen_len / length penalty, the hypothesis' step, the mel position, the cap and the uniform / RNG stream
    const int* row_shift;         // [B*nb] position counter - the row's own position (GemmArgs::pos_shift): the row-map extent follows the own position
    const int* grp_cap;           // [B] cap on the group's own steps: from own step cap on the search is frozen as at max_length (scores, hypotheses and
                                  // history keep their values; the rows emit the stop token inside their own cache rows)
    const int* grp_map;           // [n_grp] launch over a subset of the groups: block g works on group grp_map[g] (the first step of admitted groups);
                                  // with logits_shared the logits row is g
    int n_grp;                    // groups launched (0: all B)
    const GroupSampling* grp_table;   // [B] or null: per-group sampling settings (itts_gpt_set_group_sampling).  When set, entry b (the group, grp_map[g] in a
                                  // subset launch) replaces the scalars do_sample / top_k / min_keep / top_p / temperature / rep_penalty / typical_mass /
                                  // length_penalty above -- loaded once at the top of beam_rows_kernel / beam_step_kernel, so every branch on them is
                                  // block-uniform -- and the draw is rng_uniform(entry.seed, own step * 8 + d, entry.stream): `stream` where the scalar
                                  // path keys the group's slot b, `seed` instead of *seed_ptr; `uniforms`, when given, still replace the RNG.  The entry
                                  // is read EVERY step (the host rewrites a finished group's entry before it admits a new utterance there).
    const LogitsFilters* filt;    // as SampleArgs::filt (the n-gram filter is not applied here: a beam's history is not kept per row)
    const LogitsFilters* filt_table;   // [B] or null: as SampleArgs::filt_table, one record per beam group (entry b, the group after grp_map)
};
int launch_beam_step(const BeamArgs& a, hipStream_t st);
int launch_beam_apply(const BeamArgs& a, hipStream_t st);
