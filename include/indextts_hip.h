/* indextts_hip.h -- C ABI of the MI355X (gfx950) IndexTTS hot-path engine.
 *
 * The reference (index-tts/index-tts) has no FFI for this path: the replaceable seams are Python call sites
 * (SURVEY.md section 8b).  Each entry point below names the reference call it stands in for.  All device
 * pointers are raw HIP device addresses owned by the caller (PyTorch's allocator in the shipped host code);
 * the library never frees or retains them past the call, except the weights it copies at load time.
 * Every function returns 0 on success or an ITTS_ERR_* code; itts_last_error() gives the message.
 * Nothing throws across this boundary.  `stream` is a hipStream_t passed as void*.
 * Devices: a model handle belongs to the HIP device that was current when its *_create ran (the analogue of
 * `module.to(device)` in the reference, indextts/infer_v2_5.py:146,232); every call taking the handle switches to that
 * device for its duration and rejects tensors that live on another one.
 */
#ifndef INDEXTTS_HIP_H
#define INDEXTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ITTS_ABI_VERSION 13

int itts_abi_version(void);
const char* itts_last_error(void);
/* number of HIP devices visible, or <0 with the HIP error recorded (the library itself loads without a GPU) */
int itts_device_count(void);

/* ------------------------------------------------------------------------------------------------------------
 * Run-time options.  The library reads NO environment variable; every switch between kernels that tests hold to the same
 * results (most of them bitwise) is a named integer option, process-wide, read by the launchers at launch time.  The defaults
 * are the measured-best paths.  Changing a value retires the decode hipGraphs cached in GPT handles (they bake kernel choices
 * in); options marked "at create" are sampled when a model handle is created.  The reference has no counterpart (its kernels are
 * picked by PyTorch's dispatcher); the table exists for A/B tests and measurement tools.
 *   name              default  range    meaning
 *   decode_fuse_ln       1     0..2    GPT decode: LayerNorm inside the consuming GEMM, 1: at 1-8 rows, 2: up to 16 rows, 0: ln_kernel launches
 *   decode_gemm          1     0..1    bf16 decode GEMMs on the LDS-DMA slab kernel (0: register-path kernel)
 *   decode_rot           1     0..1    per-block rotation of the slab DMA issue order
 *   decode_wnt           0     0..1    non-temporal policy on the decode weight stream
 *   decode_nt            0     0..4    force the n-tiles per block of the 64-row decode GEMM
 *   prefill_gemm         1     0..1    bf16 prefill GEMMs on the LDS-DMA tile kernels (0: register-path kernel)
 *   tile256             -1    -1..2    bf16 tile GEMM: -1 by shape, 0 128x128, 1 256x256, 2 256x128
 *   f32_tile             1     0..1    f32 GEMMs with plain epilogues on the f32-MFMA tile kernel
 *   x3_products          6     6..8    plane products per f32 product of the fp32x3 GEMMs / attention (6 or 8)
 *   x3_sched             1     0..1    fp32x3 GEMM: operand split interleaved with the MFMAs
 *   x3_attn              1     0..1    fp32x3 s2mel: attention products on bf16 planes as well (0: the f32-MFMA flash kernel)
 *   sample_radix        -1    -1..1    top-k threshold: -1 per-kernel default, 0 ballot bisection, 1 radix select
 *   gpt_compact          1     0..1    row compaction of ragged decode batches
 *   attn_waves           0     0..16   waves per block of the KV-cache attention kernel (0: by shape; 4 / 8 / 16)
 *   s2mel_fused          1     0..2    s2mel: fused GEMM epilogues (at create); 1: fused, 0: separate element-wise kernels (2 = 1, round 4's spelling)
 *   fa_qs                0     0..4    bf16 flash attention: query sub-tiles per wave (0: by shape)
 *   f32_attn_scalar      0     0..1    f32 s2mel attention on the one-wave-per-query reference kernel
 *   fa32_qs              2     1..2    f32 flash attention: query sub-tiles per wave
 *   aa_act               2     0..2    anti-aliased activation kernel variant
 *   conv_bm              0     0..128  force the co-tile height of the vocoder conv kernel
 *   h3_kernel            1     0..1    f16x3 vocoder conv: window kernel / two-stage kernel
 *   decode_ln_nt         2     2..4    LayerNorm-fused decode GEMM at 5-16 rows: n-tiles per block (2 or 4)
 *   x3_aplanes           0     0..1    fp32x3 s2mel: adaptive-norm outputs as bf16 planes, wqkv / w1|w3 GEMMs without an operand split
 *   x3_pin               0     0..1    fp32x3 GEMM: 1 = non-default variants on one block per CU (round 4's workaround, diagnostic only)
 *   prefill_attn        -1    -1..1    GPT attention of S > 1 passes: -1 causal MFMA kernel (bf16 mode) / canonical streams (f32 mode), 0 canonical, 1 MFMA
 *   voc_act_planes       1     0..1    vocoder bf16x3 mode: activation writes the x3 conv's operand planes (0: f32 activation + split pass; same bits)
 *   x3_waves             8     4..8    fp32x3 GEMM: waves per 128 x 128 block, 8 (wave tile 32 x 64, weights through LDS) or 4 (64 x 64, round 5's kernel); same bits
 *   s2mel_prune_last     1     0..1    fp32x3 s2mel solve with a tail layout: last DiT layer's attention queries + post-attention stages on the tail rows only, x_in residual read from const_in (no copy); same bits
 *   x3_attn_skip         1     0..1    fp32x3 flash attention: skip the fully masked half of a last key tile and the compute of waves without a valid query; same bits
 * itts_option_count / _name / _doc / _default enumerate the table (index 0 .. count-1).
 * ---------------------------------------------------------------------------------------------------------- */
int itts_set_option(const char* name, int value);      /* ITTS_ERR_ARG: unknown name or value out of range */
int itts_get_option(const char* name, int* value);
int itts_reset_options(void);                          /* every option back to its default */
int itts_option_count(void);
const char* itts_option_name(int index);
const char* itts_option_doc(int index);
int itts_option_default(int index);

/* ------------------------------------------------------------------------------------------------------------
 * BigVGAN vocoder
 * ---------------------------------------------------------------------------------------------------------- */

/* replaces: anti_alias_activation_cuda.forward(input, up_ftr, down_ftr, alpha, beta)
 *   indextts/s2mel/modules/bigvgan/alias_free_activation/cuda/anti_alias_activation.cpp:19-23 (fwd_cuda,
 *   anti_alias_activation_cuda.cu:212) and the torch Activation1d it shadows (.../torch/act.py:25-30).
 * x, y: [B][C][T] f32; alpha, beta: [C] (log scale iff logscale != 0); up_filter, down_filter: [12].
 * lens: optional [B] int32 row lengths (in units of T / len_mult); rows are bounded at their own length. */
int itts_aa_act_forward(const float* x, float* y, const float* alpha, const float* beta, const float* up_filter,
                        const float* down_filter, int B, int C, int T, const int32_t* lens, int len_mult,
                        int logscale, void* stream);

/* host-side weight packing into MFMA A-fragment order (pure CPU; no device needed).
 * conv1d: w [Cout][Cin][k] -> out[itts_packed_conv_floats(Cout, Cin, k)]
 * convT : w [Cin][Cout][k] (torch ConvTranspose1d layout), stride u, padding (k-u)/2: phase r in [0,u) -> a (k/u)-tap
 *         conv, out as above with k/u taps (requires k a multiple of u and k-u even: 8/4, 4/2 in BigVGAN-v2, also 4/4
 *         as in the IndexTTS-1.5 vocoder config). */
size_t itts_packed_conv_floats(int Cout, int Cin, int k);
int itts_pack_conv1d_weight(const float* w, int Cout, int Cin, int k, float* out);
int itts_pack_convT_weight(const float* w, int Cin, int Cout, int k, int u, int phase, float* out);

/* replaces: torch.nn.Conv1d forward inside AMPBlock1 / conv_pre (bigvgan.py:132-141,362), "same" padding.
 * y = epi(conv(x) + bias + bias_b[b] + res), epi by acc_mode: 0 store, 1 y += v, 2 y = (y + v) / div. */
int itts_conv1d_forward(const float* x, const float* wpk, const float* bias, const float* bias_b, const float* res,
                        float* y, int B, int Cin, int Cout, int T, int k, int dilation, const int32_t* lens,
                        int len_mult, int acc_mode, float div, void* stream);

/* Opt-in second mode of the resblock Conv1d's (same arithmetic contract as itts_conv1d_forward, `same` zero padding, odd k):
 * the f32 operands are split into two f16 parts each (x = xh + 2^-11 xl, 22 significand bits) and the conv runs as three
 * v_mfma_f32_16x16x32_f16 products per fragment pair with exact f32 accumulation (the xl*wl term, 2^-22 relative, is dropped).
 * C_in % 32 == 0.  wp3 = itts_pack_conv1d_h3_weight output on the device; scratch = itts_conv1d_h3_scratch_bytes device bytes.
 * replaces: the same nn.Conv1d calls of AMPBlock1 (bigvgan.py:96-141) as itts_conv1d_forward. */
size_t itts_conv1d_h3_packed_bytes(int Cout, int Cin, int k);
int itts_pack_conv1d_h3_weight(const float* w, int Cout, int Cin, int k, void* out);        /* host -> host */
size_t itts_conv1d_h3_scratch_bytes(int B, int Cin, int T);
int itts_conv1d_h3_forward(const float* x, const void* wp3, const float* bias, const float* res, float* y, int B, int Cin, int Cout,
                           int T, int k, int dilation, const int32_t* lens, int len_mult, int acc_mode, float div, void* scratch,
                           void* stream);

/* Third mode of the resblock Conv1d's, the one that may carry the benchmark: every f32 operand EXACTLY as three bf16 planes (x = xh + xm + xl, 8 + 8 +
 * 8 significand bits), six v_mfma_f32_16x16x32_bf16 plane products per fragment pair (the three dropped ones are <= 2^-24 |x w| each), exact f32
 * accumulation -- the arithmetic of the flow-matching stage's fp32x3 GEMMs; error against an f64 convolution not above the f32-MFMA kernel's.
 * C_in % 32 == 0, odd k >= 3, (k - 1) * dilation <= 64.  wp3 = itts_pack_conv1d_x3_weight output on the device; scratch =
 * itts_conv1d_x3_scratch_bytes device bytes.
 * replaces: the same nn.Conv1d calls of AMPBlock1 (bigvgan.py:96-141) as itts_conv1d_forward. */
size_t itts_conv1d_x3_packed_bytes(int Cout, int Cin, int k);
int itts_pack_conv1d_x3_weight(const float* w, int Cout, int Cin, int k, void* out);        /* host -> host */
size_t itts_conv1d_x3_scratch_bytes(int B, int Cin, int T);
int itts_conv1d_x3_forward(const float* x, const void* wp3, const float* bias, const float* res, float* y, int B, int Cin, int Cout,
                           int T, int k, int dilation, const int32_t* lens, int len_mult, int acc_mode, float div, void* scratch,
                           void* stream);
/* replaces: torch.nn.ConvTranspose1d forward of the upsamplers (bigvgan.py:300-316,366-367); k == 2*u,
 * padding (k-u)/2.  wpk_phases: u packed 2-tap weights back to back (itts_pack_convT_weight, phase 0..u-1). */
int itts_conv_transpose1d_forward(const float* x, const float* wpk_phases, const float* bias, const float* bias_b,
                                  float* y, int B, int Cin, int Cout, int Tin, int k, int u, const int32_t* lens,
                                  int len_mult_in, void* stream);

/* Vocoder launch paths and two unit ops for the tests (v13, additive: vocoder path names).
 * Every vocoder conv / activation launcher records, on the host and per calling thread, the kernel and geometry it is about to launch (as the
 * GEMM and attention launchers do; the u phase launches of a transposed conv report the f32 conv kernel they run on).  itts_voc_last_path: the
 * name of the calling thread's last one ("none" before the first); itts_voc_path_count / itts_voc_path_name(0 .. count - 1): every name (NULL
 * outside the range).  Names: conv_f32_bm32 / _bm64 / _bm96 / _bm128 (conv_mfma_kernel by co-tile height, option conv_bm), conv_x3_nh1 / _nh2
 * (bf16 x 3 window kernel, one / two co tiles per window), conv_h3_two_stage, conv_h3_win256x128 / _win192x192 / _win256x96 (f16 x 3 kernels,
 * option h3_kernel and the padded-width rule), aa_v1_sinf, aa_v2_sinf, aa_v2_vsin (option aa_act 0 / 1 / 2), aa_planes_vsin.  Launches
 * replayed from a captured graph record nothing.
 * itts_aa_act_planes_forward: itts_aa_act_forward written straight into the bf16 x 3 conv's operand (what the generator launches in front of
 *   an x3 conv under option voc_act_planes; replaces the same Activation1d call, act.py:25-30): planes [3][B][T][C] bf16 (h, m, l with
 *   h + m + l == the f32 activation of aa_act = 2 exactly), frames beyond a row's length zeros.  C % 8 == 0.
 * itts_sin_reduced_forward: y[i] = the sine the default activation kernels evaluate (two-term Cody-Waite reduction by 2 pi, then the hardware
 *   v_sin_f32), elementwise over n f32 values on the device -- the probe that measures that sine against an f64 sine on its own (replaces
 *   the sin of SnakeBeta.forward, indextts/s2mel/modules/bigvgan/activations.py:118). */
const char* itts_voc_last_path(void);
int itts_voc_path_count(void);
const char* itts_voc_path_name(int index);
int itts_aa_act_planes_forward(const float* x, void* planes, const float* alpha, const float* beta, const float* up_filter,
                               const float* down_filter, int B, int C, int T, const int32_t* lens, int len_mult, int logscale,
                               void* stream);
int itts_sin_reduced_forward(const float* x, float* y, size_t n, void* stream);

typedef struct {
    int32_t in_channels;               /* num_mels (v2: 80) or gpt latent dim (v1) */
    int32_t upsample_initial_channel;
    int32_t num_upsamples;
    int32_t upsample_rates[8];
    int32_t upsample_kernel_sizes[8];
    int32_t num_kernels;
    int32_t resblock_kernel_sizes[4];
    int32_t num_dilations;
    int32_t resblock_dilations[4][4];
    int32_t snake_logscale;
    int32_t activation;                /* 0 snakebeta, 1 snake */
    int32_t use_tanh_at_final;         /* v2: 0 (clamp), v1: 1 */
    int32_t use_bias_at_final;
    int32_t cond_dim;                  /* 0 = v2 (no conditioning); >0 = v1 speaker embedding width */
    int32_t cond_in_each_up_layer;
} itts_bigvgan_config;

typedef struct itts_bigvgan itts_bigvgan;

/* replaces: BigVGAN.__init__ + from_pretrained/load_state_dict + remove_weight_norm
 *   (indextts/s2mel/modules/bigvgan/bigvgan.py:266-358,388-492; v1 indextts/BigVGAN/models.py).
 * Tensors are given by their reference state-dict names (weight-norm already folded), host f32 pointers. */
int itts_bigvgan_create(const itts_bigvgan_config* cfg, itts_bigvgan** out);
int itts_bigvgan_device(const itts_bigvgan* h);   /* Conv mode of the generator's resblock convs, to be chosen BEFORE the weights are loaded: 0 = exact f32 MFMA (default; the parity
 * mode), 1 = f16 x 3 split operands (itts_conv1d_h3_forward), 2 = bf16 x 3 plane operands (itts_conv1d_x3_forward; exact operands, the mode
 * the benchmark runs) for the resblocks with >= min_channels channels (0 = default 96);
 * everything else (conv_pre / upsamplers / conv_post / activations) is unchanged. */
int itts_bigvgan_set_conv_mode(itts_bigvgan* h, int mode, int min_channels);
/* f16 x 3 mode only: 1 if a forward since the last call met an activation that is not finite or not below 65504 in magnitude (that
 * forward's output is invalid -- use mode 0), else 0; synchronises the device and clears the flag; < 0 on error. */
int itts_bigvgan_range_check(itts_bigvgan* h);
/* device index the handle is bound to */
int itts_bigvgan_load_tensor(itts_bigvgan* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int itts_bigvgan_finalize(itts_bigvgan* h);       /* checks every required tensor arrived */
void itts_bigvgan_destroy(itts_bigvgan* h);
size_t itts_bigvgan_workspace_bytes(const itts_bigvgan* h, int B, int T);

/* replaces: BigVGAN.forward(mel) (bigvgan.py:360-386; call site indextts/infer_v2_5.py:850) and the v1
 *   BigVGAN.forward(latent, mel_ref) generator part (indextts/BigVGAN/models.py:216-250; infer.py:647) with the
 *   speaker embedding passed in (spk [B][cond_dim], or NULL for v2).
 * x [B][in_channels][T] f32; lens optional [B] int32 (frames); wav [B][T*prod(upsample_rates)] f32. */
int itts_bigvgan_forward(itts_bigvgan* h, const float* x, const int32_t* lens, const float* spk, float* wav, int B,
                         int T, void* workspace, size_t workspace_bytes, void* stream);

/* replaces: the vocoder stage of the reference's streaming pipeline (backends/trt/pipeline/streaming.py:57-68,140-172:
 *   overlapping chunks re-synthesised and Hann-crossfaded) by an exact overlap-save stream: one utterance, mel frames
 *   [in_channels][n_frames] (row stride ld_mel floats, device) pushed in chunks of at most chunk_frames; each push writes
 *   the samples that became final to wav_out (capacity (chunk_frames + halo_frames) * prod(upsample_rates) floats) and
 *   their count to *n_samples_out.  Output trails the input by halo_frames until the push with is_last != 0.  The
 *   concatenation equals itts_bigvgan_forward over the whole mel when halo_frames covers the receptive field (43 frames
 *   for the 22 kHz v2 generator).  spk: v1 speaker embedding [cond_dim] or NULL. */
typedef struct itts_bigvgan_stream itts_bigvgan_stream;
int itts_bigvgan_stream_open(itts_bigvgan* h, int chunk_frames, int halo_frames, itts_bigvgan_stream** out);
size_t itts_bigvgan_stream_workspace_bytes(const itts_bigvgan_stream* s);
int itts_bigvgan_stream_push(itts_bigvgan_stream* s, const float* mel, int ld_mel, int n_frames, int is_last,
                             const float* spk, float* wav_out, int32_t* n_samples_out, void* workspace,
                             size_t workspace_bytes, void* stream);
void itts_bigvgan_stream_close(itts_bigvgan_stream* s);

/* measurement hooks (no reference counterpart: the reference only has unsynchronised perf_counter stage timers,
 *   indextts/infer_v2_5.py:744-746,871-876).  With profiling enabled every kernel launch of the forward is bracketed
 *   by HIP events on the launch stream; profile_read returns, for the LAST forward and per kernel class
 *   {0: Conv1d MFMA, 1: ConvTranspose1d MFMA, 2: anti-aliased activation, 3: conv_post}, the summed GPU ms, launch
 *   count, algorithmic FLOPs and algorithmic tensor bytes (arrays of 4 doubles). */
int itts_bigvgan_set_profiling(itts_bigvgan* h, int enable);
int itts_bigvgan_profile_read(itts_bigvgan* h, double* ms, double* launches, double* flops, double* bytes);
/* per-launch records of the last forward, launch order: out[4*i..] = {class, ms, flops, bytes}; returns the count */
int itts_bigvgan_profile_records(itts_bigvgan* h, double* out, int max_records);

/* ------------------------------------------------------------------------------------------------------------
 * GPT speech-token decoder
 * ---------------------------------------------------------------------------------------------------------- */
#define ITTS_PREC_F32 0   /* parity mode: f32 weights / KV / MFMA (v_mfma_f32_16x16x4_f32, exact f32) */
#define ITTS_PREC_BF16 1  /* bf16 weights / KV / GEMM inputs, f32 accumulate and residual stream */
#define ITTS_PREC_F32X3 2 /* s2mel and itts_gemm_forward only: f32 activations; GEMMs on the bf16 matrix pipe with every f32 operand carried
                           * exactly as three bf16 planes (x = h + m + l), 8 plane products per f32 product, f32 accumulate.  Weights are
                           * packed for it by itts_pack_gemm_weight(..., precision = 2); attention, norms, gates run their f32 code. */

typedef struct {
    int32_t layers, model_dim, heads;   /* head_dim = model_dim / heads must be 64 */
    int32_t vocab;                      /* number_mel_codes (8194) */
    int32_t n_mel_pos;                  /* rows of mel_pos_embedding (max_mel_tokens + 2 + max_conditioning_inputs) */
    int32_t precision;                  /* ITTS_PREC_* */
    int32_t start_mel_token, stop_mel_token;
    float ln_eps;                       /* 1e-5 (GPT2Config.layer_norm_epsilon / nn.LayerNorm default) */
} itts_gpt_config;

typedef struct {
    int32_t do_sample;                  /* 0: argmax (HF greedy), 1: multinomial after the warpers */
    int32_t num_beams;                  /* 1 for itts_gpt_generate / _chunk / itts_gpt_admit_rows; 2..4 for itts_gpt_generate_beam and the beam
                                           sessions (itts_gpt_generate_beam_chunk, itts_gpt_admit_beam_groups) */
    int32_t top_k;                      /* 1..64 when do_sample */
    int32_t min_tokens_to_keep;         /* 1 (2 under beams) */
    int32_t max_new_tokens;             /* max_generate_length */
    int32_t pos_offset;                 /* 2: HF kv-cache position rule (k-th token at mel position k+1, 1-based k);
                                           1: kv_cache=False rule (positions 0..n-1), model_v2.py:145-161 */
    float top_p, temperature, repetition_penalty, length_penalty;
    float typical_mass;                 /* 0: off; else typical_sampling=True with this typical_mass in (0,1)
                                           (model_v2.py:794-799, indextts/utils/typical_sampling.py:4-30) */
    int32_t reserved;                   /* must be 0 */
    uint64_t seed;                      /* device RNG seed when no uniform stream is supplied */
} itts_gen_params;

typedef struct itts_gpt itts_gpt;

/* host-side packing of a [K][N] (transposed=0, HF Conv1D) or [N][K] (transposed=1, nn.Linear) f32 matrix into
 * MFMA B-fragment order for the given precision (pure CPU). */
size_t itts_packed_gemm_bytes(int K, int N, int precision);
int itts_pack_gemm_weight(const float* w, int K, int N, int transposed, int precision, void* out);

/* replaces: UnifiedVoice.__init__/load_checkpoint/post_init_gpt2_config for the decoder stack
 *   (indextts/gpt/model_v2.py:305-493, indextts/utils/checkpoint.py:22-35).  Tensors by reference state-dict name:
 *   gpt.h.{i}.{ln_1,ln_2}.{weight,bias}, gpt.h.{i}.attn.{c_attn,c_proj}.{weight,bias}, gpt.h.{i}.mlp.{c_fc,c_proj}.*,
 *   gpt.ln_f.*, final_norm.*, mel_head.*, mel_embedding.weight, mel_pos_embedding.emb.weight (host f32 pointers). */
int itts_gpt_create(const itts_gpt_config* cfg, itts_gpt** out);
int itts_gpt_device(const itts_gpt* h);           /* device index the handle is bound to */
int itts_gpt_load_tensor(itts_gpt* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int itts_gpt_finalize(itts_gpt* h);
void itts_gpt_destroy(itts_gpt* h);
size_t itts_gpt_workspace_bytes(const itts_gpt* h, int nseq, int S, int Tmax);

/* replaces: GPT2InferenceModel.generate(...) as called by UnifiedVoice.inference_speech
 *   (indextts/gpt/model_v2.py:815-820 -> vendored GenerationMixin._sample, transformers_generation_utils.py:3123-3297;
 *    per-step forward model_v2.py:121-198; KV cache transformers_gpt2.py:325-328).
 * prefix_embeds [nseq][S][D] f32 device: rows = [left pad][cond][text] embeddings followed by the start-mel row
 *   (mel_embedding[start]+mel_pos[0]) -- what prepare_gpt_inputs + the prefill branch of forward build.
 * pad_lens [nseq] int32 device (left-pad length per row) or NULL.  penalty_ids: host ints already "in input_ids"
 *   for the repetition penalty (the fake prefix id 1 and start_mel).
 * uniforms: optional device f64 [max_new_tokens][nseq] stream for sampled modes (else seeded device RNG).
 * codes_out [nseq][max_new_tokens] int64 device, pre-filled with stop_mel; *n_steps_out = columns generated before
 *   every row finished (HF returns sequences of that length).  Runs on an internal stream ordered after/before
 *   `stream`; the per-token step is one hipGraph replay when use_graph != 0. */
int itts_gpt_generate(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int nseq, int S,
                      const itts_gen_params* params, const int32_t* penalty_ids, int n_penalty_ids,
                      const double* uniforms, int64_t* codes_out, int32_t* n_steps_out, void* workspace,
                      size_t workspace_bytes, int use_graph, void* stream);
/* Chunked form of itts_gpt_generate for streaming (replaces: GPTTRTEngine.generate_chunks, backends/trt/runtime/
 *   gpt_trtllm_runtime.py:381-520, whose TRT-LLM session yields tokens from inside its decode loop).  First call: prefix_embeds
 *   non-NULL -- prefill + decode until `step_limit` tokens exist (or every row finished).  Later calls: prefix_embeds NULL --
 *   the decode loop continues from the device state left in the SAME workspace (KV cache, step / position, finished flags,
 *   repetition set) up to the new step_limit; nseq, S, params->max_new_tokens, codes_out, uniforms must be those of the first
 *   call.  *n_steps_out = steps run so far (< step_limit only when every row has finished).  The first call clamps step_limit to
 *   params->max_new_tokens; a later call may run past it (sessions with itts_gpt_admit_rows): each row is bounded by its OWN step -- from its step
 *   max_new_tokens on it emits the stop token and stores nothing. */
int itts_gpt_generate_chunk(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int nseq, int S,
                            const itts_gen_params* params, const int32_t* penalty_ids, int n_penalty_ids,
                            const double* uniforms, int64_t* codes_out, int32_t step_limit, int32_t* n_steps_out,
                            void* workspace, size_t workspace_bytes, int use_graph, void* stream);
/* Admission of new utterances into a suspended itts_gpt_generate_chunk loop (in-flight batching; design reference: backends/trt/serving/
 *   triton_server.py:96-305, backends/trt/pipeline/pipeline.py:459-548 -- the HF loop itself has no counterpart).  prefix_embeds [n_new][S_new][D]
 *   f32 device: the new prompts at their OWN length (left-padded among themselves, pad_lens [n_new] device: pad positions per row; 1 <= S_new <= the
 *   session's prompt bucket), ending with the start-mel row as for itts_gpt_generate.  slots [n_new] host: the utterances (rows of the first call)
 *   whose cache rows / code rows the new ones take over -- they must have FINISHED.  row_limits_new [n_new] host: the new utterances' token caps,
 *   given exactly when limits are installed (itts_gpt_set_row_limits over the first call's rows; the call writes them into that device array once
 *   every check has passed).  The new rows are prefilled on admit_workspace (itts_gpt_admit_workspace_bytes), keep their keys at their own cache
 *   positions (a per-row shift under the batch's position counter), their code row is refilled with the stop token and their first token lands in
 *   its column 0; the following chunk calls decode them with the rest -- token column, position embedding, uniform / RNG stream and row limit follow
 *   the row's own step; the session's step counter may run past params->max_new_tokens (itts_gpt_generate_chunk), each ROW stops at its own
 *   step max_new_tokens.  params, penalty ids, uniforms, codes_out,
 *   workspace: those of the chunk calls.  The running batch is un-compacted by the call.  An admitted row produces bit for bit the ids it produces
 *   decoded alone, whatever step it joins at (tests/test_gpu_admission.py).  codes_out, uniforms and *params are checked against the ones the
 *   suspended loop was run with (its captured step has them baked in; *params field by field): ITTS_ERR_STATE on a mismatch, the session untouched. */
size_t itts_gpt_admit_workspace_bytes(const itts_gpt* h, int n_new, int S_new);
int itts_gpt_admit_rows(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, const int32_t* slots, int n_new, int S_new,
                        const int32_t* row_limits_new, const itts_gen_params* params, const int32_t* penalty_ids, int n_penalty_ids,
                        const double* uniforms, int64_t* codes_out, void* workspace, size_t workspace_bytes, void* admit_workspace,
                        size_t admit_bytes, void* stream);
/* replaces: the same generate() call in beam mode, num_beams > 1 (the reference default is 3-beam beam-sample,
 *   indextts/infer_v2_5.py:732-740) -> vendored GenerationMixin._beam_search (transformers_generation_utils.py:3325-3609),
 *   BeamSearchScorer.process (3rd-party; mirror indextts/gpt/transformers_beam_search.py:215-305,930-1013) and
 *   _reorder_cache (model_v2.py:200-213, done here as a per-position row map instead of copying the KV cache).
 * prefix_embeds / pad_lens are given per SEQUENCE row (n_utts*num_beams rows, beams of one utterance adjacent, i.e.
 *   repeat_interleave as _expand_inputs_for_generation does); the beams of an utterance must therefore carry identical
 *   prefix rows -- the engine prefills row n*num_beams of each utterance once and all its beams read that prompt K/V
 *   through the row map.  uniforms: optional f64 [max_new][n_utts][2*num_beams].
 * Outputs (device): per step the chosen token and parent row of every sequence row (hist_*: [max_new][n_utts*num_beams]
 *   int32), the running beam scores, the finished-hypothesis records hyps_out [n_utts][4]{f32 score, i32 step, i32 row,
 *   i32 pad}, their count and the per-utterance done flags; BeamSearchScorer.finalize (:320-408) is a host-side walk over
 *   these (indextts_amd/gpt.py).  Max 4 beams.
 * Suspended loops: a handle holds at most ONE suspended decode loop (itts_gpt_generate / _chunk: rows; itts_gpt_generate_beam_chunk: beam groups).
 *   Every first (prefix_embeds non-NULL) call of itts_gpt_generate, _chunk, _beam or _beam_chunk ends it once the call's own argument checks have
 *   passed -- a rejected call leaves it resumable -- so a later resume of, or admission into, the loop that call has overwritten returns
 *   ITTS_ERR_STATE.  itts_gpt_generate_beam itself leaves nothing to resume. */
size_t itts_gpt_beam_workspace_bytes(const itts_gpt* h, int n_utts, int num_beams, int S, int Tmax);
int itts_gpt_generate_beam(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int n_utts, int num_beams,
                           int S, const itts_gen_params* params, const int32_t* penalty_ids, int n_penalty_ids,
                           const double* uniforms, int32_t* hist_tok_out, int32_t* hist_par_out, float* beam_scores_out,
                           float* hyps_out, int32_t* n_hyps_out, uint8_t* done_out, int32_t* n_steps_out,
                           void* workspace, size_t workspace_bytes, int use_graph, void* stream);
/* Beam sessions (v13, additive: beam sessions): the loop of itts_gpt_generate_beam suspended between calls, its finished groups replaced by new
 *   utterances -- in-flight batching for the reference's DEFAULT generation mode (3-beam beam-sample, indextts/infer_v2_5.py:732-740; the loop
 *   replaced is GenerationMixin._beam_search, transformers_generation_utils.py:3325-3609; design reference for the scheduling: TRT-LLM's in-flight
 *   batcher, backends/trt/serving/triton_server.py:96-305, backends/trt/pipeline/pipeline.py:459-548).  A GROUP is one utterance's num_beams adjacent
 *   rows; it is the slot of the session.
 * itts_gpt_generate_beam_chunk -- first call: prefix_embeds non-NULL (arguments as itts_gpt_generate_beam; workspace of
 *   itts_gpt_beam_workspace_bytes: histories, row maps and cache rows are indexed by a group's OWN step and its rows' OWN positions, so that
 *   workspace serves a session of any length): prefill + beam steps until `step_limit` steps exist (clamped to params->max_new_tokens).  Later calls:
 *   prefix_embeds NULL -- the loop continues from the device state in the SAME workspace up to the new step_limit, which may run past
 *   max_new_tokens (each GROUP is bounded by its own step); n_utts, num_beams, S and *params must be those of the first call (else
 *   ITTS_ERR_STATE).  group_caps [n_utts] host or NULL (first call only): per-group cap on own steps, clamped to 1 .. max_new_tokens -- a group at its
 *   cap is treated as the reference treats max_length: the search stops for it, its open beams keep their scores (the host adds them with
 *   generated_len = cap), and it counts as finished.  Every 4 steps the done flags come to the host: the call ends early when every group is done or
 *   capped, or -- itts_gpt_set_chunk_return(k) -- once k groups are.  The seeded device stream is keyed by (seed, own step, slot); there is no
 *   uniforms argument (slots change utterances).  On EVERY return the search state of all groups is copied to the caller's buffers (layout as
 *   itts_gpt_generate_beam; a hypothesis' step and the history rows are own steps), so the host finalises groups as they finish.
 *   *n_steps_out = session steps so far.
 * itts_gpt_admit_beam_groups -- between two chunk calls: n_new utterances take over the groups `slots` [n_new] (host), which must be distinct, in
 *   range and done or capped -- otherwise ITTS_ERR_ARG with every piece of running state untouched.  prefix_embeds [n_new][S_new][D] f32 device: ONE
 *   prompt row per utterance (not repeated per beam), 1 <= S_new <= the session's prompt bucket; pad_lens [n_new] device; group_caps_new [n_new] host
 *   or NULL (written after all checks).  *params must equal the session's, field by field (else ITTS_ERR_STATE, the session untouched).  The prompts are prefilled on admit_workspace
 *   (itts_gpt_admit_beam_workspace_bytes), their K / V copied to cache row slot*num_beams, the group's search state re-initialised, its first beam
 *   step (own step 0) run from the shared logits row and the num_beams next-step inputs placed.  The admitted utterance's hypotheses are, bit for
 *   bit, those it has in the same slot of a batch decoded from step 0, whatever session step it joins at (tests/test_gpu_beam_session.py). */
int itts_gpt_generate_beam_chunk(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int n_utts, int num_beams, int S,
                                 const itts_gen_params* params, const int32_t* penalty_ids, int n_penalty_ids, const int32_t* group_caps,
                                 int32_t* hist_tok_out, int32_t* hist_par_out, float* beam_scores_out, float* hyps_out, int32_t* n_hyps_out,
                                 uint8_t* done_out, int32_t step_limit, int32_t* n_steps_out, void* workspace, size_t workspace_bytes,
                                 int use_graph, void* stream);
size_t itts_gpt_admit_beam_workspace_bytes(const itts_gpt* h, int n_new, int S_new);
int itts_gpt_admit_beam_groups(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, const int32_t* slots, int n_new, int S_new,
                               const int32_t* group_caps_new, const itts_gen_params* params, const int32_t* penalty_ids, int n_penalty_ids,
                               void* workspace, size_t workspace_bytes, void* admit_workspace, size_t admit_bytes, void* stream);
/* HIP-event timings of the last itts_gpt_generate call on its internal stream */
int itts_gpt_last_timing(const itts_gpt* h, float* prefill_ms, float* decode_ms, int32_t* steps);
/* The instantiated decode-step graph is kept in the handle and reused by later generate calls with the same workspace base,
 * batch rows, prompt-length bucket (multiples of 32), max_new_tokens, generation parameters and codes / uniforms pointers (small
 * LRU).  Counters since create: graphs captured, generate calls that reused one. */
int itts_gpt_graph_stats(const itts_gpt* h, int32_t* captures, int32_t* hits);
/* Ragged batches (continuous batching of the decode loop; design reference: backends/trt/pipeline/pipeline.py:459-548,
 * backends/trt/runtime/gpt_trtllm_runtime.py:381-519 -- the HF loop itself keeps finished rows in the batch, generation_utils.py:3256).
 * Utterances that have emitted their stop token leave the running batch: every 8 tokens the survivors are compacted to the front
 * (cache rows stay in place behind a row map) and the step is replayed from the graph of the smaller batch, in buckets of
 * `granularity` rows (default on, 8).  Results are unchanged: a row's arithmetic does not depend on the batch it runs in. */
int itts_gpt_set_compaction(itts_gpt* h, int enable, int granularity);
/* In-flight batching (with itts_gpt_admit_rows): the following itts_gpt_generate_chunk calls return early -- at one of the finished-flag checks the
 * loop makes every 8 steps anyway -- once at least `finished_rows` utterances of the batch have finished (those finished before the call count),
 * so the caller refills their slots without polling in short chunks.  0 = off.  No counterpart in the HF loop; TRT-LLM's in-flight batcher does
 * this inside its executor (backends/trt/serving/triton_server.py:96-305). */
int itts_gpt_set_chunk_return(itts_gpt* h, int finished_rows);
/* Per-utterance caps on generated tokens for the following generate / generate_chunk calls of exactly n utterances (one batch merges
 * requests carrying their own `max_mel_tokens`, infer_v2_5.py:740): utterance u emits the stop token from token index limits[u] on.
 * limits: DEVICE int32 [n], caller-owned, must outlive those calls; NULL clears. */
int itts_gpt_set_row_limits(itts_gpt* h, const int32_t* limits, int n);
/* Code prefix (v13, additive: code prefix).  Replaces: `UnifiedVoice.inference_speech(..., input_tokens=...)` (indextts/gpt/model_v2_5.py:682,
 *   735-751; model.py:660-694), which appends given mel codes to the prompt and generates after them.
 * A row with prefix p[0 .. k) decodes as the row that had generated those k codes itself: its own step starts at k.  Column j of its code row
 *   holds p[j] for j < k and the generated codes from k on; the draw is keyed by (seed, stream, own step) and a given uniform stream is read at
 *   row own step; max_new_tokens and its row limit count the prefix; the repetition penalty's set holds the prefix codes; the logits filters
 *   count from the row's first code; score and alignment columns are the row's own columns (prefix columns hold 0.0, as forced tokens do).
 * codes: DEVICE int64 [n][width], caller-owned, must outlive the calls; lens: HOST int32 [n], 0 .. width (copied); ids of the first lens[b]
 *   columns in 0 .. vocab - 1 (read back and checked here: the call synchronises).  prefix_pos_offset: prefix code j is embedded as
 *   mel_emb[code] + mel_pos[j + prefix_pos_offset] -- itts_gen_params.pos_offset resumes the engine's own run (the decode step's rule; in
 *   exact arithmetic the continuation is the tail of the plain run), 1 is the reference's prefill of input_tokens (positions 0 .. k after the
 *   start token; the next decoded token then sits at k + pos_offset).  chunk 1 .. 65535: prefix positions per pass.
 * Sticky like itts_gpt_set_row_limits; NULL, NULL, 0 clears.  It serves the following FIRST (non-resume) itts_gpt_generate /
 *   itts_gpt_generate_chunk calls with nseq == n, and itts_gpt_admit_rows calls with n_new == n (row i of the table = entry i of the
 *   admission): another size is ITTS_ERR_STATE; lens[b] >= max_new_tokens or positions past the mel position table ITTS_ERR_ARG.  The beam
 *   entries and beam admissions return ITTS_ERR_STATE while a table is installed.
 * After the prompt's prefill the prefix runs through the stack at cache positions S .. S + max(lens) - 1, min(chunk, prompt bucket) positions
 *   per pass on the call's own workspace (itts_gpt_workspace_bytes is unchanged) with the many-query kernels of the rescoring pass; the head
 *   runs on one query per row, its last valid one.  Logits of an ingested prefix are therefore not bit-equal to those of decoded codes.
 *   With no table installed every call issues exactly the launches it always did.
 * An admission with a table needs an admission workspace of itts_gpt_admit_prefix_workspace_bytes(h, n_new, S_new, max(lens)).
 * itts_gpt_last_prefix: max(lens) and the passes of the last first call / admission's ingest (max_len = -1: it ran none). */
int itts_gpt_set_code_prefix(itts_gpt* h, const int64_t* codes, const int32_t* lens, int n, int width, int prefix_pos_offset, int chunk);
size_t itts_gpt_admit_prefix_workspace_bytes(const itts_gpt* h, int n_new, int S_new, int max_prefix);
int itts_gpt_last_prefix(const itts_gpt* h, int32_t* max_len, int32_t* chunks);
/* Per-token log-probabilities (v13, additive: token scores).  Replaces: `output_scores=True, return_dict_in_generate=True` plus
 *   `compute_transition_scores(..., normalize_logits=True)` of the vendored generation utils (indextts/gpt/transformers_generation_utils.py:1132);
 *   the logits never leave the device, so the token selection itself writes the two numbers next to the token it stores.
 * logp_model, logp_sampled: caller-owned DEVICE f32 arrays [n][max_new], laid out like codes_out (row = utterance slot, column = the row's OWN
 *   step), which must outlive the calls.  Sticky like itts_gpt_set_row_limits; NULL, NULL, 0, 0 clears.  Both or neither, else ITTS_ERR_ARG.
 *   logp_model[u][t]   = log_softmax(raw logits row)[token]: the model's own distribution, before the repetition penalty, the logits filters,
 *                        the typical warper, temperature and top-k / top-p.
 *   logp_sampled[u][t] = the log-probability the token was selected with.  Sampling: the log of its share of the renormalised kept set the draw
 *                        itself walked (= compute_transition_scores over `scores`, normalize_logits=True).  Greedy: log_softmax(processed row)[token];
 *                        entries the filters set to -inf contribute nothing.
 *   A forced token -- the row had already finished, or its own step is at / past its row limit or max_new_tokens -- gets 0.0f in both, at the
 *   columns where a token is stored; the first stop token the model chose itself IS scored.
 * Accumulation: the row maximum in f32 (exact), f32 exponentials summed in F64, f64 log, one rounding to f32.  Every reduction runs in one fixed
 *   order, so the BITS of a row's scores do not depend on the batch, the dense row, compaction or the step at which the row joined.
 * Serves the following itts_gpt_generate / itts_gpt_generate_chunk / itts_gpt_admit_rows calls with exactly n utterances and max_new_tokens ==
 *   max_new (else they return ITTS_ERR_STATE).  A first call (prefill) zero-fills both arrays; an admission zero-fills the rows of the slots it takes
 *   over before the new row's first token is scored, as it refills the code row with the stop token.  The pointers are part of the decode graph's key.
 *   With nothing installed the selection kernel is the one it always was (a separate instantiation carries the scores).
 * Beam calls, beam sessions and beam admissions with scores installed return ITTS_ERR_STATE (per-token transition scores of a beam need
 *   beam_indices, which the beam entries do not expose). */
int itts_gpt_set_token_scores(itts_gpt* h, float* logp_model, float* logp_sampled, int n, int max_new);
/* Text-attention export (v13, additive: alignment export).  Replaces: `output_attentions=True` of the vendored GPT-2 / generation utils
 *   (indextts/gpt/transformers_gpt2.py:189, GPT2Attention._attn returns attn_weights), which hands back every layer's whole matrix; here the decode
 *   steps write the softmax weights of a few selected (layer, head) pairs over each utterance's text span, and nothing else leaves the device.
 * pairs: HOST int32 [n_pairs][2] (layer, head), 1 <= n_pairs <= 8, in range and distinct (copied).  span: DEVICE int32 [n][2] (off, len) per
 *   utterance slot, relative to the row's first valid key (its left padding), so an admitted row needs no special case; read every step.
 *   out: DEVICE f32 [n][max_new][n_pairs][text_cap]; text_cap a multiple of 4, 4 .. 1024.  Both caller-owned, must outlive the calls.  Sticky like
 *   itts_gpt_set_token_scores; NULL, 0, NULL, NULL, 0, 0, 0 uninstalls.
 * A decode step writes, for dense row b carrying utterance u at the row's own step rstep (the column its token is stored in), pair k = (l, hd):
 *     out[u][rstep][k][j] = softmax_{t in first..last}(q . K_t / 8)[first + off + j],   j < len;   0 where first + off + j > last
 *   with first / last and the keys exactly those layer l's attention reads at that step (itts_gpt_attention_forward, nq = 1, no row map).  Columns
 *   len .. text_cap - 1 are never written.  Nothing is written when the step's token is forced (the row had finished, or rstep is at / past its row
 *   limit or max_new): those rows keep the zeros of the fill.  Row 0 stays zero: code 0 comes from the prefill, whose attention is not exported.
 * Reduction: exact f32 maximum; e_t = expf(s_t - max) in f32, computed once; their sum in F64 in one fixed order (per thread ascending keys, xor-shuffle
 *   tree, the sixteen wave partials in index order); p = (float)(e_t / sum).  The BITS of a row do not depend on the batch, the dense row, compaction, the
 *   fused-LayerNorm path or the step at which the row joined.
 * Serves itts_gpt_generate / itts_gpt_generate_chunk / itts_gpt_admit_rows calls with exactly n utterances and max_new_tokens == max_new (else they
 *   return ITTS_ERR_STATE).  A first call (prefill) zero-fills `out`; an admission zero-fills the rows of the slots it takes.  The arrays and the pair
 *   list are part of the decode graph's key (a captured step bakes in which launches exist).  With nothing installed a transformer pass issues exactly
 *   the launches it always did.  Beam calls, beam sessions and beam admissions with an export installed return ITTS_ERR_STATE. */
int itts_gpt_set_alignment(itts_gpt* h, const int32_t* pairs, int n_pairs, const int32_t* span, float* out, int n, int max_new, int text_cap);
/* Per-slot sampling settings (v13, additive: per-slot sampling table): one decode batch carries requests that each chose their own temperature /
 *   top_p / top_k / repetition penalty / typical mass / seed -- per-request settings in one batch, as the reference's serving path keeps them
 *   (backends/trt/serving/triton_server.py:96-305); the HF loop takes one set per generate() call.  table: DEVICE array of n entries, caller-owned,
 *   must outlive the calls; one entry per utterance slot of the following itts_gpt_generate / itts_gpt_generate_chunk / itts_gpt_admit_rows calls,
 *   which must have exactly n utterances (else ITTS_ERR_STATE).  It stays installed across chunk calls and admissions; NULL, 0 uninstalls it.
 * While installed the token selection reads slot u's entry EVERY step and ignores do_sample, top_k, min_tokens_to_keep, top_p, temperature,
 *   repetition_penalty, typical_mass and seed of itts_gen_params; max_new_tokens, num_beams, pos_offset and length_penalty still apply, and
 *   `uniforms`, when given, still replace the RNG.  The RNG draw of a row is keyed by (entry.seed, the row's own step, entry.stream): `stream`
 *   stands where the scalar path keys the slot index, so a table holding the call's scalars with stream = slot in every entry reproduces the
 *   scalar call bit for bit, and an entry with a fixed stream makes a request's ids independent of the slot it runs in.
 * The entries are checked HERE (one device-to-host copy), not in the kernel: do_sample with top_k outside 1..64, typical_mass outside (0,1)
 *   unless 0, repetition_penalty or temperature <= 0, min_tokens_to_keep outside 0..2 -> ITTS_ERR_ARG, nothing installed.  Because the kernel reads
 *   the entry every step, the host may rewrite the entry of a FINISHED slot, in stream order, before it admits a new utterance there with
 *   itts_gpt_admit_rows (whose signature is unchanged); such entries keep to the domain above.  The table pointer is part of the decode graph's key.
 * Beam calls and beam sessions with a table installed return ITTS_ERR_STATE (the beam kernels take their own table: itts_gpt_set_group_sampling). */
typedef struct {
    int32_t  do_sample, top_k, min_tokens_to_keep;
    float    top_p, temperature, repetition_penalty, typical_mass;
    int32_t  stream;                    /* RNG stream key; the scalar path uses the slot index */
    uint64_t seed;
} itts_row_sampling;
int itts_gpt_set_row_sampling(itts_gpt* h, const itts_row_sampling* table, int n);
/* Per-group sampling settings of the beam kernels (v13, additive: per-group sampling table): itts_gpt_set_row_sampling for num_beams > 1 -- the
 *   reference's default generation mode is 3-beam beam-sample (indextts/infer_v2_5.py:732-740), and its serving path keeps per-request settings in
 *   one batch (backends/trt/serving/triton_server.py:96-305); the HF beam loop takes one set per generate() call.  Replaces: one top_p / top_k /
 *   temperature / repetition_penalty / typical_mass / length_penalty / seed per beam batch, and the slot-keyed beam draw.  table: DEVICE array of
 *   n_groups entries, caller-owned, must outlive the calls; one entry per utterance (= beam group) of the following itts_gpt_generate_beam /
 *   itts_gpt_generate_beam_chunk / itts_gpt_admit_beam_groups calls, which must have exactly n_groups utterances (else ITTS_ERR_STATE).  It stays
 *   installed across chunk calls and admissions; NULL, 0 uninstalls it.
 * While installed the two beam kernels read group u's entry EVERY step and ignore do_sample, top_k, min_tokens_to_keep, top_p, temperature,
 *   repetition_penalty, typical_mass, length_penalty and seed of itts_gen_params (which are still range-checked as without a table, and still
 *   compared field by field at a resume / admission); num_beams, max_new_tokens and pos_offset stay call-wide: they fix the layout.  Beam search
 *   (do_sample = 0) and beam-sample groups may share a batch.  length_penalty enters the hypothesis scores and the done rule on the device; the
 *   host's finaliser must use the same per-group value.  The draw d of a group's own step s is keyed (entry.seed, s * 8 + d, entry.stream):
 *   `stream` stands where the scalar path keys the group's slot, so a table holding the call's scalars with stream = slot in every entry
 *   reproduces the scalar call bit for bit, and an entry with a fixed stream makes a request's ids independent of the slot it runs in.
 *   `uniforms`, when given, still replace the RNG.
 * The entries are checked HERE (one device-to-host copy), not in a kernel: do_sample with top_k < 1 or max(top_k, min_tokens_to_keep) > 64,
 *   typical_mass outside (0,1) unless 0, repetition_penalty or temperature <= 0, min_tokens_to_keep outside 0..2 -> ITTS_ERR_ARG, nothing
 *   installed.  The host may rewrite the entry of a FINISHED group, in stream order, before it admits a new utterance there with
 *   itts_gpt_admit_beam_groups (whose signature is unchanged); such entries keep to the domain above.  The table pointer is part of the beam
 *   step graph's key.
 * The two tables stay apart: with this one installed itts_gpt_generate / _chunk / itts_gpt_admit_rows (num_beams = 1) return ITTS_ERR_STATE, as
 *   the beam entries do with an itts_row_sampling table (an entry without length_penalty is not a beam entry). */
typedef struct {
    int32_t  do_sample, top_k, min_tokens_to_keep;
    float    top_p, temperature, repetition_penalty, typical_mass, length_penalty;
    int32_t  stream;                    /* RNG stream key; the scalar path keys the group's slot */
    uint64_t seed;
} itts_group_sampling;
int itts_gpt_set_group_sampling(itts_gpt* h, const itts_group_sampling* table, int n_groups);
/* Logits filters (v13, additive: device logits processors): the processors and warpers that GenerationMixin._get_logits_processor builds from
 *   generate() kwargs beyond the engine's defaults (indextts/gpt/transformers_generation_utils.py:843-1070; the reference forwards
 *   **hf_generate_kwargs there, indextts/gpt/model_v2.py:815-820), applied inside the selection kernels in HF's order -- repetition penalty,
 *   no-repeat-ngram, bad words, min_length, min_new_tokens, exponential decay, suppress, begin-suppress, [typical warper], temperature, top-k,
 *   top-p, min-p, epsilon, eta -- at no extra launch.  Replaces: NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor (single-token words:
 *   pass them among suppress_ids; an entry equal to [eos] is dropped as HF drops it), MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
 *   ExponentialDecayLengthPenalty, SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor, MinPLogitsWarper, EpsilonLogitsWarper,
 *   EtaLogitsWarper of transformers.generation.logits_process.  In the beam entries they act on the log-probs, as the repetition penalty does.
 * Sticky handle state, like itts_gpt_set_row_limits: it serves every following generate / chunk / beam / admission call until f == NULL clears it.
 *   All arrays are HOST arrays, copied here into handle-owned device buffers whose addresses never change; the kernels read every setting from
 *   device memory, so the decode graph's key carries only whether a filter is installed, never its values.  Do not change it while a chunked
 *   loop is suspended on the handle.
 * Steps are the row's OWN step (an utterance admitted into a session behaves as decoded alone); `prompt length` is the S of the call (for an
 *   admitted row its own S_new): the fake ids HF sees are [1] * (S - 1) + [start_mel_token], which is also the prefix of the n-gram history.
 *   The warpers run with do_sample only and keep min_tokens_to_keep ids; the score processors run in every mode.
 * no_repeat_ngram_size serves num_beams = 1: with it installed the beam entries return ITTS_ERR_ARG (a beam's history is not kept per row).
 * Checked here (ITTS_ERR_ARG, nothing installed): h == NULL; min_new_tokens / min_length / no_repeat_ngram_size < 0; min_p > 1; epsilon_cutoff
 *   or eta_cutoff outside (0, 1) unless 0; ids outside 0 .. vocab - 1; n_decay above n_mel_pos + 1; a count without its array. */
typedef struct {
    int32_t  min_new_tokens;            /* 0 = off: the stop token is -inf while the row's own step < min_new_tokens */
    int32_t  min_length;                /* 0 = off: ... while prompt length + own step < min_length */
    int32_t  no_repeat_ngram_size;      /* 0 = off */
    int32_t  decay_start;               /* exponential_decay_length_penalty[0]; read when n_decay > 0 */
    float    min_p;                     /* negative = off, else in [0, 1] */
    float    epsilon_cutoff;            /* 0 = off, else in (0, 1) */
    float    eta_cutoff;                /* 0 = off, else in (0, 1) */
    int32_t  n_suppress, n_begin_suppress, n_decay;
    const int32_t* suppress_ids;        /* host [n_suppress]: -inf at every step (suppress_tokens, single-token bad_words_ids) */
    const int32_t* begin_suppress_ids;  /* host [n_begin_suppress]: -inf at the row's step 0 */
    const float*   decay_table;         /* host [n_decay]: entry t = f32(factor ** (t - decay_start) - 1) for t > decay_start, formed in double as HF
                                         * forms it; the stop score at own step t becomes score + |score| * entry (steps past the table: its last entry) */
} itts_logits_filters;
int itts_gpt_set_logits_filters(itts_gpt* h, const itts_logits_filters* f);   /* f == NULL clears */
/* Per-slot logits filters (v13, additive: per-request filters in one batch; design reference: per-request settings in one batch,
 *   backends/trt/serving/triton_server.py:96-305): a TABLE of filter records, one per utterance slot (itts_gpt_generate / _chunk / admit_rows) or
 *   per beam group (the beam entries).  A selection block loads its own slot's record -- the index of the row-sampling table: the utterance a
 *   compacted dense row carries, the group after the subset map -- where it would load the call-wide one.
 * entries: HOST array of n itts_logits_filters records (their arrays host arrays too); slots: the n slots they go to, NULL = 0 .. n-1; n_slots:
 *   the table's size, which the generate entries require to equal their utterances (ITTS_ERR_STATE otherwise).  The first installation after
 *   an uninstall sizes the table and fills every unnamed slot with the OFF record (all counts 0, no decay, min_p off, cutoffs 0, empty mask),
 *   under which a row computes the bits of the unfiltered kernel; later calls rewrite the named slots only (an admission's).
 *   entries == NULL uninstalls: the call-wide record, if any, rules again.  While a table is installed it rules for EVERY slot; the call-wide
 *   record is not read (the caller merges its defaults into the entries).
 * Each entry is checked as itts_gpt_set_logits_filters checks its record (ITTS_ERR_ARG, naming the entry; nothing is written unless all pass).
 *   Sticky handle state like the call-wide record.  The table, the [n_slots][vocab] masks and the [n_slots][n_mel_pos + 1] decay rows are
 *   handle-owned device memory (freed by itts_gpt_destroy, not before) that does not move while installed; the handle's stream is synchronised before a rewrite; the kernels read
 *   everything from device memory, so the decode graph's key carries the table's address, never its contents.  n_slots may not change while a
 *   decode loop is suspended on the handle (ITTS_ERR_STATE).  An entry with no_repeat_ngram_size > 0 makes the beam entries return
 *   ITTS_ERR_ARG, as the call-wide one does. */
int itts_gpt_set_row_filters(itts_gpt* h, const itts_logits_filters* entries, const int32_t* slots, int n, int n_slots);
/* Of the last generate call: sum over its decode steps of the rows each step ran (= steps x utterances without compaction), and
 * the number of compactions. */
int itts_gpt_compaction_stats(const itts_gpt* h, int64_t* row_steps, int32_t* compactions);

/* replaces: UnifiedVoice.forward(..., return_latent=True) transformer pass (model_v2.py:596-646, get_logits
 *   :528-554; call site indextts/infer_v2.py:636-651): x [nseq][S][D] -> final_norm(ln_f(blocks(x))) [nseq][S][D]. */
int itts_gpt_forward_latent(itts_gpt* h, const float* x, int nseq, int S, float* out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* Teacher-forced latent SESSION: itts_gpt_forward_latent with its KV cache kept, for streaming IndexTTS-2 -- every chunk of codes needs the latents
 *   of its mel positions, and the pass is causal and unmasked, so the latents of a code prefix are those of the finished utterance.
 *   replaces, per chunk: UnifiedVoice.forward(..., return_latent=True) (model_v2.py:528-554,596-646); the reference's streaming pipeline takes the
 *   chunk's latent out of its TRT-LLM session (backends/trt/runtime/gpt_trtllm_runtime.py:381-519).
 * itts_gpt_latent_open (replaces model_v2.py:528-554,596-646 over the prefix; gpt_trtllm_runtime.py:381-519 context phase): prefix_x
 *   [nseq][max_prefix][D] f32 device = conds | text_emb([start_text, ids, stop_text]) of every row, RIGHT-padded to max_prefix (any finite values);
 *   prefix_lens [nseq] HOST int32, 1 .. max_prefix, rows may differ.  The prefix is prefilled into a KV cache inside `workspace`
 *   (itts_gpt_latent_workspace_bytes; the caller keeps it alive and untouched until close).  The session owns that workspace alone: it may be opened,
 *   appended to and closed while an itts_gpt_generate_chunk loop is suspended on the same handle, whose state it does not touch.
 * itts_gpt_latent_append (replaces model_v2.py:528-554,596-646 over the new mel positions; gpt_trtllm_runtime.py:381-519 generation phase):
 *   codes [nseq][n] int64 device = the NEXT n codes of every row (rows that have ended are fed their stop-token padding); out [nseq][n][D] f32
 *   device = final_norm(ln_f(hidden)) at the n new mel positions: position j of a row has input mel_emb[code j-1] + mel_pos[j] (start_mel for
 *   j = 0), i.e. out[b][i] is the latent that goes with code `appended + i`.  ITTS_ERR_ARG: n outside 1 .. max_append, more than max_codes
 *   appended in all, a position past the mel position table; ITTS_ERR_STATE: the session is closed.  Ids outside the code table are clamped.
 * itts_gpt_latent_appended: mel positions appended so far (-1: closed).  itts_gpt_latent_close (replaces the end of the reference's per-request
 *   session, gpt_trtllm_runtime.py:381-519; model_v2.py:528-554,596-646 keep no state): frees the session object (the workspace is the caller's);
 *   ITTS_ERR_STATE when already closed.  itts_gpt_destroy closes the handle's open sessions. */
typedef struct itts_gpt_latent itts_gpt_latent;
size_t itts_gpt_latent_workspace_bytes(const itts_gpt* h, int nseq, int max_prefix, int max_codes, int max_append);
int itts_gpt_latent_open(itts_gpt* h, const float* prefix_x, const int32_t* prefix_lens, int nseq, int max_prefix, int max_codes,
                         int max_append, void* workspace, size_t workspace_bytes, void* stream, itts_gpt_latent** session);
int itts_gpt_latent_append(itts_gpt_latent* session, const int64_t* codes, int n, float* out, void* stream);
int itts_gpt_latent_appended(const itts_gpt_latent* session);
int itts_gpt_latent_close(itts_gpt_latent* session);

/* Teacher-forced rescoring (v13, additive: rescoring pass): per-token log-probabilities and text attention of GIVEN codes -- a beam search's
 *   result, codes kept from an earlier call, codes of another checkpoint or precision -- which the decode step's own exports (itts_gpt_set_token_scores,
 *   itts_gpt_set_alignment: num_beams = 1, live steps only) cannot give.
 * itts_gpt_rescore (replaces: teacher forcing through UnifiedVoice.forward / get_logits, indextts/gpt/model_v2.py:528-554,596-646, followed by
 *   compute_transition_scores(normalize_logits=True), indextts/gpt/transformers_generation_utils.py:1132, and by output_attentions=True,
 *   indextts/gpt/transformers_gpt2.py:189, whose logits (rows x 8194) and whole attention matrices go to the host; here neither leaves the device):
 *   prefix_embeds [nseq][S][D] f32 and pad_lens [nseq] exactly as itts_gpt_generate takes them (left-padded, the start-mel row last); codes
 *   [nseq][max_codes] DEVICE int64; code_lens [nseq] HOST int32, 0 .. max_codes; pos_offset as itts_gen_params.pos_offset; logp_out DEVICE f32
 *   [nseq][max_codes]; optionally pairs HOST int32 [n_pairs][2], span DEVICE int32 [nseq][2], align_out DEVICE f32 [nseq][max_codes][n_pairs][text_cap]
 *   and text_cap with the rules of itts_gpt_set_alignment (all NULL / 0: no export; S + max_codes <= 12288 with one); chunk 1 .. 65535 = positions
 *   per pass.  The prompt is prefilled; its last position is the query that predicts code 0.  Then, `chunk` positions at a time, position
 *   S - 1 + i (i >= 1) gets the DECODE step's input mel_emb[codes[b][i - 1]] + mel_pos[i - 1 + pos_offset] (its position quirk included -- not
 *   the forward() layout of the latent session), the stack runs as a prefill over the chunk with the rows' pad, ln_f -> final_norm and the head
 *   GEMM run on the chunk's rows and
 *     logp_out[b][i]        = log_softmax(logits of the query that predicts code i)[codes[b][i]]     (the arithmetic of logp_model: f32 max, f32
 *                             exponentials summed in F64 in one fixed order, f64 log, one rounding; 0.0f for an id outside the code table)
 *     align_out[b][i][k][j] = softmax_{first..last}(q . K / 8)[first + off + j], j < len, for pair k = (layer, head): the definition of
 *                             itts_gpt_set_alignment with last = S - 1 + i, computed after layer l's QKV GEMM (reduction order as there)
 *   for i < code_lens[b]; both are ZERO for i >= code_lens[b] and align_out in the columns from len on.  Row 0 IS written -- the start-mel
 *   query's attention -- which the decode export leaves zero: a documented difference.  Ids outside the code table are clamped for the embedding.
 *   Workspace (itts_gpt_rescore_workspace_bytes): a KV cache of S + max_codes positions, and activations / logits of max(S, chunk) and chunk rows per
 *   sequence -- it grows with chunk, not with max_codes, except for the cache.  The pass OWNS that workspace and nothing else: it shares the
 *   handle's weights and stream, reads none of the installed tables (row limits, sampling tables, logits filters, score / alignment arrays) and
 *   touches nothing of a decode or beam loop suspended on the handle (itts_gpt_generate_chunk / itts_gpt_generate_beam_chunk), which resumes with
 *   the bits it would have produced without the call, as with the latent session.  No graph capture.  ITTS_ERR_ARG: a shape out of range (nseq,
 *   S, chunk <= 65535; nseq * S and nseq * chunk <= 2^24; nseq * chunk * vocab < 2^31; the workspace query then returns 0), a
 *   code_lens entry outside 0 .. max_codes, positions past the mel position table, a bad pair list / text_cap, a workspace too small. */
size_t itts_gpt_rescore_workspace_bytes(const itts_gpt* h, int nseq, int S, int max_codes, int chunk);
int itts_gpt_rescore(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int nseq, int S, const int64_t* codes,
                     const int32_t* code_lens, int max_codes, int pos_offset, float* logp_out, const int32_t* pairs, int n_pairs,
                     const int32_t* span, float* align_out, int text_cap, int chunk, void* workspace, size_t workspace_bytes, void* stream);
/* unit-level forms of the two kernels of the rescoring pass.
 * itts_gpt_logp_gather_forward (replaces compute_transition_scores over teacher-forced logits, transformers_generation_utils.py:1132): logits DEVICE f32
 *   [rows][ldl] with V <= ldl valid columns, targets DEVICE int64 [rows]: out[r] = (float)(((double)row[tok] - max) - log sum_i exp(row[i] - max)), tok =
 *   targets[r]; 0.0f when tok lies outside 0 .. V - 1 or the row's max is -inf.  One block per row; the reduction of itts_gpt_set_token_scores.
 * itts_gpt_attention_align_mq_forward (replaces output_attentions=True over a teacher-forced pass, transformers_gpt2.py:189): the many-query form
 *   of itts_gpt_attention_align_forward, with the argument conventions of itts_gpt_attention_forward: q [nseq][nq][heads_model * 64] f32; for sequence
 *   b, the i-th listed head and query qi < (q_len ? q_len[b] : nq), last = min(*pos_ptr + qi - pos_shift[pb], Tmax - 1), (off, len) = span[b]:
 *     out[b][row0 + qi][i][j] = softmax_{t in first..last}(q[b][qi][hd] . K[pb][hd][t] / 8)[first + off + j],  j < min(len, text_cap);  0 past `last`;
 *   queries from q_len[b] on write nothing.  out DEVICE f32 [nseq][out_rows][n_heads][text_cap], row0 + nq <= out_rows; span DEVICE int32 [nseq][2];
 *   q_len DEVICE int32 [nseq] or NULL.  A query's row has the BITS itts_gpt_attention_align_forward gives for the same q row, cache and tables; a block
 *   serves a tile of min(8, 15872 / Tmax) (at least 1) consecutive queries, so each key load feeds the whole tile.  Tmax <= 12288. */
int itts_gpt_logp_gather_forward(const float* logits, const int64_t* targets, float* out, int rows, int V, int ldl, void* stream);
int itts_gpt_attention_align_mq_forward(const float* q, const void* kcache, float* out, const int32_t* span, const int32_t* heads, int n_heads,
                                        const int32_t* pos_ptr, const int32_t* pad, const int32_t* pos_shift, const int32_t* seq_map,
                                        const int32_t* q_len, int nseq, int n_heads_model, int nq, int Tmax, int seq_mul, int row0, int out_rows,
                                        int text_cap, int precision, void* stream);

/* diagnostics: resident blocks per CU the HIP runtime predicts for the 128 x 128 tile GEMM kernel of a precision (0 f32, 1 bf16, 2 f32x3) */
int itts_gemm_tile_occupancy(int precision, int32_t* blocks_per_cu);
/* which GEMM kernel and geometry ran: every GEMM launcher records, on the host and per calling thread, the path it is about to launch.
 * itts_gemm_last_path: the name of the path the calling thread's last GEMM launch took ("none" before the first); itts_gemm_path_count /
 * itts_gemm_path_name(0 .. count - 1): every path name (NULL outside the range).  Names: bf16_tile128[_novec], bf16_tile256, bf16_tile256x128,
 * bf16_reg_prefill, bf16_slab_mt1 / _mt2 / _mt4_nt1 / _mt4_nt2 / _mt4_nt4, bf16_reg_decode_mt1 / 2 / 4, f32_tile, f32_reg_prefill,
 * f32_reg_decode_mt1 / 2 / 4, x3_4w_p6 / _p8 / _aplanes, x3_8w, bf16_ln_decode_4w, bf16_ln_decode_wide_nt2 / _nt4.  Launches replayed from a
 * captured graph record nothing (the record is made when the launch is issued). */
const char* itts_gemm_last_path(void);
int itts_gemm_path_count(void);
const char* itts_gemm_path_name(int index);
/* unit-level ops for the parity tests: C[M,N] = A[M,K] * W + bias (A in the precision's activation dtype), LayerNorm */
int itts_gemm_forward(const void* A, const void* Wp, const float* bias, float* out, int M, int N, int K, int precision,
                      int prefill_tiles, int gelu, void* stream);
int itts_layernorm_forward(const float* x, const float* gamma, const float* beta, const float* gamma2,
                           const float* beta2, float* out, int rows, int D, float eps, void* stream);
/* which KV-cache attention kernel and geometry ran: launch_attention records, on the host and per calling thread, the path it is about to launch
 * (as the GEMM launchers do).  itts_attention_last_path: the calling thread's last one ("none" before the first); itts_attention_path_count /
 * itts_attention_path_name(0 .. count - 1): every name (NULL outside the range).  Names: streams_{f32,bf16}_w{4,8,16}[_rmap] -- the canonical-stream
 * kernel by cache precision, waves per block and beam row map -- and prefill_mfma_{f32,bf16}, the causal MFMA kernel of S > 1 passes. */
const char* itts_attention_last_path(void);
int itts_attention_path_count(void);
const char* itts_attention_path_name(int index);
/* unit-level form of one layer's KV-cache attention (what every transformer pass launches between its qkv and projection GEMMs; the reference's
 * counterpart is GPT2Attention._attn over past_key_values, indextts/gpt/transformers_gpt2.py:189): for sequence b, head h, query qi
 *   pb    = seq_map ? seq_map[b] : b * max(seq_mul, 1)                       physical cache row / entry of pad and pos_shift
 *   last  = min(*pos_ptr + qi - (pos_shift ? pos_shift[pb] : 0), Tmax - 1),  first = pad ? pad[pb] : 0
 *   out[b][qi][h] = softmax_{t in first..last}(q[b][qi][h] . K[row(t)][h][t] / 8) V[row(t)][h][t]   (0 when the window is empty)
 *   row(t) = (row_map ? ((*step_ptr & 1) ? row_map_alt : row_map)[b * Tmax + t] : pb).
 * All pointers are device memory.  q [nseq][nq][heads * 64] f32; kcache / vcache [rows][heads][Tmax][64] and out [nseq][nq][heads * 64] are f32 for
 * precision 0 and bf16 for precision 1 (ITTS_PREC_F32X3 is refused: the GPT has no such mode).  pos_ptr, step_ptr: one int32 each; pad, pos_shift: one
 * int32 per cache row; seq_map [nseq]; row_map, row_map_alt [nseq][Tmax]; every one but pos_ptr may be NULL (row_map_alt and step_ptr come together
 * and with row_map).  The launch must stay inside what the caller allocated: *pos_ptr + nq <= Tmax when nq > 1 (a decode step, nq = 1, is clamped to
 * Tmax - 1).  Kernel and geometry follow the options attn_waves / prefill_attn exactly as inside the engine. */
int itts_gpt_attention_forward(const float* q, const void* kcache, const void* vcache, void* out, const int32_t* pos_ptr, const int32_t* pad,
                               const int32_t* pos_shift, const int32_t* seq_map, const int32_t* row_map, const int32_t* row_map_alt,
                               const int32_t* step_ptr, int nseq, int heads, int nq, int Tmax, int seq_mul, int precision, void* stream);
/* unit-level form of the alignment export (the launch itts_gpt_set_alignment adds to a decode step, after the layer's qkv GEMM), with the argument
 * conventions of itts_gpt_attention_forward (nq = 1, no row map): for dense row b and the i-th listed head hd = heads[i] (HOST int32 [n_heads],
 * 1 .. 8, distinct), u = row_slot ? row_slot[b] : b, rstep = *step_ptr - (row_step0 ? row_step0[u] : 0), (off, len) = span[u]:
 *     out[u][rstep][i][j] = softmax_{t in first..last}(q[b][hd] . K[pb][hd][t] / 8)[first + off + j],  j < min(len, text_cap);  0 past `last`.
 * Nothing is written for a row with finished[u] != 0, rstep < 0, rstep >= max_new or rstep >= row_limit[u].  q [nseq][heads_model * 64] f32; kcache
 * [rows][heads_model][Tmax][64] f32 (precision 0) or bf16 (1); out DEVICE f32 [utterances][max_new][n_heads][text_cap]; span DEVICE int32
 * [utterances][2]; pad, pos_shift per cache row; seq_map, row_slot [nseq]; row_step0, row_limit [utterances] int32, finished [utterances] bytes; every
 * table but span may be NULL.  Tmax <= 12288 (one f32 score per cache position is kept in LDS); text_cap a multiple of 4, 4 .. 1024. */
int itts_gpt_attention_align_forward(const float* q, const void* kcache, float* out, const int32_t* span, const int32_t* heads, int n_heads,
                                     const int32_t* pos_ptr, const int32_t* pad, const int32_t* pos_shift, const int32_t* seq_map,
                                     const int32_t* row_slot, const int32_t* step_ptr, const int32_t* row_step0, const int32_t* row_limit,
                                     const uint8_t* finished, int nseq, int n_heads_model, int Tmax, int seq_mul, int max_new, int text_cap,
                                     int precision, void* stream);
/* unit-level form of the LayerNorm-fused decode GEMM (what a decode step of 1-4 rows runs instead of a LayerNorm launch + a GEMM launch;
 * replaces GPT2Block's ln_1 -> c_attn and ln_2 -> c_fc pairs, indextts/gpt/transformers_gpt2.py:616-618,652-654, for a single new position):
 *   x' = x + (p0 + p1) + (p2 + p3) + bias_prev  when `partial` ([4][M][K] f32 split-K partials of the previous GEMM) is given, else x' = x;
 *   out [M][N] f32 = bf16(LayerNorm(x'; ln_gamma, ln_beta, eps)) * W (bf16-packed, precision 1) + bias;  x_out [M][K] = x' (required with
 *   `partial`, and a different buffer than x).  M <= 4, K in {256, 512, 1280}.  Bitwise itts_layernorm_forward -> bf16 -> itts_gemm_forward. */
int itts_gemm_ln_forward(const float* x, const float* partial, const float* bias_prev, const float* ln_gamma, const float* ln_beta, float eps,
                         const void* Wp, const float* bias, float* out, float* x_out, int M, int N, int K, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * s2mel flow-matching decoder (DiT estimator + classifier-free-guidance Euler solver)
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t hidden_dim, num_heads, depth;          /* DiT (head_dim must be 64)                                   */
    int32_t in_channels;                           /* mel bands (80)                                              */
    int32_t wavenet_hidden, wavenet_layers, wavenet_kernel, wavenet_dilation_rate;
    int32_t precision;                             /* ITTS_PREC_F32 (what the reference computes, infer_v2_5.py:827-828), _BF16 (GEMM
                                                    * operands / Q K V P in bf16, f32 accumulate) or _F32X3 */
    float norm_eps;
} itts_s2mel_config;

typedef struct itts_s2mel itts_s2mel;

/* replaces: CFM.__init__ / DiT.__init__ + load_checkpoint2 (indextts/s2mel/modules/flow_matching.py:117-135,
 *   diffusion_transformer.py:103-184, commons.py load_checkpoint2; call site indextts/infer_v2_5.py:190-206).
 * Tensors by reference state-dict name under `estimator.` with weight-norm folded into `.weight` (host f32): per layer
 *   transformer.layers.{i}.attention.{wqkv,wo}.weight, feed_forward.{w1,w2,w3}.weight, {attention_norm,ffn_norm}.norm.weight,
 *   skip_in_linear.{weight,bias} (layers past the middle); transformer.norm.norm.weight; cond_x_merge_linear.weight (its mel
 *   columns are used); skip_linear, conv1, res_projection, final_layer.linear, conv2 {weight,bias};
 *   wavenet.{in_layers,res_skip_layers}.{i}.conv.conv.{weight,bias}. */
int itts_s2mel_create(const itts_s2mel_config* cfg, itts_s2mel** out);
int itts_s2mel_device(const itts_s2mel* h);
int itts_s2mel_load_tensor(itts_s2mel* h, const char* name, const float* host_data, const int64_t* shape, int ndim);
int itts_s2mel_finalize(itts_s2mel* h);
void itts_s2mel_destroy(itts_s2mel* h);
size_t itts_s2mel_workspace_bytes(const itts_s2mel* h, int n_tok, int n_seq, int t_max);
/* floats of per-step modulation vectors the host supplies (everything that depends on the timestep only):
 *   per layer [attention_norm (weight|bias) 2H][ffn_norm 2H], transformer.norm 2H, WaveNet cond_layer output L*2W,
 *   final-layer (shift|scale) 2W -- AdaptiveLayerNorm.project_layer / WN.cond_layer / FinalLayer.adaLN_modulation applied
 *   to the timestep embeddings (gpt_fast/model.py:31-37, wavenet.py:150, diffusion_transformer.py:98). */
int itts_s2mel_mods_per_step(const itts_s2mel* h);

/* Token layout of both calls: the sequences (CFG branch major: all utterances of the conditional branch, then the null
 * branch) are packed back to back into [n_tok][channels] matrices.  Device int32 tables: tok_seq / tok_t [n_tok] (sequence and
 * frame of a row), seq_start / seq_T / seq_len [n_seq] (first row, frames processed, valid frames = the reference's x_lens).
 * rope [t_max][32][2] f32 (cos, sin) = precompute_freqs_cis rows (gpt_fast/model.py:336-345).
 * const_in [n_tok][hidden] f32 = cond_x_merge_linear applied to the step-invariant columns (prompt mel, projected content,
 * style) plus its bias (diffusion_transformer.py:205-216).
 *
 * replaces: DiT.forward (diffusion_transformer.py:186-257), one call: x [n_tok][in_channels] f32 -> d_out, same shape. */
int itts_s2mel_estimator(itts_s2mel* h, const float* x, const float* const_in, const float* mods, const float* rope,
                         const int32_t* tok_seq, const int32_t* tok_t, const int32_t* seq_start, const int32_t* seq_T,
                         const int32_t* seq_len, int n_seq, int n_tok, int t_max, float* d_out, void* workspace,
                         size_t workspace_bytes, void* stream);
/* replaces: BASECFM.solve_euler (flow_matching.py:57-115; call site indextts/infer_v2_5.py:841-845).  x_state
 * [n_tok / n_branch][in_channels] f32 in/out (noise in, mel out; prompt frames are held at 0), n_branch = 2 with
 * classifier-free guidance (the estimator sees [cond ; null]) or 1 without; mods [n_steps][mods_per_step] device;
 * t_span [n_steps + 1] HOST floats; prompt_len [n_seq] device. */
int itts_s2mel_solve(itts_s2mel* h, float* x_state, const float* const_in, const float* mods, const float* rope,
                     const int32_t* tok_seq, const int32_t* tok_t, const int32_t* seq_start, const int32_t* seq_T,
                     const int32_t* seq_len, const int32_t* prompt_len, int n_seq, int n_tok, int t_max, int n_branch, int n_steps,
                     const float* t_span, float cfg_rate, void* workspace, size_t workspace_bytes, void* stream);

/* HIP-event timing of the last estimator / solve call per kernel class: [0] GEMMs on the MFMA tile kernels (algorithmic FLOPs
 * reported), [1] attention, [2] the wall span of every estimator call (element-wise time = [2] - [0] - [1]). */
int itts_s2mel_set_profiling(itts_s2mel* h, int enable);
int itts_s2mel_profile_read(itts_s2mel* h, double* ms, double* launches, double* flops);

/* Diagnostics: a 64-bit order-independent checksum of every stage's output buffer of the following estimator / solve calls, in launch order, into
 * dev_u64 (capacity 64-bit words on the handle's device; NULL clears).  Each call clears the words and restarts at entry 0; itts_s2mel_trace_count = entries
 * written by the last call, itts_s2mel_trace_label = what entry i is.  Two runs on the same inputs compared entry by entry name the first stage
 * that is not bit-stable (tools/s2mel_trace.py).  The reference has no counterpart. */
int itts_s2mel_set_trace(itts_s2mel* h, void* dev_u64, int capacity);
int itts_s2mel_trace_count(const itts_s2mel* h);
int itts_s2mel_trace_wanted(const itts_s2mel* h);   /* entries the last call asked for; > trace_count: the trace stopped at its capacity */
const char* itts_s2mel_trace_label(const itts_s2mel* h, int index);
/* ... and a COPY of the output of every traced stage whose label starts with label_prefix, packed into dev_buf in launch order (256-byte aligned;
 * stages that no longer fit are skipped): the checksums name the stage that differed between two runs, the images say which elements and how
 * (tools/s2mel_capture.py).  itts_s2mel_capture_offset = byte offset of trace entry `index` of the last call in dev_buf (-1: not captured). */
int itts_s2mel_set_capture(itts_s2mel* h, void* dev_buf, size_t bytes, const char* label_prefix);
long long itts_s2mel_capture_offset(const itts_s2mel* h, int index, size_t* bytes);

/* Dead-row elimination for the following itts_s2mel_solve calls.  The Euler step never reads the estimator's output at prompt frames
 * (flow_matching.py:107 zeroes them) and everything after the DiT's last attention is row-wise except the WaveNet's few frames of
 * context, so that part can run on the TAIL of every sequence only (frames >= prompt_len - receptive field).  Device tables of the
 * tail layout: per tail row its sequence and its frame relative to the sequence's cut; per sequence the first tail row, the tail
 * frames and the valid tail frames; tail_src [n_tail] = full-layout row of a tail row; tail_base [n_seq]: frame t of sequence s is
 * tail row tail_base[s] + t.  Caller-owned, must outlive the solves; tok_seq = NULL clears.  Results of the solve are bit-identical. */
int itts_s2mel_set_tail(itts_s2mel* h, const int32_t* tok_seq, const int32_t* tok_t, const int32_t* seq_start, const int32_t* seq_T,
                        const int32_t* seq_len, const int32_t* tail_src, const int32_t* tail_base, int n_seq, int n_tail, int t_max);

/* Seeded flow-matching noise (v13, additive: seeded flow-matching noise): the initial state of the Euler solve, written straight into the packed
 * solver rows x_rows [n_rows][channels] f32 (the rows of the FIRST CFG branch: tok_seq / tok_t [n_rows] of that branch) from a counter-based
 * generator, so that a sequence's noise depends on its own key and on nothing else -- not on the batch, its slot, the widest row or an earlier draw.
 * Device tables per sequence: prompt_len, seq_seed (u64), seq_key (u64) = stream | (chunk << 32), seq_temperature.  For frame t of sequence s and
 * channel c of C, with j = t - prompt_len[s] (the counter starts at the first frame after the prompt):
 *     j < 0:  +0.0f (prompt frames; itts_s2mel_solve holds them at 0)
 *     a = seq_key[s];  b = j * C + c
 *     x = (seq_seed[s] ^ 0x43464D4E4F495345) + 0x9E3779B97F4A7C15 * (a + 1) + 0xBF58476D1CE4E5B9 * (b + 1)            (mod 2^64)
 *     x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31      (the token sampler's finaliser; the xor
 *                                                                                        tag keeps the two streams of one seed apart)
 *     u1 = ((x >> 32) + 1) * 2^-32  in (0, 1];   u2 = (x & 0xffffffff) * 2^-32  in [0, 1)
 *     z  = sqrt(-2 ln u1) * cos(2 pi u2) * (double)seq_temperature[s]        evaluated in f64, rounded once to f32;  |z| <= 6.67 x temperature
 * replaces: z = torch.randn([1, 80, T]) * temperature of BASECFM.inference (flow_matching.py:31-55), whose draw comes from the global generator. */
int itts_s2mel_noise_forward(float* x_rows, const int32_t* tok_seq, const int32_t* tok_t, const int32_t* prompt_len,
                             const uint64_t* seq_seed, const uint64_t* seq_key, const float* seq_temperature,
                             int n_seq, int n_rows, int channels, void* stream);

/* unit-level (parity tests): one layer's RoPE + split + non-causal attention.  replaces: Attention.forward between wqkv and wo
 * (gpt_fast/model.py:262-307): qkv f32 [n_tok][3 * heads * 64] -> out [n_tok][heads * 64] in the precision's activation type. */
size_t itts_s2mel_attention_scratch_bytes(int n_tok, int n_seq, int heads, int t_max, int precision);
int itts_s2mel_attention_forward(const float* qkv, const float* rope, const int32_t* tok_seq, const int32_t* tok_t,
                                 const int32_t* seq_start, const int32_t* seq_T, const int32_t* seq_len, int n_seq, int n_tok,
                                 int t_max, int heads, int precision, void* out, void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * codes -> content features: EnhancedCodec.decode and the s2mel InterpolateRegulator, as token-major f32 ops on packed
 * sequences ([n_tok][C]; int32 tables tok_seq / tok_t per row, start / T per sequence).  The dense layers between them
 * run on itts_gemm_forward (precision 0) and itts_layernorm_forward; indextts_amd/codec.py sequences the calls.
 * ---------------------------------------------------------------------------------------------------------- */
/* replaces: FVQ.vq2emb = codebook lookup + weight-normed 1x1 out_project
 *   (indextts/codec/amphion_codec/quantize/factorized_vector_quantize.py:99-127); codes int64 [n] -> out [n][H] */
int itts_vq_project_forward(const int64_t* codes, const float* codebook, const float* w, const float* bias, float* out, int n,
                            int n_codes, int cd, int H, void* stream);
/* replaces: FVQ.forward up to the indices (eval mode; indextts/codec/amphion_codec/quantize/factorized_vector_quantize.py:52-118, reached
 *   from EnhancedCodec.quantize, indextts/codec/models.py:179-199 <- indextts/infer_v2.py:465): the weight-normed 1x1 in_project
 *   (w_in [cd][H], b_in [cd]), L2 normalisation, nearest row of the L2-normalised codebook cb_norm [n_codes][cd] (cb_sq [n_codes] = its
 *   squared row norms) by the reference's distance expression; h [n][H] -> idx int64 [n] (first index on ties); cd <= 16.
 *   itts_vq_project_forward on idx then gives the quantized features. */
int itts_vq_search_forward(const float* h, const float* w_in, const float* b_in, const float* cb_norm, const float* cb_sq, int64_t* idx,
                           int n, int H, int n_codes, int cd, void* stream);
/* replaces: F.interpolate(mode="nearest") + the im2col of a "same" zero-padded Conv1d that follows it
 *   (indextts/codec/models.py:226-229 `up`; indextts/s2mel/modules/length_regulator.py:121-125; vocos.py:770 `embed`):
 *   col [n_dst][k*C], the GEMM with the [k*C][C_out] matrix of the conv weight finishes the conv. */
int itts_tok_gather_conv_forward(const float* x, float* col, const int32_t* tok_seq, const int32_t* tok_t, const int32_t* src_start,
                                 const int32_t* src_T, const int32_t* dst_T, int n_dst, int C, int k, void* stream);
/* replaces: ConvNeXtBlock.dwconv (depthwise Conv1d k=7, vocos.py:490-491,509); w [C][k] */
int itts_tok_dwconv_forward(const float* x, const float* w, const float* b, float* y, const int32_t* tok_seq, const int32_t* tok_t,
                            const int32_t* seq_T, int n, int C, int k, void* stream);
/* replaces: nn.GELU() (erf form) of ConvNeXtBlock (vocos.py:496,515), in place */
int itts_tok_gelu_forward(float* x, size_t n, void* stream);
/* replaces: x = residual + gamma * x of ConvNeXtBlock (vocos.py:517-521): x += gamma[c] * y */
int itts_tok_scale_residual_forward(float* x, const float* y, const float* gamma, int n, int C, void* stream);
/* replaces: nn.GroupNorm(groups=1, C) + nn.Mish() of the regulator stack (length_regulator.py:52-57), in place */
int itts_tok_groupnorm_mish_forward(float* x, const float* gamma, const float* beta, const int32_t* seq_start, const int32_t* seq_T,
                                    int n_seq, int C, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * conditioning encoders: the Conformer encoder + Perceiver resampler behind UnifiedVoice.get_conditioning /
 * get_emo_conditioning / get_emovec (indextts/gpt/model_v2.py:556-593,827-838), as f32 unit ops on packed rows; the dense layers run
 * on itts_gemm_forward, LayerNorms on itts_layernorm_forward, the depthwise conv on itts_tok_dwconv_forward;
 * indextts_amd/cond.py sequences the calls.
 * ---------------------------------------------------------------------------------------------------------- */
/* replaces: softmax(Q K^T * scale + key mask) V of RelPositionMultiHeadedAttention.forward (matrix_ac + matrix_bd as ONE product of
 *   [q + u | q + v] with [k | p], indextts/gpt/conformer/attention.py:232-312,85-120) and of perceiver.py Attend.forward.
 *   q [n_q][heads][dq], k [n_k][heads][dq], v [n_k][heads][dv], out [n_q][heads][dv]; query row m attends key rows
 *   kstart[m] .. kstart[m] + klen[m] - 1 (klen 0 -> zeros, as the reference's masked softmax).  dq >= 4 of any size, 4 <= dv <= 128,
 *   both multiples of 4; anything else is ITTS_ERR_ARG. */
int itts_attention_forward(const float* q, const float* k, const float* v, float* out, const int32_t* kstart, const int32_t* klen,
                           int n_q, int heads, int dq, int dv, float scale, void* stream);
/* replaces: Wav2Vec2BertSelfAttention.forward with position_embeddings_type "relative_key" (transformers modeling_wav2vec2_bert.py, the
 *   `semantic_model` of indextts/infer_v2_5.py:171-176,282-290): scores = (q . k_j + q . dist_emb[clamp(j - qpos, -left, right) + left]) * scale
 *   over the query's key range, softmax, . V.  dist_emb [left + right + 1][dq] (shared by the heads), qpos[m] = the query's index inside
 *   its own key range; the rest as itts_attention_forward. */
int itts_attention_relkey_forward(const float* q, const float* k, const float* v, float* out, const int32_t* kstart, const int32_t* klen,
                                  const int32_t* qpos, const float* dist_emb, int left, int right, int n_q, int heads, int dq, int dv,
                                  float scale, void* stream);
/* replaces: the causal depthwise Conv1d of Wav2Vec2BertConvolutionModule (left pad k - 1, no bias: b may be NULL); layout as
 *   itts_tok_dwconv_forward */
int itts_tok_dwconv_causal_forward(const float* x, const float* w, const float* b, float* y, const int32_t* tok_seq, const int32_t* tok_t,
                                   const int32_t* seq_T, int n, int C, int k, void* stream);
/* replaces: F.glu (mode 0, conformer_encoder.py:147) / GEGLU (mode 1, perceiver.py): x [n][2C] -> out [n][C] */
int itts_tok_glu_forward(const float* x, float* out, int n, int C, int mode, void* stream);
/* replaces: ReLU (mode 0, subsampling.py:150) / SiLU (mode 1, conformer activation) / tanh (mode 2, ECAPA attention), in place */
int itts_tok_act_forward(float* x, size_t n, int mode, void* stream);
/* replaces: perceiver.py RMSNorm (F.normalize(x) * sqrt(dim) * gamma), in place */
int itts_tok_l2norm_forward(float* x, const float* gamma, int n, int C, float scale, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * CAMPPlus speaker encoder (indextts/s2mel/modules/campplus/{DTDNN,layers}.py, eval mode): BatchNorm folded
 * into the adjacent conv where it follows one, else applied by itts_tok_affine_forward; convs are row gathers + itts_gemm_forward;
 * indextts_amd/campplus.py sequences the calls.
 * ---------------------------------------------------------------------------------------------------------- */
/* replaces: get_nonlinear('batchnorm-relu') in eval mode (layers.py): out[m][c] = act(x[m][c] * scale[c] + shift[c]); x rows may be
 *   wider than C (row stride ld_x): the dense blocks' growing feature matrix */
int itts_tok_affine_forward(const float* x, int ld_x, const float* scale, const float* shift, float* out, int n, int C, int relu,
                            void* stream);
/* replaces: CAMLayer context = x.mean(-1) + seg_pooling(x, 100) (layers.py CAMLayer.forward / seg_pooling), one sequence of n rows */
int itts_tok_ctxpool_forward(const float* h, float* out, int n, int C, int seg_len, void* stream);
/* replaces: y * sigmoid(linear2(...)) of CAMLayer.forward, in place on y */
int itts_tok_gate_forward(float* y, const float* g, size_t n, void* stream);
/* replaces: AttentiveStatisticsPooling._compute_statistics (indextts/BigVGAN/ECAPA_TDNN.py:282-338, the speaker encoder inside the v1 / v1.5
 *   vocoder, models.py:191,202): per channel, weights softmax over the n frames of logit [n][C] (NULL: uniform, the global-context statistics);
 *   x [n][C] -> out [2C] = weighted mean | sqrt(max(weighted variance, eps)) */
int itts_tok_attnstats_forward(const float* x, const float* logit, float* out, int n, int C, float eps, void* stream);
/* replaces: StatsPool (mean | unbiased std over time, layers.py statistics_pooling): x [n][C] -> out [2C] */
int itts_tok_statspool_forward(const float* x, float* out, int n, int C, void* stream);
/* CAMPPlus on packed ragged rows (v13, additive: ragged prompt batch): N prompts through ONE pass of indextts_amd/campplus.py
 *   (`CAMPPlus.forward_ragged`); the reference's CAMPPlus.forward (DTDNN.py:111-116) takes a padded (B, T, 80) batch, whose zero frames would
 *   enter every pooling and every conv edge, so the pipeline calls it per prompt (indextts/infer_v2_5.py:649).  Sequences are addressed through
 *   DEVICE int32 tables (seq_start / seq_T [n_seq], as itts_tok_groupnorm_mish_forward; seq_start may leave gaps); 1 <= n_seq <= 65535, bad
 *   arguments return ITTS_ERR_ARG before any launch.
 * replaces: CAMLayer context = x.mean(-1) + seg_pooling(x, 100) (layers.py:93-110) per sequence: segments restart at each sequence's own row 0;
 *   h, out [rows][C].  The reduction order is itts_tok_ctxpool_forward's, so a sequence's rows have the bits of that entry run on them alone. */
int itts_tok_ctxpool_seq_forward(const float* h, float* out, const int32_t* seq_start, const int32_t* seq_T, int n_seq, int C, int seg_len,
                                 void* stream);
/* replaces: StatsPool (layers.py:26-37, statistics_pooling: mean | unbiased std over time) per sequence: x [rows][C] -> out [n_seq][2C].  Bits as
 *   itts_tok_statspool_forward on the sequence alone; a sequence of fewer than 2 rows is the caller's error (its out row is left untouched). */
int itts_tok_statspool_seq_forward(const float* x, float* out, const int32_t* seq_start, const int32_t* seq_T, int n_seq, int C, void* stream);
/* replaces: the im2col of a zero-padded, dilated, strided nn.Conv1d (TDNNLayer.linear, layers.py:55-61; CAMLayer.linear_local, layers.py:81-87) over
 *   packed sequences: col[m][j*C + c] = x[src_start[s] + tok_t[m]*stride + j*dilation - pad][c], s = tok_seq[m], 0 outside [0, src_T[s]).
 *   tok_seq / tok_t [n_dst]: the destination row's sequence and its frame in the OUTPUT sequence; the GEMM with the [k*C][C_out] weight finishes
 *   the conv.  A row never reads a neighbouring sequence. */
int itts_tok_gather_conv1d_seq_forward(const float* x, float* col, const int32_t* tok_seq, const int32_t* tok_t, const int32_t* src_start,
                                       const int32_t* src_T, int n_dst, int C, int k, int dilation, int stride, int pad, void* stream);
/* replaces: the im2col of the FCM head's nn.Conv2d layers (DTDNN.py:21,27; BasicResBlock, layers.py:223-246: ksize x ksize, padding (ksize-1)/2,
 *   stride (stride_f, 1)) over packed sequences.  Sequence s holds rows (f, t) at F_in*seq_start[s] + f*T_s + t, [.][C]; its output block starts at
 *   row F_out*seq_start[s], F_out = (F_in + 2*pad - ksize)/stride_f + 1, rows (f_out, t), columns (i, j, ci) [ksize*ksize*C]; 0 outside the
 *   sequence's own (F_in, T_s) rectangle.  ksize odd; C = 1 (the first conv) is supported. */
int itts_tok_gather_conv2d_seq_forward(const float* x, float* col, const int32_t* seq_start, const int32_t* seq_T, int n_seq, int F_in, int C,
                                       int ksize, int stride_f, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * prompt-audio front end (the DSP half; once per speaker prompt): resampling and the three framed-spectrum
 * feature kinds of indextts/infer_v2_5.py:626-648; indextts_amd/audio.py builds the filter banks / windows / twiddles and mirrors the
 * reference callables (mel_spectrogram, kaldi.fbank, SeamlessM4TFeatureExtractor, Resample).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t frame_length;   /* samples per frame (<= n_fft; the frame sits at the start of the zero-padded FFT buffer) */
    int32_t hop;            /* frame shift */
    int32_t n_fft;          /* power of two, 64 .. 2048 */
    int32_t n_mels;
    int32_t pad;            /* > 0: the waveform is reflect-padded by this much on both sides (mel_spectrogram: (n_fft - hop) / 2);
                               0: Kaldi snip_edges framing */
    int32_t remove_dc;      /* subtract the frame mean (Kaldi remove_dc_offset) */
    int32_t power;          /* 2: |X|^2;  1: sqrt(|X|^2 + mag_eps) */
    int32_t take_log;       /* natural log after the floor */
    int32_t layout;         /* 0: out [frames][ld_out >= n_mels];  1: out [n_mels][ld_out >= frames] */
    float preemphasis;      /* y[i] = x[i] - c x[i-1], y[0] = (1 - c) x[0];  0 = none */
    float mag_eps;
    float floor;            /* mel energies are floored here before the log (Kaldi: FLT_EPSILON; mel_spectrogram: 1e-5) */
    float scale;            /* multiplies the samples first (SeamlessM4T: 32768) */
} itts_fbank_config;
/* frames the configuration yields for n_samples (0 when shorter than one frame; < 0 on a bad configuration) */
int itts_fbank_frames(const itts_fbank_config* cfg, int n_samples);
/* replaces: mel_spectrogram (indextts/s2mel/modules/audio.py:43-83: reflect pad + torch.stft + magnitude + mel basis + log clamp),
 *   torchaudio.compliance.kaldi.fbank (indextts/infer_v2_5.py:644-647) and transformers' SeamlessM4TFeatureExtractor._extract_fbank_features
 *   (infer_v2_5.py:174,631), by configuration.  wave [B][n_samples] (row stride wave_stride), window [frame_length],
 *   twiddle [n_fft / 2][2] = (cos, -sin)(2 pi m / n_fft), mel [n_mels][n_fft / 2 + 1], out per `layout` (batch stride out_stride). */
int itts_fbank_forward(const float* wave, int B, int n_samples, int64_t wave_stride, const itts_fbank_config* cfg, const float* window,
                       const float* twiddle, const float* mel, float* out, int ld_out, int64_t out_stride, void* stream);
/* replaces: torchaudio.transforms.Resample.forward (infer_v2_5.py:627-628,642; functional._apply_sinc_resample_kernel): x [B][L_in],
 *   kernel [new_rate][2 width + orig] (rates already divided by their gcd), y [B][L_out], L_out = ceil(new_rate L_in / orig) */
int itts_resample_forward(const float* x, const float* kernel, float* y, int B, int L_in, int64_t x_stride, int L_out, int64_t y_stride,
                          int orig, int new_rate, int width, void* stream);
/* replaces: `feat - feat.mean(dim=0)` (mode 0, infer_v2_5.py:648) and the per-mel-bin normalisation of SeamlessM4TFeatureExtractor
 *   (mode 1: (x - mean) / sqrt(var(ddof) + eps)); x [n][C] -> out [n][ld_out >= C] */
int itts_tok_colnorm_forward(const float* x, float* out, int n, int C, int ld_out, int mode, int ddof, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Delivery formats (v13, additive: delivery formats): the rendered 22.05 kHz f32 rows resampled and encoded on the device
 *   (indextts_amd/output.py).  Replaces: the host tail of every pipeline entry -- `.cpu()` per segment row, torch.cat of
 *   the interval silences and `.type(torch.int16)` (indextts/infer_v2_5.py:1180-1200), the numpy cross-fade of the streaming decoder
 *   (backends/trt/pipeline/streaming.py:17-27) -- and the CPU resampler every deployment puts behind it.
 * All entries work on packed ragged sequences addressed through DEVICE int64 tables, one row per sequence (offsets in samples into the entry's
 *   buffers; 64 bits because a stream's global sample index outgrows 31 bits); 1 <= n_seq <= 65535, bad arguments return ITTS_ERR_ARG before any
 *   launch.  `max_*` is the longest sequence's length (it sizes the grid; a shorter sequence's surplus blocks exit).
 * ---------------------------------------------------------------------------------------------------------- */
#define ITTS_PCM_RESAMPLE_TILE 1024        /* consecutive outputs of one sequence a block serves */
#define ITTS_PCM_TABLE_MAX_BYTES (1 << 20) /* largest coefficient table (K * L f32) a rate pair may need */
#define ITTS_PCM_TAIL_FADE 512             /* samples of the linear fade-out that ends a stream */
#define ITTS_PCM_S16LE 0
#define ITTS_PCM_MULAW 1
#define ITTS_PCM_ALAW 2
#define ITTS_PCM_F32LE 3
int itts_pcm_resample_tile(void);
/* Rational polyphase resampler, f32 -> f32.  g = gcd(orig, new), M = orig / g, L = new / g; the prototype h[n], |n| <= H, is a Kaiser-windowed
 *   sinc at the rate orig * L (built in f64 on the host, rounded once to f32; output.py:resample_table) and
 *     y[m] = sum over i of h[m*M - i*L] * x[i],   i ascending over |m*M - i*L| <= H and over the samples that exist,
 *   ONE f32 fmaf chain from 0.f in that order: the bits of y[m] depend on neither the tile, the batch nor the sequence's place in the buffer.
 *   table [K][L], K = ceil((2H + 1) / L): table[k*L + m mod L] = h[m*M - (ceil((m*M - H) / L) + k) * L] (0 where that lies outside [-H, H]).
 *   seq [n_seq][8] = { x_start, n_buf, in_offset, y_start, out_offset, n_out, final, 0 }: x[x_start .. x_start + n_buf) holds the stream's samples
 *   in_offset .. in_offset + n_buf (the carried history and the new piece), y[y_start .. y_start + n_out) receives outputs out_offset ..; samples
 *   before the stream's start, and on a final call past its end, count as zero.  A non-final sequence must only ask for outputs whose whole
 *   support has been received, m*M + H < (in_offset + n_buf) * L (others are left unwritten).  One-shot: in_offset = out_offset = 0, final = 1,
 *   n_out = ceil(n_buf * L / M).  No sequence reads outside its own x range. */
int itts_pcm_resample_seq_forward(const float* x, float* y, const float* table, const int64_t* seq, int n_seq, int64_t max_n_out, int L, int M,
                                  int H, int K, void* stream);
/* per-sequence max |x|, NaN ignored (0 for an empty or all-NaN sequence): peak [n_seq]; seq [n_seq][2] = { x_start, n }.  Order-independent, so
 *   the result is bitwise reproducible. */
int itts_pcm_peak_seq_forward(const float* x, float* peak, const int64_t* seq, int n_seq, int64_t max_n, void* stream);
/* per-sequence gain and encoding: s = x * g (one f32 multiply, NaN -> 0), g = gain[seq], or gain[seq] / peak[seq] (an f32 division; peak 0 -> g = 1)
 *   when `peak` is given.  ITTS_PCM_S16LE: q = (int16) rintf(clamp(s * 32767, -32767, 32767)) (half to even); ITTS_PCM_MULAW / ITTS_PCM_ALAW: G.711 of
 *   that q, one byte per sample (the bytes of CPython's audioop.lin2ulaw / lin2alaw); ITTS_PCM_F32LE: clamp(s, -1, 1).
 *   seq [n_seq][4] = { x_start, n, y_start, 0 }, y_start in samples of the encoding's type. */
int itts_pcm_encode_seq_forward(const float* x, void* y, const int64_t* seq, int n_seq, int64_t max_n, int encoding, const float* gain,
                                const float* peak, void* stream);
/* replaces: RowStream.push / flush (indextts_amd/streaming.py; the reference's StreamingDecoder cross-fade) for all jobs of a render.
 *   jobs [n_jobs][12] = { tail_start, audio_start, piece_start, keep_start, n_blend, piece_len, keep_len, rest_src, keep_src, win_off, flags, 0 }:
 *     piece[j] = tails[tail_start + j] * win[win_off + n_blend + j] + audio[audio_start + j] * win[win_off + j]   for j < n_blend
 *              = src[rest_src + j - n_blend] otherwise (src = the job's audio row, or its tail row when flags & 2: a flush);
 *     flags & 1: the piece's last ITTS_PCM_TAIL_FADE samples are scaled by fade[0 .. ITTS_PCM_TAIL_FADE);
 *     keep[keep_start + j] = audio[audio_start + keep_src + j], j < keep_len: the new held-back tail.
 *   win holds np.hanning(2 n) as f32 (rising half, then falling half) for each n in use; each sample is formed in f64 and rounded once. */
int itts_pcm_stream_piece_seq_forward(const float* tails, const float* audio, float* piece, float* keep, const float* win, const float* fade,
                                      const int64_t* jobs, int n_jobs, int64_t max_len, void* stream);

/* Loudness normalisation (v13, additive: loudness): integrated loudness after ITU-R BS.1770-4 / EBU R 128 of packed ragged sequences, and the gain
 *   that brings each to a target (indextts_amd/output.py).  Replaces: the CPU loudness meter a deployment puts behind the engine.
 *   K-weighting at `rate`: the standard's two biquads by bilinear transform (a shelf: f0 1681.974450955533 Hz, G 3.999843853973347 dB,
 *   Q 0.7071752369554196; a high-pass: f0 38.13547087602444 Hz, Q 0.5003270373238773), zero initial state, a NaN sample counts as 0.
 *   hop = (rate + 5) / 10; S_k = sum of y^2 over the k-th whole sub-block of hop samples; z_j = (S_j + .. + S_j+3) / (4 hop); the blocks with
 *   -0.691 + 10 log10 z_j > -70, then those also above (the loudness of these) - 10, are kept; L = -0.691 + 10 log10 mean(z over the kept), -inf
 *   with fewer than four sub-blocks or nothing kept.  State and sums are f64 and every sum has one order, counted from the sequence's start: L
 *   has the same bits alone, in any batch and anywhere in the buffer.  No thread's work grows with the sequence beyond one 16-fma step per
 *   sub-block (the chain over the sub-block states). */
#define ITTS_PCM_LOUDNESS_MIN_RATE 4000    /* the shelf's 1682 Hz must lie under the Nyquist rate */
#define ITTS_PCM_LOUDNESS_MAX_RATE 384000
#define ITTS_PCM_LOUDNESS_WS_DOUBLES 9     /* workspace doubles per sub-block: end state (4), start state (4), S_k */
int itts_pcm_loudness_hop(int rate);
/* out [23] = stage 1 { b0, b1, b2, a1, a2 }, stage 2 { a1, a2 } (its b is [1, -2, 1]), then row-major the 4 x 4 transition of the output state
 *   (y1[-1], y1[-2], y2[-1], y2[-2]) over hop samples of zero input.  Host arithmetic only, f64. */
int itts_pcm_loudness_coefficients(int rate, double* out);
size_t itts_pcm_loudness_workspace_bytes(int64_t total_sub);
/* lufs [n_seq] (f64); peak (optional) [n_seq]: max |x| of the sequence, the value of itts_pcm_peak_seq_forward, found on the way.
 *   seq [n_seq][4] = { x_start, n, sub_start, 0 }: the sequence's floor(n / hop) sub-blocks use the workspace rows sub_start .. of total_sub (the
 *   caller lays them out, e.g. as a running sum); a row that would leave the workspace is not served and reads NaN.  max_n: the longest n.
 *   Four launches: sub-block end states from zero state, the chain of true states, the sums, the gates. */
int itts_pcm_loudness_seq_forward(const float* x, double* lufs, float* peak, const int64_t* seq, int n_seq, int64_t max_n, int rate,
                                  int64_t total_sub, void* workspace, size_t workspace_bytes, void* stream);
/* gain[i] = f32(10^((target_lufs - lufs[i]) / 20)), formed in f64 and rounded once; 1 where lufs[i] is -inf (or NaN).  has_ceiling (needs `peak`):
 *   where peak[i] > 0, gain[i] = min(gain[i], f32(10^(ceiling_dbfs / 20)) / peak[i]) (the f32 division of itts_pcm_encode_seq_forward).  The array
 *   is the `gain` of itts_pcm_encode_seq_forward (with a null `peak` there).  report (optional) [n_seq][3] = { lufs, 20 log10 gain, 20 log10
 *   min(peak * gain, 1) (NaN without `peak`) }.  -70 <= target_lufs <= 0, ceiling_dbfs <= 0. */
int itts_pcm_loudness_gain_forward(const double* lufs, const float* peak, float* gain, double* report, int n_seq, double target_lufs,
                                   int has_ceiling, double ceiling_dbfs, void* stream);

/* Look-ahead limiter and true-peak meter (v13, additive: delivery formats; indextts_amd/output.py).  Replaces: the CPU
 *   limiter and the BS.1770 Annex 2 meter a deployment puts behind a loudness stage.  All quantities are at the delivery rate.
 *   La = itts_pcm_limiter_lookahead(rate) = (rate * 5 + 500) / 1000 samples (about 5 ms; 1 <= La <= 1024 or the entry refuses), W = La + 1.
 *   True-peak signal: u[q], 0 <= q < 4N, is the output of itts_pcm_resample_seq_forward for the rate pair (1, 4) (L 4, M 1, H 96, K 49; the same
 *   table, the same fmaf chain, zero-extension outside [0, N)); u = 0 outside [0, 4N).
 *   a[n] = |f32(x[n] g0)| (sample mode), or f32(max over |p| <= 3 of |u[4n + p]| * |g0|) (true-peak mode); a NaN asks for nothing.
 *   r[n] = a[n] > c ? c / a[n] : 1 (one f32 division; 1 outside [0, N)), m[j] = min r[j .. j + La],
 *   G[n] = 1 - (fmaf chain from 0.f over k = 0 .. La ascending of w[k] * (1 - m[n - k])), z[n] = clamp(f32(x[n] g0) * G[n], -c, c), NaN -> 0.
 *   Where no sample within +-La exceeds c, z[n] has the bits of f32(x[n] g0); in sample mode |z[n]| <= c holds exactly.
 *   Reach R = La (+ 24 in true-peak mode): a non-final sequence may only ask for outputs n with n + R < in_offset + n_buf, and its buffer must
 *   start at or before max(0, out_offset - R); a stream's pieces then concatenate to the bits of the one-shot call. */
#define ITTS_PCM_LIMITER_TILE 1024           /* consecutive outputs of one sequence a block serves */
#define ITTS_PCM_LIMITER_MAX_LOOKAHEAD 1024
int itts_pcm_limiter_lookahead(int rate);
/* peak[i] = max |u| of sequence i (NaN ignored, 0 for an empty sequence); seq [n_seq][2] = { x_start, n }; table4 = phase_table(1, 4).  The bits
 *   are those of itts_pcm_peak_seq_forward over the (1, 4) resampler's output, which is never written. */
int itts_pcm_truepeak_seq_forward(const float* x, float* peak, const float* table4, const int64_t* seq, int n_seq, int64_t max_n, void* stream);
/* seq [n_seq][8] = { x_start, n_buf, in_offset, y_start, out_offset, n_out, final, 0 } -- the resampler's row, same meaning;
 *   window [lookahead + 1]: w[k] proportional to sin^2(pi (k + 1) / (La + 2)), summing to 1; table4 null: sample mode; gain [n_seq]: g0;
 *   0 < ceiling <= 1: c; stats optional [n_seq][2] = { min G, max |z| } over the outputs written (integer atomics on the float bits, exact). */
int itts_pcm_limiter_seq_forward(const float* x, float* z, const float* window, const float* table4, const int64_t* seq, int n_seq,
                                 int64_t max_n_out, int lookahead, const float* gain, float ceiling, float* stats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INDEXTTS_HIP_H */
