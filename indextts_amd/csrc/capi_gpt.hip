// C-ABI entry points for the GPT speech-token decoder (see include/indextts_hip.h for the reference call sites).
#include <math.h>
#include <stddef.h>
#include <string.h>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/indextts_hip.h"
#include "gpt_kernels.h"

// ---- host-side weight packing ----------------------------------------------------------------------------------
extern "C" size_t itts_packed_gemm_bytes(int K, int N, int precision) {
    if (precision == PREC_F32X3) return (size_t)((N + 15) / 16) * (K / 32) * 3 * 64 * 16;       // three bf16 planes per 32-deep k-block
    const int KB = precision == PREC_BF16 ? 32 : 16;
    return (size_t)((N + 15) / 16) * (K / KB) * 64 * 16;
}

// w: [K][N] row-major (HF Conv1D) when transposed == 0, [N][K] (nn.Linear) when transposed != 0
extern "C" int itts_pack_gemm_weight(const float* w, int K, int N, int transposed, int precision, void* out) {
    const int KB = precision == PREC_F32 ? 16 : 32;
    if (!w || !out || K <= 0 || N <= 0 || K % KB) {
        itts_set_error("pack_gemm: K=%d must be a positive multiple of %d", K, KB);
        return ITTS_ERR_ARG;
    }
    if (precision != PREC_F32 && precision != PREC_BF16 && precision != PREC_F32X3) { itts_set_error("pack_gemm: precision %d", precision); return ITTS_ERR_ARG; }
    const int ntiles = (N + 15) / 16, nkb = K / KB, per = KB / 4;   // per = k elements per lane
    if (precision == PREC_F32X3) {
        // [N/16][K/32][3 planes][64 lanes][8 bf16]: x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) (exact: 24 bits);
        // lane (kg, n) element j holds k = 32 kb + 4 kg + j (j < 4) or 32 kb + 16 + 4 kg + (j - 4): the two 16-byte pieces of the
        // f32 activation row that gemm_x3_kernel's lane reads
        auto b2f = [](uint16_t b) { uint32_t u = (uint32_t)b << 16; float f; memcpy(&f, &u, 4); return f; };
        for (int nt = 0; nt < ntiles; ++nt)
            for (int kb = 0; kb < nkb; ++kb)
                for (int lane = 0; lane < 64; ++lane) {
                    const int n = nt * 16 + (lane & 15), kg = lane >> 4;
                    for (int j = 0; j < 8; ++j) {
                        const int k = kb * 32 + (j < 4 ? 4 * kg + j : 16 + 4 * kg + (j - 4));
                        float v = 0.f;
                        if (n < N) v = transposed ? w[(size_t)n * K + k] : w[(size_t)k * N + n];
                        const uint16_t h = host_f32_to_bf16(v);
                        const float r1 = v - b2f(h);
                        const uint16_t m = host_f32_to_bf16(r1);
                        const float r2 = r1 - b2f(m);
                        const uint16_t l = host_f32_to_bf16(r2);
                        const size_t blk = ((size_t)nt * nkb + kb) * 3;
                        ((u16*)out)[((blk + 0) * 64 + lane) * 8 + j] = h;
                        ((u16*)out)[((blk + 1) * 64 + lane) * 8 + j] = m;
                        ((u16*)out)[((blk + 2) * 64 + lane) * 8 + j] = l;
                    }
                }
        return ITTS_OK;
    }
    for (int nt = 0; nt < ntiles; ++nt)
        for (int kb = 0; kb < nkb; ++kb)
            for (int lane = 0; lane < 64; ++lane) {
                const int n = nt * 16 + (lane & 15);
                const size_t base = (((size_t)nt * nkb + kb) * 64 + lane);
                for (int j = 0; j < per; ++j) {
                    const int k = kb * KB + (lane >> 4) * per + j;
                    float v = 0.f;
                    if (n < N) v = transposed ? w[(size_t)n * K + k] : w[(size_t)k * N + n];
                    if (precision == PREC_BF16) ((u16*)out)[base * 8 + j] = host_f32_to_bf16(v);
                    else ((float*)out)[base * 4 + j] = v;
                }
            }
    return ITTS_OK;
}

// ---- model object ----------------------------------------------------------------------------------------------
struct GLayer {
    float *ln1_g = 0, *ln1_b = 0, *ln2_g = 0, *ln2_b = 0;
    void *w_qkv = 0, *w_proj = 0, *w_fc = 0, *w_fc2 = 0;
    float *b_qkv = 0, *b_proj = 0, *b_fc = 0, *b_fc2 = 0;
};

struct itts_gpt {
    itts_gpt_config cfg;
    std::vector<GLayer> layers;
    float *lnf_g = 0, *lnf_b = 0, *fn_g = 0, *fn_b = 0;
    void* w_head = 0;
    float* b_head = 0;
    float *mel_emb = 0, *mel_pos = 0;
    std::vector<void*> owned;
    bool finalized = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_t0 = nullptr, ev_t1 = nullptr, ev_t2 = nullptr;
    int* host_flag = nullptr;          // pinned
    unsigned char* host_fin = nullptr; // pinned, capacity fin_cap
    int fin_cap = 0;
    float last_prefill_ms = 0, last_decode_ms = 0;
    int last_steps = 0;
    int device = -1;                   // device current at itts_gpt_create: owns weights, stream, events
    // Instantiated decode-step graphs, reused across generate calls.  A graph bakes in every pointer and scalar of the step's
    // 171 launches, so the key is everything those derive from: workspace base, carve shape (rows, bucketed prompt length,
    // cache stride), output / uniforms pointers, the generation parameters.  Small LRU (a serving process sees a handful of
    // (batch, prompt-bucket) shapes).
    struct GraphEntry {
        const void* base; const void* tokens; const void* uniforms; const void* aux0; const void* aux1; const void* aux2; const void* aux3;
        const void* filt;                    // the logits-filter record the step reads (null: none installed) -- filled by step_graph
        int filt_is_table;                   // ... and whether that address is the per-slot table's (the step then indexes it by slot)
        const void* scores0; const void* scores1;   // the token-score arrays the step writes (null: none installed) -- filled by step_graph
        const void* align_out; const void* align_span; unsigned align_epoch;   // the alignment export the step carries (itts_gpt_set_alignment): its
                                             // arrays, and an epoch that changes with every install -- the pair list decides which launches a step HAS
        int nseq, nb, Sb, Tmax, S;           // S: only where the step bakes the exact prompt length in (beam kernels), else 0
        unsigned opt_epoch;                  // itts_opt_epoch() at capture: a graph bakes the kernel choices of the options in
        itts_gen_params gp;
        hipGraphExec_t exec;
        unsigned long long stamp;
    };
    std::vector<GraphEntry> graphs;
    unsigned long long graph_clock = 0;
    int graph_hits = 0, graph_captures = 0;
    // The decode loop suspended on this handle between two calls (itts_gpt_generate_chunk / itts_gpt_generate_beam_chunk and the admissions into
    // them), its state on the device in `ws`.  ONE record: a first (non-resume) call of any generate entry ends whatever was suspended once its
    // own checks have passed, and a resume or an admission needs the record of its own kind -- a loop whose workspace another call has
    // overwritten is refused (ITTS_ERR_STATE), never decoded from.
    struct Suspended {
        enum Kind { NONE, ROWS, BEAM_GROUPS } kind = NONE;
        const void* ws = nullptr;              // the caller's workspace pointer
        int n_utts = 0, nb = 1, S = 0;         // utterances (rows / beam groups), beams per utterance, prompt length of the first call
        itts_gen_params gp{};
        // what the loop's captured step bakes in beside the shapes above: a row admission must be given the same ones
        const void* codes = nullptr; const void* uniforms = nullptr;
        int steps = 0;                         // tokens / beam steps generated so far
        bool admitted = false;                 // a row / group has been admitted into the loop: the decode step reads the per-row position shifts
        // beam groups: per group (= utterance slot) the session step of its own step 0 and its cap on own steps (host mirrors of the device tables)
        std::vector<int> step0, cap;
    } susp;
    // row compaction of a ragged decode batch (itts_gpt_set_compaction): finished utterances leave the running batch in steps of
    // `compact_gran` rows, so the step's cost follows the live rows.  cur_slots[i] = utterance carried by dense row i.
    bool compact = true;
    int compact_gran = 8;
    std::vector<int> cur_slots;
    bool cur_mapped = false;
    int* host_map = nullptr;               // pinned [2][map_cap]: new slot map | gather sources
    int map_cap = 0;
    long long last_row_steps = 0;          // sum over the decode steps of the rows that step ran (itts_gpt_compaction_stats)
    int last_compactions = 0;
    const int32_t* row_limits = nullptr;   // device [row_limits_n] per-utterance token caps for the next generate calls, or null
    int row_limits_n = 0;
    const itts_row_sampling* row_sampling = nullptr;   // device [row_sampling_n] per-slot sampling settings (itts_gpt_set_row_sampling), or null
    int row_sampling_n = 0;
    const itts_group_sampling* group_sampling = nullptr;   // device [group_sampling_n] per-group settings of the beam kernels (itts_gpt_set_group_sampling), or null
    int group_sampling_n = 0;
    int chunk_return_finished = 0;         // itts_gpt_set_chunk_return: a chunk call returns at a flag check once that many utterances have finished
    // Logits filters (itts_gpt_set_logits_filters): the device record the selection kernels read, the [V] suppress mask and the decay table --
    // allocated once at the first installation, at addresses that never change (a captured step bakes the record's address in, not its contents).
    LogitsFilters* filt_dev = nullptr;
    unsigned char* filt_mask = nullptr;
    float* filt_decay = nullptr;
    int filt_decay_cap = 0;
    bool filt_on = false;
    int filt_ngram = 0;                    // host mirror: the beam entries refuse an installed n-gram filter
    // Per-slot filter table (itts_gpt_set_row_filters): ftab_n records (0: none installed) with their mask / decay rows; while installed it
    // rules for every slot and the call-wide record is not read
    LogitsFilters* ftab_dev = nullptr;
    unsigned char* ftab_mask = nullptr;      // [ftab_cap][V]
    float* ftab_decay = nullptr;             // [ftab_cap][n_mel_pos + 1]
    int ftab_cap = 0, ftab_n = 0;
    std::vector<int> ftab_ngram;             // host mirror of the entries' n-gram sizes: the beam entries refuse an installed n-gram filter
    const LogitsFilters* filt_table() const { return ftab_n ? ftab_dev : nullptr; }
    const LogitsFilters* filt() const { return (filt_on && !ftab_n) ? filt_dev : nullptr; }
    // Token scores (itts_gpt_set_token_scores): caller-owned device arrays [scores_n][scores_max_new] the sampler writes next to the tokens
    float* logp_model = nullptr;
    float* logp_sampled = nullptr;
    int scores_n = 0, scores_max_new = 0;
    // Alignment export (itts_gpt_set_alignment): caller-owned device span table [align_n][2] and output [align_n][align_max_new][n_pairs][text_cap]
    const int32_t* align_span = nullptr;
    float* align_out = nullptr;
    int align_pairs[ALIGN_MAX_PAIRS][2] = {};       // (layer, head), in the caller's order: index k of the output
    int align_n_pairs = 0, align_n = 0, align_max_new = 0, align_text_cap = 0;
    unsigned align_epoch = 0;                       // part of the decode graph's key: bumped by an install whose pair list or sizes differ from
    int align_keyed[4 + 2 * ALIGN_MAX_PAIRS] = {};  // those of the install before it ({n_pairs, n, max_new, text_cap, pairs}; kept over an uninstall)
    // Code prefix (itts_gpt_set_code_prefix): caller-owned device codes [prefix_n][prefix_width], the host's copy of the lengths, the position
    // offset of the prefix embeddings and the positions per ingest pass; what the last ingest did (itts_gpt_last_prefix)
    const int64_t* prefix_codes = nullptr;
    std::vector<int> prefix_lens;
    int prefix_n = 0, prefix_width = 0, prefix_pos_offset = 0, prefix_chunk = 0;
    int last_prefix_chunks = 0, last_prefix_max = 0;
};
#define GRAPH_CACHE_MAX 24        // a ragged batch replays one graph per live-row bucket (8 at the bench shape) beside the callers' own shapes
// prompt lengths are bucketed to multiples of 32 for the workspace carve and the cache stride, so that prompts of nearby lengths
// share one workspace layout and therefore one decode graph
static inline int s_bucket(int S) { return (S + 31) & ~31; }

static hipGraphExec_t graph_lookup(itts_gpt* h, const itts_gpt::GraphEntry& k) {
    for (auto& e : h->graphs)
        if (e.base == k.base && e.tokens == k.tokens && e.uniforms == k.uniforms && e.aux0 == k.aux0 && e.aux1 == k.aux1 && e.aux2 == k.aux2 && e.aux3 == k.aux3 &&
            e.filt == k.filt && e.filt_is_table == k.filt_is_table && e.scores0 == k.scores0 && e.scores1 == k.scores1 && e.align_out == k.align_out && e.align_span == k.align_span && e.align_epoch == k.align_epoch && e.nseq == k.nseq && e.nb == k.nb && e.Sb == k.Sb && e.Tmax == k.Tmax && e.S == k.S && e.opt_epoch == k.opt_epoch && memcmp(&e.gp, &k.gp, sizeof(k.gp)) == 0) {
            e.stamp = ++h->graph_clock;
            ++h->graph_hits;
            return e.exec;
        }
    return nullptr;
}
static void graph_insert(itts_gpt* h, itts_gpt::GraphEntry k, hipGraphExec_t exec) {
    k.exec = exec;
    k.stamp = ++h->graph_clock;
    ++h->graph_captures;
    if ((int)h->graphs.size() >= GRAPH_CACHE_MAX) {
        size_t old = 0;
        for (size_t i = 1; i < h->graphs.size(); ++i) if (h->graphs[i].stamp < h->graphs[old].stamp) old = i;
        (void)hipGraphExecDestroy(h->graphs[old].exec);
        h->graphs[old] = k;
    } else {
        h->graphs.push_back(k);
    }
}

static int g_upload(itts_gpt* h, const void* host, size_t bytes, void** dst) {
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, bytes));
    h->owned.push_back(d);
    HIP_TRY(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
    *dst = d;
    return ITTS_OK;
}

extern "C" int itts_gpt_create(const itts_gpt_config* cfg, itts_gpt** out) {
    if (!cfg || !out) { itts_set_error("gpt_create: null"); return ITTS_ERR_ARG; }
    const itts_gpt_config& c = *cfg;
    const int KB = c.precision == PREC_BF16 ? 32 : 16;
    if (c.layers < 1 || c.heads < 1 || c.model_dim != c.heads * 64 || c.model_dim % KB || c.vocab < 2 ||
        (c.precision != PREC_F32 && c.precision != PREC_BF16) || c.n_mel_pos < 3) {
        itts_set_error("gpt_create: unsupported config (layers=%d dim=%d heads=%d: head_dim must be 64; vocab=%d prec=%d)",
                       c.layers, c.model_dim, c.heads, c.vocab, c.precision);
        return ITTS_ERR_ARG;
    }
    itts_gpt* h = new itts_gpt();
    h->cfg = c;
    h->device = itts_current_device();
    h->layers.resize(c.layers);
    *out = h;
    return ITTS_OK;
}

extern "C" int itts_gpt_device(const itts_gpt* h) { return h ? h->device : -1; }

void itts_gpt_latent_drop_handle(itts_gpt* h);     // (latent sessions, below)
extern "C" void itts_gpt_destroy(itts_gpt* h) {
    if (!h) return;
    itts_gpt_latent_drop_handle(h);
    ItDevGuard dg(h->device);
    for (auto& e : h->graphs) (void)hipGraphExecDestroy(e.exec);
    for (void* p : h->owned) (void)hipFree(p);
    if (h->host_flag) (void)hipHostFree(h->host_flag);
    if (h->host_fin) (void)hipHostFree(h->host_fin);
    if (h->host_map) (void)hipHostFree(h->host_map);
    if (h->ev_in) { (void)hipEventDestroy(h->ev_in); (void)hipEventDestroy(h->ev_out); (void)hipEventDestroy(h->ev_t0);
                    (void)hipEventDestroy(h->ev_t1); (void)hipEventDestroy(h->ev_t2); }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

static bool g_eat(const char*& s, const char* lit) {
    size_t n = strlen(lit);
    if (strncmp(s, lit, n) == 0) { s += n; return true; }
    return false;
}

static size_t numel(const int64_t* shape, int ndim) {
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    return n;
}

static int load_vec(itts_gpt* h, const float* data, const int64_t* shape, int ndim, size_t want, float** dst, const char* name) {
    if (numel(shape, ndim) != want) { itts_set_error("%s: expected %zu elements, got %zu", name, want, numel(shape, ndim)); return ITTS_ERR_ARG; }
    return g_upload(h, data, want * sizeof(float), (void**)dst);
}

static int load_mat(itts_gpt* h, const float* data, const int64_t* shape, int ndim, int K, int N, int transposed, void** dst,
                    const char* name) {
    const int64_t d0 = transposed ? N : K, d1 = transposed ? K : N;
    if (ndim != 2 || shape[0] != d0 || shape[1] != d1) {
        itts_set_error("%s: expected shape [%lld,%lld]", name, (long long)d0, (long long)d1);
        return ITTS_ERR_ARG;
    }
    std::vector<char> pk(itts_packed_gemm_bytes(K, N, h->cfg.precision));
    int rc = itts_pack_gemm_weight(data, K, N, transposed, h->cfg.precision, pk.data());
    if (rc) return rc;
    return g_upload(h, pk.data(), pk.size(), dst);
}

// Reference state-dict names: gpt.h.{i}.{ln_1,attn.c_attn,attn.c_proj,ln_2,mlp.c_fc,mlp.c_proj}.{weight,bias},
// gpt.ln_f, final_norm, mel_head, mel_embedding.weight, mel_pos_embedding.emb.weight.  HF Conv1D weights are [in, out].
extern "C" int itts_gpt_load_tensor(itts_gpt* h, const char* name, const float* data, const int64_t* shape, int ndim) {
    if (!h || !name || !data || !shape || ndim < 1 || ndim > 2) { itts_set_error("gpt_load_tensor: bad args"); return ITTS_ERR_ARG; }
    ItDevGuard dg(h->device);
    const itts_gpt_config& c = h->cfg;
    const int D = c.model_dim;
    const char* s = name;
    h->finalized = false;
    if (g_eat(s, "gpt.h.")) {
        int i = 0;
        if (*s < '0' || *s > '9') { itts_set_error("bad name %s", name); return ITTS_ERR_ARG; }
        while (*s >= '0' && *s <= '9') i = i * 10 + (*s++ - '0');
        if (i >= c.layers || !g_eat(s, ".")) { itts_set_error("bad layer index in %s", name); return ITTS_ERR_ARG; }
        GLayer& L = h->layers[i];
        if (!strcmp(s, "ln_1.weight")) return load_vec(h, data, shape, ndim, D, &L.ln1_g, name);
        if (!strcmp(s, "ln_1.bias")) return load_vec(h, data, shape, ndim, D, &L.ln1_b, name);
        if (!strcmp(s, "ln_2.weight")) return load_vec(h, data, shape, ndim, D, &L.ln2_g, name);
        if (!strcmp(s, "ln_2.bias")) return load_vec(h, data, shape, ndim, D, &L.ln2_b, name);
        if (!strcmp(s, "attn.c_attn.weight")) return load_mat(h, data, shape, ndim, D, 3 * D, 0, &L.w_qkv, name);
        if (!strcmp(s, "attn.c_attn.bias")) return load_vec(h, data, shape, ndim, 3 * D, &L.b_qkv, name);
        if (!strcmp(s, "attn.c_proj.weight")) return load_mat(h, data, shape, ndim, D, D, 0, &L.w_proj, name);
        if (!strcmp(s, "attn.c_proj.bias")) return load_vec(h, data, shape, ndim, D, &L.b_proj, name);
        if (!strcmp(s, "mlp.c_fc.weight")) return load_mat(h, data, shape, ndim, D, 4 * D, 0, &L.w_fc, name);
        if (!strcmp(s, "mlp.c_fc.bias")) return load_vec(h, data, shape, ndim, 4 * D, &L.b_fc, name);
        if (!strcmp(s, "mlp.c_proj.weight")) return load_mat(h, data, shape, ndim, 4 * D, D, 0, &L.w_fc2, name);
        if (!strcmp(s, "mlp.c_proj.bias")) return load_vec(h, data, shape, ndim, D, &L.b_fc2, name);
    }
    if (!strcmp(name, "gpt.ln_f.weight")) return load_vec(h, data, shape, ndim, D, &h->lnf_g, name);
    if (!strcmp(name, "gpt.ln_f.bias")) return load_vec(h, data, shape, ndim, D, &h->lnf_b, name);
    if (!strcmp(name, "final_norm.weight")) return load_vec(h, data, shape, ndim, D, &h->fn_g, name);
    if (!strcmp(name, "final_norm.bias")) return load_vec(h, data, shape, ndim, D, &h->fn_b, name);
    if (!strcmp(name, "mel_head.weight")) return load_mat(h, data, shape, ndim, D, c.vocab, 1, &h->w_head, name);
    if (!strcmp(name, "mel_head.bias")) return load_vec(h, data, shape, ndim, c.vocab, &h->b_head, name);
    if (!strcmp(name, "mel_embedding.weight")) return load_vec(h, data, shape, ndim, (size_t)c.vocab * D, &h->mel_emb, name);
    if (!strcmp(name, "mel_pos_embedding.emb.weight")) return load_vec(h, data, shape, ndim, (size_t)c.n_mel_pos * D, &h->mel_pos, name);
    itts_set_error("gpt_load_tensor: unrecognised tensor name '%s'", name);
    return ITTS_ERR_ARG;
}

extern "C" int itts_gpt_finalize(itts_gpt* h) {
    if (!h) { itts_set_error("gpt_finalize: null"); return ITTS_ERR_ARG; }
    ItDevGuard dg(h->device);
    std::string missing;
    for (size_t i = 0; i < h->layers.size(); ++i) {
        const GLayer& L = h->layers[i];
        if (!L.ln1_g || !L.ln1_b || !L.ln2_g || !L.ln2_b || !L.w_qkv || !L.w_proj || !L.w_fc || !L.w_fc2 || !L.b_qkv || !L.b_proj ||
            !L.b_fc || !L.b_fc2)
            missing += "gpt.h." + std::to_string(i) + ".* ";
    }
    if (!h->lnf_g || !h->lnf_b) missing += "gpt.ln_f ";
    if (!h->fn_g || !h->fn_b) missing += "final_norm ";
    if (!h->w_head || !h->b_head) missing += "mel_head ";
    if (!h->mel_emb) missing += "mel_embedding.weight ";
    if (!h->mel_pos) missing += "mel_pos_embedding.emb.weight ";
    if (!missing.empty()) { itts_set_error("gpt_finalize: missing tensors: %s", missing.c_str()); return ITTS_ERR_STATE; }
    if (!h->stream) {
        HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
        HIP_TRY(hipEventCreate(&h->ev_t0));
        HIP_TRY(hipEventCreate(&h->ev_t1));
        HIP_TRY(hipEventCreate(&h->ev_t2));
        HIP_TRY(hipHostMalloc((void**)&h->host_flag, 64, hipHostMallocDefault));
    }
    h->finalized = true;
    return ITTS_OK;
}

// caller tensors must live on the device that owns the engine (weights, stream): a mismatch would fault or go through
// silent peer access
static int check_same_device(const itts_gpt* h, const void* in, const void* ws, const char* who) {
    const int di = itts_ptr_device(in), dw = itts_ptr_device(ws);
    if ((di >= 0 && di != h->device) || (dw >= 0 && dw != h->device)) {
        itts_set_error("%s: tensors are on device %d/%d but the engine was created on device %d", who, di, dw, h->device);
        return ITTS_ERR_ARG;
    }
    return ITTS_OK;
}

// ---- workspace -------------------------------------------------------------------------------------------------
static size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

struct GptWs {
    char *kc, *vc;      // [L][nseq][H][Tmax][64] cache dtype
    float* x;           // [rows][D]
    float* x2;          // [16][D] second residual buffer of the LayerNorm-fused decode GEMMs (1-16 rows; run_layers alternates x / x2)
    char* hbuf;         // [rows][D] act
    float* qbuf;        // [rows][D]
    char* attn;         // [rows][D] act
    char* fc;           // [rows][4D] act
    float* partial;     // [4][nseq][D]
    char* hlast;        // [nseq][D] act
    float* logits;      // [nseq][V]
    unsigned char* seen;     // [nseq][V]
    unsigned char* finished; // [nseq]
    int* state;         // [0] step, [1] pos
    int* pad;           // [nseq]
    int* pen_ids;       // [16]
    int* slot_map;      // [nseq] dense row -> utterance (row compaction; unused while the batch is uncompacted)
    int* gather_src;    // [nseq] compaction: the old dense row each new dense row is taken from
    int* row_step0;     // [nseq] the step at which the utterance joined the running batch (itts_gpt_admit_rows; 0 otherwise)
    int* row_shift;     // [nseq] batch position counter - the cache row's own position (0 for the rows of the first call; admitted rows keep their
                        // keys at their own positions 0 .. prompt + generated, whatever the running batch's counter says)
    // beam search (nb > 1)
    unsigned char* seen2;    // second seen buffer
    int* row_map[2];         // [nseq][Tmax]
    float* beam_scores; float* next_scores; int* next_tokens; int* next_indices;   // [nseq]
    BeamHyp* hyps; int* n_hyps; float* worst; unsigned char* done;                 // per utterance
    int* grp_cap;                                                                   // [B] per-group cap on own steps (beam sessions)
    int* hist_tok; int* hist_par;                                                   // [max_new][nseq]
    int* surv_idx; float* surv_val; int* surv_n;                                    // [nseq][64], [nseq]
    size_t total;
    size_t layer_cache_bytes;
};

static GptWs carve(const itts_gpt_config& c, char* base, int nseq, int S, int Tmax, int nb = 1) {
    GptWs w;
    const size_t esz = c.precision == PREC_BF16 ? 2 : 4;
    const size_t D = c.model_dim, rows = (size_t)nseq * S;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += a256(bytes); return p; };
    w.layer_cache_bytes = a256((size_t)nseq * D * Tmax * esz);
    w.kc = take(w.layer_cache_bytes * c.layers);
    w.vc = take(w.layer_cache_bytes * c.layers);
    w.x = (float*)take(rows * D * 4);
    w.x2 = (float*)take((size_t)16 * D * 4);
    w.hbuf = take(rows * D * esz);
    w.qbuf = (float*)take(rows * D * 4);
    w.attn = take(rows * D * esz);
    w.fc = take(rows * 4 * D * esz);
    w.partial = (float*)take((size_t)4 * nseq * D * 4);
    w.hlast = take((size_t)nseq * D * esz);
    w.logits = (float*)take((size_t)nseq * c.vocab * 4);
    w.seen = (unsigned char*)take((size_t)nseq * c.vocab);
    w.finished = (unsigned char*)take(nseq);
    w.state = (int*)take(64);
    w.pad = (int*)take((size_t)nseq * 4);
    w.pen_ids = (int*)take(64);
    w.slot_map = (int*)take((size_t)nseq * 4);
    w.gather_src = (int*)take((size_t)nseq * 4);
    w.row_step0 = (int*)take((size_t)nseq * 4);
    w.row_shift = (int*)take((size_t)nseq * 4);
    w.seen2 = nullptr; w.row_map[0] = w.row_map[1] = nullptr;
    if (nb > 1) {
        const int B = nseq / nb, max_new = Tmax - S;
        w.seen2 = (unsigned char*)take((size_t)nseq * c.vocab);
        w.row_map[0] = (int*)take((size_t)nseq * Tmax * 4);
        w.row_map[1] = (int*)take((size_t)nseq * Tmax * 4);
        w.beam_scores = (float*)take((size_t)nseq * 4);
        w.next_scores = (float*)take((size_t)nseq * 4);
        w.next_tokens = (int*)take((size_t)nseq * 4);
        w.next_indices = (int*)take((size_t)nseq * 4);
        w.hyps = (BeamHyp*)take((size_t)B * BEAM_MAX * sizeof(BeamHyp));
        w.n_hyps = (int*)take((size_t)B * 4);
        w.worst = (float*)take((size_t)B * 4);
        w.done = (unsigned char*)take((size_t)B);
        w.hist_tok = (int*)take((size_t)max_new * nseq * 4);
        w.hist_par = (int*)take((size_t)max_new * nseq * 4);
        w.surv_idx = (int*)take((size_t)nseq * 64 * 4);
        w.surv_val = (float*)take((size_t)nseq * 64 * 4);
        w.surv_n = (int*)take((size_t)nseq * 4);
        w.grp_cap = (int*)take((size_t)B * 4);
    }
    w.total = off + 256;
    return w;
}

extern "C" size_t itts_gpt_workspace_bytes(const itts_gpt* h, int nseq, int S, int Tmax) {
    if (!h || nseq <= 0 || S <= 0 || Tmax < S) return 0;
    return carve(h->cfg, nullptr, nseq, s_bucket(S), Tmax + s_bucket(S) - S).total + 256;
}
extern "C" size_t itts_gpt_beam_workspace_bytes(const itts_gpt* h, int n_utts, int num_beams, int S, int Tmax) {
    if (!h || n_utts <= 0 || num_beams < 2 || num_beams > BEAM_MAX || S <= 0 || Tmax <= S) return 0;
    return carve(h->cfg, nullptr, n_utts * num_beams, s_bucket(S), Tmax + s_bucket(S) - S, num_beams).total + 256;
}

// ---- small state kernels ---------------------------------------------------------------------------------------
__global__ void set_state_kernel(int* state, int step, int pos) { state[0] = step; state[1] = pos; state[2] = 0; }
__global__ void set_seed_kernel(int* state, unsigned long long seed) { *(unsigned long long*)(state + 4) = seed; }   // state[4..5]
__global__ void set_filter_prompt_kernel(LogitsFilters* f, int S) { f->prompt_len = S; }
__global__ void set_filter_table_prompt_kernel(LogitsFilters* f, int n, int S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) f[i].prompt_len = S;
}
__global__ void fill_i64_kernel(long long* p, long long v, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}
__global__ void mark_seen_kernel(unsigned char* seen, const int* ids, int n_ids, int V) {
    const int b = blockIdx.x;
    if ((int)threadIdx.x < n_ids) {
        const int id = ids[threadIdx.x];
        if (id >= 0 && id < V) seen[(size_t)b * V + id] = 1;
    }
}

// row compaction: x_new[i] = x_old[src[i]] through a scratch copy (src[i] >= i, but rows are moved by independent blocks)
__global__ void gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ src, float* __restrict__ tmp, int D) {
    const int i = blockIdx.x;
    const float* s = x + (size_t)src[i] * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) tmp[(size_t)i * D + c] = s[c];
}
__global__ void copy_rows_kernel(const float* __restrict__ tmp, float* __restrict__ x, int D) {
    const int i = blockIdx.x;
    for (int c = threadIdx.x; c < D; c += blockDim.x) x[(size_t)i * D + c] = tmp[(size_t)i * D + c];
}

// ---- one transformer pass --------------------------------------------------------------------------------------
// rows = nseq*S new positions (S = 1 for a decode step).  prefill: direct residual epilogues + big-tile GEMMs;
// decode: split-K partials reduced inside the next LayerNorm kernel.
// x_cur (optional out): the buffer that holds the residual stream after the pass (w.x, or w.x2 when the LayerNorm-fused decode GEMMs ran)
// The alignment export of a many-query pass (itts_gpt_rescore): after each listed layer's QKV GEMM, attn_align_mq over the queries
// q_row0 .. q_row0 + nq - 1 of every sequence's S rows, whose first sits at cache index *qpos_ptr; rows row0 .. of `out`
struct MqAlign {
    const int (*pairs)[2]; int n_pairs;
    const int* span; float* out; int out_rows, text_cap;
    const int* q_len; const int* qpos_ptr;
    int q_row0, nq, row0;
};

static int run_layers(itts_gpt* h, const GptWs& w, int nseq, int S, int Tmax, bool prefill, const int* pos_ptr, const int* pad,
                      bool* pending, hipStream_t st, bool beam = false, int seq_mul = 1, const int* seq_map = nullptr, float** x_cur = nullptr,
                      const int* pos_shift = nullptr, const MqAlign* mq = nullptr) {
    const itts_gpt_config& c = h->cfg;
    const int D = c.model_dim, prec = c.precision, rows = nseq * S;
    int rc;
    const float* pend_bias = nullptr;   // bias of a GEMM whose partials are pending reduction
    // Decode steps of 1-8 rows (one utterance, its beams, the 8-utterance shard of an 8-GPU run): the two LayerNorm launches of a layer are fused into
    // the GEMMs that consume them (gemm_decode_ln_kernel at 1-4 rows, gemm_decode_lnw_kernel at 5-8: same arithmetic, bitwise the same results; option
    // decode_fuse_ln = 0 is the A/B switch).  The fused kernel's block 0 writes the updated residual to the OTHER buffer (its sibling blocks still read
    // the current one): cur / alt alternate.  Measured (profiles/r04a, r04h; ms per token at 560 tokens, fused / separate): 1 row 0.776 / 0.915, 4 rows
    // 0.874 / 0.957, 5 rows 0.935 / 0.963, 8 rows 0.977 / 0.986 -- and 12 rows 1.110 / 1.016, 16 rows 1.294 / 1.099: every block repeats the LayerNorm
    // of every row, which outgrows the launch it removes.  decode_fuse_ln = 2 keeps the 9-16-row form reachable (bitwise equal, tested).
    const int fuse_opt = itts_opt(OPT_DECODE_FUSE_LN);
    const bool fuse_ln = fuse_opt != 0 && rows <= (fuse_opt >= 2 ? 16 : 8) && !prefill && S == 1 && prec == PREC_BF16 &&
                         gemm_decode_ln_ok(rows, D, EPI_QKV) && w.x2 != nullptr;
    float *cur = w.x, *alt = w.x2;
    for (int l = 0; l < c.layers; ++l) {
        const GLayer& L = h->layers[l];
        LnArgs ln{};
        ln.x = cur; ln.partial = pend_bias ? w.partial : nullptr; ln.nsplit = 4; ln.bias_prev = pend_bias;
        ln.g1 = L.ln1_g; ln.b1 = L.ln1_b; ln.g2 = nullptr; ln.b2 = nullptr; ln.out = w.hbuf; ln.out_f32 = 0;
        ln.rows = rows; ln.D = D; ln.in_row_mul = 1; ln.in_row_add = 0; ln.eps = c.ln_eps;
        if (!fuse_ln && (rc = launch_ln(ln, prec, st))) return rc;

        GemmArgs g{};
        g.A = w.hbuf; g.lda = D; g.Wp = L.w_qkv; g.bias = L.b_qkv; g.M = rows; g.N = 3 * D; g.K = D; g.nsplit = 1; g.epi = EPI_QKV;
        g.qbuf = w.qbuf; g.kcache = w.kc + w.layer_cache_bytes * l; g.vcache = w.vc + w.layer_cache_bytes * l;
        g.pos_ptr = pos_ptr; g.S = S; g.H = c.heads; g.Tmax = Tmax; g.D = D; g.seq_mul = seq_mul; g.seq_map = seq_map; g.pos_shift = pos_shift;
        if (fuse_ln) {
            g.ln_x = cur; g.ln_partial = ln.partial; g.ln_bias_prev = pend_bias; g.ln_g = L.ln1_g; g.ln_b = L.ln1_b; g.ln_eps = c.ln_eps;
            g.ln_x_out = pend_bias ? alt : nullptr;
            if ((rc = launch_gemm_decode_ln(g, st))) return rc;
            if (pend_bias) { float* t = cur; cur = alt; alt = t; }
        } else if ((rc = launch_gemm(g, prec, prefill, st))) return rc;
        pend_bias = nullptr;

        // alignment export (itts_gpt_set_alignment): the decode query's attention over the row's text span, for this layer's selected heads.
        // Decode steps only; with nothing installed the pass issues exactly the launches it always did.
        if (h->align_out && !prefill && S == 1 && !beam) {
            AlignArgs al{};
            for (int k = 0; k < h->align_n_pairs; ++k)
                if (h->align_pairs[k][0] == l) { al.head[al.n_heads] = h->align_pairs[k][1]; al.kidx[al.n_heads] = k; ++al.n_heads; }
            if (al.n_heads) {
                al.qbuf = w.qbuf; al.kcache = g.kcache; al.pad = pad; al.pos_ptr = pos_ptr; al.pos_shift = pos_shift; al.seq_map = seq_map;
                al.seq_mul = seq_mul; al.row_slot = seq_map; al.step_ptr = w.state; al.row_step0 = w.row_step0;
                al.row_limit = (h->row_limits && h->row_limits_n == h->align_n) ? h->row_limits : nullptr;
                al.finished = w.finished; al.span = h->align_span; al.out = h->align_out;
                al.nseq = nseq; al.H = c.heads; al.Tmax = Tmax; al.D = D; al.max_new = h->align_max_new; al.n_pairs = h->align_n_pairs;
                al.text_cap = h->align_text_cap;
                if ((rc = launch_attention_align(al, prec, st))) return rc;
            }
        }

        if (mq) {                                                  // the rescoring pass's export: this layer's selected heads, many queries
            AlignMqArgs am{};
            for (int k = 0; k < mq->n_pairs; ++k)
                if (mq->pairs[k][0] == l) { am.head[am.n_heads] = mq->pairs[k][1]; am.kidx[am.n_heads] = k; ++am.n_heads; }
            if (am.n_heads) {
                am.qbuf = w.qbuf + (size_t)mq->q_row0 * D; am.q_stride = S; am.kcache = g.kcache; am.pad = pad; am.pos_ptr = mq->qpos_ptr;
                am.pos_shift = pos_shift; am.seq_map = seq_map; am.seq_mul = seq_mul; am.q_len = mq->q_len; am.span = mq->span; am.out = mq->out;
                am.nseq = nseq; am.nq = mq->nq; am.row0 = mq->row0; am.out_rows = mq->out_rows; am.H = c.heads; am.Tmax = Tmax; am.D = D;
                am.n_pairs = mq->n_pairs; am.text_cap = mq->text_cap;
                if ((rc = launch_attention_align_mq(am, prec, st))) return rc;
            }
        }

        AttnArgs at{};
        at.qbuf = w.qbuf; at.kcache = g.kcache; at.vcache = g.vcache; at.pad = pad; at.pos_ptr = pos_ptr; at.pos_shift = pos_shift;
        at.row_map = beam ? w.row_map[0] : nullptr; at.row_map_alt = beam ? w.row_map[1] : nullptr; at.step_ptr = beam ? w.state : nullptr;
        at.out = w.attn; at.nseq = nseq; at.H = c.heads; at.nq = S; at.Tmax = Tmax; at.D = D; at.seq_mul = seq_mul; at.seq_map = seq_map;
        if ((rc = launch_attention(at, prec, st))) return rc;

        GemmArgs p{};
        p.A = w.attn; p.lda = D; p.Wp = L.w_proj; p.bias = L.b_proj; p.M = rows; p.N = D; p.K = D; p.D = D;
        if (prefill) { p.nsplit = 1; p.epi = EPI_RESIDUAL; p.out_f32 = w.x; p.ldo = D; }
        else { p.nsplit = 4; p.epi = EPI_PARTIAL; p.partial = w.partial; }
        if ((rc = launch_gemm(p, prec, prefill, st))) return rc;

        LnArgs ln2 = ln;
        ln2.x = cur;
        ln2.partial = prefill ? nullptr : w.partial; ln2.bias_prev = prefill ? nullptr : L.b_proj;
        ln2.g1 = L.ln2_g; ln2.b1 = L.ln2_b;
        if (!fuse_ln && (rc = launch_ln(ln2, prec, st))) return rc;

        GemmArgs f{};
        f.A = w.hbuf; f.lda = D; f.Wp = L.w_fc; f.bias = L.b_fc; f.M = rows; f.N = 4 * D; f.K = D; f.nsplit = 1; f.epi = EPI_GELU_ACT;
        f.out_act = w.fc; f.ldo = 4 * D; f.D = D;
        if (fuse_ln) {                                             // (decode: the proj GEMM left partials, so the residual moves to `alt`)
            f.ln_x = cur; f.ln_partial = w.partial; f.ln_bias_prev = L.b_proj; f.ln_g = L.ln2_g; f.ln_b = L.ln2_b; f.ln_eps = c.ln_eps;
            f.ln_x_out = alt;
            if ((rc = launch_gemm_decode_ln(f, st))) return rc;
            float* t = cur; cur = alt; alt = t;
        } else if ((rc = launch_gemm(f, prec, prefill, st))) return rc;

        GemmArgs f2{};
        f2.A = w.fc; f2.lda = 4 * D; f2.Wp = L.w_fc2; f2.bias = L.b_fc2; f2.M = rows; f2.N = D; f2.K = 4 * D; f2.D = D;
        if (prefill) { f2.nsplit = 1; f2.epi = EPI_RESIDUAL; f2.out_f32 = w.x; f2.ldo = D; }
        else { f2.nsplit = 4; f2.epi = EPI_PARTIAL; f2.partial = w.partial; pend_bias = L.b_fc2; }
        if ((rc = launch_gemm(f2, prec, prefill, st))) return rc;
    }
    *pending = pend_bias != nullptr;   // decode: the last FC2's partials are reduced by the caller's final LayerNorm
    if (x_cur) *x_cur = cur;
    else if (cur != w.x) { itts_set_error("run_layers: the fused-LayerNorm path needs the caller to take x_cur"); return ITTS_ERR_STATE; }
    return ITTS_OK;
}

// final norm(s) + head: rows_out rows, input row r*mul+add
static int run_head(itts_gpt* h, const GptWs& w, int nseq, int mul, int add, bool pending, hipStream_t st, float* x = nullptr) {
    const itts_gpt_config& c = h->cfg;
    const int D = c.model_dim, prec = c.precision;
    int rc;
    LnArgs ln{};
    ln.x = x ? x : w.x;                  // (the residual stream: w.x2 after a decode pass on the LayerNorm-fused GEMMs)
    ln.partial = pending ? w.partial : nullptr; ln.nsplit = 4; ln.bias_prev = pending ? h->layers.back().b_fc2 : nullptr;
    ln.g1 = h->lnf_g; ln.b1 = h->lnf_b; ln.g2 = h->fn_g; ln.b2 = h->fn_b; ln.out = w.hlast; ln.out_f32 = 0;
    ln.rows = nseq; ln.D = D; ln.in_row_mul = mul; ln.in_row_add = add; ln.eps = c.ln_eps;
    if ((rc = launch_ln(ln, prec, st))) return rc;
    GemmArgs g{};
    g.A = w.hlast; g.lda = D; g.Wp = h->w_head; g.bias = h->b_head; g.M = nseq; g.N = c.vocab; g.K = D; g.nsplit = 1;
    g.epi = EPI_STORE_F32; g.out_f32 = w.logits; g.ldo = c.vocab; g.D = D;
    return launch_gemm(g, prec, false, st);
}

// rows: dense rows of this launch; n_utts: utterances of the call (stride of the uniform stream); mapped: the batch is compacted
static SampleArgs make_sample(itts_gpt* h, const GptWs& w, const itts_gen_params& gp, int nseq, long long* tokens,
                              const double* uniforms, int n_utts = 0, bool mapped = false) {
    const itts_gpt_config& c = h->cfg;
    SampleArgs s{};
    s.logits = w.logits; s.seen = w.seen; s.finished = w.finished; s.tokens = tokens; s.step_ptr = w.state;
    s.uniforms = uniforms; s.seed = gp.seed; s.B = nseq; s.V = c.vocab; s.max_new = gp.max_new_tokens;
    s.do_sample = gp.do_sample; s.top_k = gp.top_k; s.min_keep = gp.min_tokens_to_keep < 1 ? 1 : gp.min_tokens_to_keep;
    s.top_p = gp.top_p; s.temperature = gp.temperature; s.rep_penalty = gp.repetition_penalty;
    s.typical_mass = gp.typical_mass;
    s.stop_token = c.stop_mel_token; s.mel_emb = h->mel_emb; s.mel_pos = h->mel_pos; s.x_next = w.x; s.D = c.model_dim;
    s.pos_offset = gp.pos_offset; s.n_mel_pos = c.n_mel_pos;
    s.seed_ptr = (const unsigned long long*)(w.state + 4);
    s.row_slot = mapped ? w.slot_map : nullptr;
    s.uniforms_stride = n_utts > 0 ? n_utts : nseq;
    s.row_limit = (h->row_limits && h->row_limits_n == s.uniforms_stride) ? h->row_limits : nullptr;
    s.row_step0 = w.row_step0;
    s.row_table = (const RowSampling*)h->row_sampling;      // (the callers have checked that it covers the call's utterances)
    s.filt = h->filt(); s.filt_table = h->filt_table(); s.row_shift = w.row_shift;      // (the callers have checked the table's size: check_filter_table)
    s.logp_model = h->logp_model; s.logp_sampled = h->logp_sampled;      // (the callers have checked that they cover the call: check_scores)
    return s;
}

// rows: the dense rows this step runs (= n_utts until finished utterances have been compacted away)
// shifted: a row has been admitted into the batch (itts_gpt_admit_rows) -- the QKV epilogues and the attention read the per-row position shifts.
// Until then they are all zero and the step does not load them (the load sits behind the slot-map load in the QKV epilogue: ~1 % of a
// 1-8-row token step, profiles/r06e vs r05p).
static int decode_step(itts_gpt* h, const GptWs& w, const itts_gen_params& gp, int rows, int n_utts, bool mapped, int Tmax, long long* tokens,
                       const double* uniforms, hipStream_t st, bool shifted) {
    bool pending = false;
    float* xc = w.x;
    int rc = run_layers(h, w, rows, 1, Tmax, false, w.state + 1, w.pad, &pending, st, false, 1, mapped ? w.slot_map : nullptr, &xc,
                        shifted ? w.row_shift : nullptr);
    if (rc) return rc;
    if ((rc = run_head(h, w, rows, 1, 0, pending, st, xc))) return rc;
    SampleArgs s = make_sample(h, w, gp, rows, tokens, uniforms, n_utts, mapped);
    s.adv_state = w.state;                      // the sample kernel's last block advances step / pos
    return launch_sample(s, st);
}

// ---- the pieces every decode entry is made of ------------------------------------------------------------------------------------------
// never decode a batch with filters meant for another one
static int check_filter_table(const itts_gpt* h, int n_utts, const char* who) {
    if (h->ftab_n && h->ftab_n != n_utts) {
        itts_set_error("%s: the installed filter table has %d slots, the call %d utterances (itts_gpt_set_row_filters)", who, h->ftab_n, n_utts);
        return ITTS_ERR_STATE;
    }
    return ITTS_OK;
}

// ... and the beam entries refuse a table entry with an n-gram filter as they refuse the call-wide one
static int check_filter_table_beam(const itts_gpt* h, int n_groups, const char* who) {
    if (int rc = check_filter_table(h, n_groups, who)) return rc;
    for (int u = 0; u < h->ftab_n; ++u)
        if (h->ftab_ngram[(size_t)u] > 0) {
            itts_set_error("%s: no_repeat_ngram_size = %d is installed for group %d (itts_gpt_set_row_filters): the n-gram filter serves num_beams = 1 only "
                           "(a beam's history is not kept per row)", who, h->ftab_ngram[(size_t)u], u);
            return ITTS_ERR_ARG;
        }
    return ITTS_OK;
}

// Installed token-score arrays serve calls of exactly their shape: never write a batch's scores into arrays sized for another one
static int check_scores(const itts_gpt* h, int n_utts, int max_new, const char* who) {
    if (h->logp_model && (h->scores_n != n_utts || h->scores_max_new != max_new)) {
        itts_set_error("%s: the installed token-score arrays are [%d][%d], the call has %d utterances and max_new_tokens = %d (itts_gpt_set_token_scores)",
                       who, h->scores_n, h->scores_max_new, n_utts, max_new);
        return ITTS_ERR_STATE;
    }
    return ITTS_OK;
}
static int refuse_scores_beam(const itts_gpt* h, const char* who) {
    if (h->logp_model) {
        itts_set_error("%s: token-score arrays are installed (itts_gpt_set_token_scores): they serve num_beams = 1 only (a beam's transition scores need beam_indices)", who);
        return ITTS_ERR_STATE;
    }
    return ITTS_OK;
}
// An installed alignment export serves calls of exactly its shape, as the token scores do
static int check_alignment(const itts_gpt* h, int n_utts, int max_new, const char* who) {
    if (h->align_out && (h->align_n != n_utts || h->align_max_new != max_new)) {
        itts_set_error("%s: the installed alignment output is [%d][%d][..], the call has %d utterances and max_new_tokens = %d (itts_gpt_set_alignment)",
                       who, h->align_n, h->align_max_new, n_utts, max_new);
        return ITTS_ERR_STATE;
    }
    return ITTS_OK;
}
static int refuse_alignment_beam(const itts_gpt* h, const char* who) {
    if (h->align_out) {
        itts_set_error("%s: an alignment export is installed (itts_gpt_set_alignment): it serves num_beams = 1 only (a beam's rows change parents every step)", who);
        return ITTS_ERR_STATE;
    }
    return ITTS_OK;
}
static size_t align_row_elems(const itts_gpt* h) { return (size_t)h->align_max_new * h->align_n_pairs * h->align_text_cap; }
static char* align256(void* p) { return (char*)(((uintptr_t)p + 255) & ~(uintptr_t)255); }

// a call's workspace: the 256-byte aligned base inside the caller's buffer and the carve of (nseq, Sb, Tmax, nb) on it
struct WsCarve { char* base; GptWs w; };
static int carve_ws(const itts_gpt* h, void* workspace, size_t workspace_bytes, int nseq, int Sb, int Tmax, int nb, const char* who, WsCarve* out) {
    const size_t need = carve(h->cfg, nullptr, nseq, Sb, Tmax, nb).total;
    if (workspace_bytes < need) { itts_set_error("%s: workspace too small (%zu < %zu)", who, workspace_bytes, need); return ITTS_ERR_ARG; }
    out->base = align256(workspace);
    out->w = carve(h->cfg, out->base, nseq, Sb, Tmax, nb);
    return ITTS_OK;
}

// the pinned buffer the finished / done flags come to the host in
static int grow_host_fin(itts_gpt* h, int n) {
    if (h->fin_cap >= n) return ITTS_OK;
    if (h->host_fin) (void)hipHostFree(h->host_fin);
    HIP_TRY(hipHostMalloc((void**)&h->host_fin, (size_t)n, hipHostMallocDefault));
    h->fin_cap = n;
    return ITTS_OK;
}

// order the handle's stream after the caller's stream ...
static int stream_enter(itts_gpt* h, hipStream_t cs) {
    HIP_TRY(hipEventRecord(h->ev_in, cs));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_in, 0));
    return ITTS_OK;
}
// ... and hand back to it; the call returns with its work done
static int stream_leave(itts_gpt* h, hipStream_t cs) {
    HIP_TRY(hipEventRecord(h->ev_out, h->stream));
    HIP_TRY(hipStreamWaitEvent(cs, h->ev_out, 0));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return ITTS_OK;
}
// stream_leave of a generate call (ev_t0 | prefill | ev_t1 | decode loop | ev_t2 recorded): itts_gpt_last_timing
static int leave_timed(itts_gpt* h, hipStream_t cs, int steps) {
    if (int rc = stream_leave(h, cs)) return rc;
    (void)hipEventElapsedTime(&h->last_prefill_ms, h->ev_t0, h->ev_t1);
    (void)hipEventElapsedTime(&h->last_decode_ms, h->ev_t1, h->ev_t2);
    h->last_steps = steps;
    return ITTS_OK;
}

static int check_penalty_ids(int n_penalty_ids, const char* who) {
    if (n_penalty_ids < 0 || n_penalty_ids > 16) { itts_set_error("%s: at most 16 initial penalty ids", who); return ITTS_ERR_ARG; }
    return ITTS_OK;
}

// ---- code prefix (itts_gpt_set_code_prefix) ---------------------------------------------------------------------------------------------
// A row with a prefix p[0 .. k) is a row that has already taken k of its own steps: the prompt is prefilled as always, the prefix codes run
// through the stack as the rescoring pass runs given codes (the decode step's inputs, `chunk` cache positions per run_layers(prefill = true)),
// and the row's step / position tables are set so that every kernel of the decode step finds the row at own step k and own position S + k
// under the shared counters, which start where they always start (step 0, position S).  The first selection then writes column k.
// An installed table serves calls of exactly its rows; kmax: the longest prefix
static int check_prefix(const itts_gpt* h, int n, const itts_gen_params& gp, const char* who, int* kmax) {
    if (h->prefix_n != n) {
        itts_set_error("%s: the installed code prefix has %d rows, the call %d (itts_gpt_set_code_prefix)", who, h->prefix_n, n);
        return ITTS_ERR_STATE;
    }
    int m = 0;
    for (int b = 0; b < n; ++b) {
        const int k = h->prefix_lens[b];
        if (k >= gp.max_new_tokens) {
            itts_set_error("%s: code prefix of row %d holds %d codes, max_new_tokens = %d counts them and must leave one to generate", who, b, k, gp.max_new_tokens);
            return ITTS_ERR_ARG;
        }
        m = k > m ? k : m;
    }
    if (m > 0 && m - 1 + h->prefix_pos_offset >= h->cfg.n_mel_pos) {
        itts_set_error("%s: a code prefix of %d codes at position offset %d exceeds the mel position table (%d rows)", who, m, h->prefix_pos_offset, h->cfg.n_mel_pos);
        return ITTS_ERR_ARG;
    }
    *kmax = m;
    return ITTS_OK;
}
static int refuse_prefix(const itts_gpt* h, const char* who) {
    if (h->prefix_codes) {
        itts_set_error("%s: a code prefix is installed (itts_gpt_set_code_prefix): it serves num_beams = 1 rows only", who);
        return ITTS_ERR_STATE;
    }
    return ITTS_OK;
}
// The ingest, called after the prompt's prefill on `w` (residual stream of the n prompts in w.x, their K / V at cache positions 0 .. S - 1, w.pad
// set): the prefix codes at cache positions S .. S + kmax - 1, at most min(chunk, Sb) per pass -- the activations of `w` hold Sb rows per
// sequence -- and ln_f -> final_norm -> head over ONE query per row, its last valid one (S - 1 + lens[b]; the prompt's last position at
// lens[b] = 0), gathered into w.partial (free until the first decode step).  Leaves n rows of logits in w.logits.
// `tab`: the workspace whose per-utterance tables (seen, row_step0, row_shift) the rows live in, at slots_dev[b] (null: b); step0 / shift: what
// a row without a prefix gets there.
// A row shorter than kmax runs dead queries: they write K / V at the row's cache positions S + lens[b] .. S + kmax - 1.  Nothing reads those
// before the row's own decode steps rewrite them -- the step at own position p stores K / V at p before its attention reads keys <= p, and p
// starts at S + lens[b] -- and the row's live queries never attend past themselves (causal), so a row's logits do not depend on kmax.
static int prefix_ingest(itts_gpt* h, const GptWs& w, const GptWs& tab, int n, int S, int Sb, int Tmax, const int* slots_dev, int step0, int shift,
                         long long* tokens, int max_new, const int* lens_dev, int kmax, hipStream_t st) {
    const itts_gpt_config& c = h->cfg;
    int rc;
    float* xg = w.partial;
    PrefixGatherArgs ga{};
    ga.x = w.x; ga.n = S; ga.j0 = 0; ga.force_q = S - 1; ga.nseq = n; ga.D = c.model_dim; ga.lens = lens_dev; ga.out = xg;
    if ((rc = launch_prefix_gather(ga, st))) return rc;
    int chunk = h->prefix_chunk < Sb ? h->prefix_chunk : Sb;
    chunk = chunk < kmax ? chunk : kmax;
    int chunks = 0;
    for (int j0 = 0; j0 < kmax; j0 += chunk, ++chunks) {
        const int nq = kmax - j0 < chunk ? kmax - j0 : chunk;
        hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 0, S + j0);
        PrefixEmbedArgs e{};
        e.codes = (const long long*)h->prefix_codes; e.width = h->prefix_width; e.lens = lens_dev; e.slots = slots_dev;
        e.j0 = j0; e.n = nq; e.nseq = n; e.pos_offset = h->prefix_pos_offset; e.V = c.vocab; e.n_mel_pos = c.n_mel_pos; e.D = c.model_dim;
        e.mel_emb = h->mel_emb; e.mel_pos = h->mel_pos; e.x = w.x; e.tokens = tokens; e.max_new = max_new; e.seen = tab.seen;
        e.row_step0 = tab.row_step0; e.row_shift = tab.row_shift; e.step0 = step0; e.shift = shift;
        e.logp_model = h->logp_model; e.logp_sampled = h->logp_sampled;
        if ((rc = launch_prefix_embed(e, st))) return rc;
        bool pending = false;
        if ((rc = run_layers(h, w, n, nq, Tmax, true, w.state + 1, w.pad, &pending, st))) return rc;
        ga.n = nq; ga.j0 = j0; ga.force_q = -1;
        if ((rc = launch_prefix_gather(ga, st))) return rc;
    }
    h->last_prefix_chunks = chunks;
    h->last_prefix_max = kmax;
    return run_head(h, w, n, 1, 0, false, st, xg);
}

// A decode step graph bakes in every pointer and scalar of its launches; the fields every step has (the callers add theirs: aux0 .. aux3, ...)
static itts_gpt::GraphEntry graph_key(const void* base, int nseq, int nb, int Sb, int Tmax, int S, const itts_gen_params& gp) {
    itts_gpt::GraphEntry key{};
    key.base = base; key.nseq = nseq; key.nb = nb; key.Sb = Sb; key.Tmax = Tmax; key.S = S;
    key.gp = gp; key.gp.seed = 0;                                      // the seed lives in device memory
    key.opt_epoch = itts_opt_epoch();
    return key;
}
// The step graph of `key`: the handle's cached one, else one decode step -- step() issues its launches on h->stream; all step-varying state
// lives in device memory -- is captured, instantiated and kept in the handle for later calls.
template <class Step>
static int step_graph(itts_gpt* h, const itts_gpt::GraphEntry& key_in, const char* who, Step step, hipGraphExec_t* exec) {
    itts_gpt::GraphEntry key = key_in;
    key.scores0 = h->logp_model; key.scores1 = h->logp_sampled;
    key.align_out = h->align_out; key.align_span = h->align_span; key.align_epoch = h->align_out ? h->align_epoch : 0;
    // a step captured without filters has a null record baked in: never replay it for a filtered call (or the reverse); a step captured
    // under the per-slot table indexes the address by slot, one under the call-wide record reads one record: the kind is part of the key
    // beside the address (and no filter allocation is freed before the handle is, so no address is ever handed out for the other kind)
    key.filt = h->ftab_n ? (const void*)h->ftab_dev : (const void*)h->filt();
    key.filt_is_table = h->ftab_n ? 1 : 0;
    if ((*exec = graph_lookup(h, key))) return ITTS_OK;
    hipGraph_t graph = nullptr;
    bool ok = false;
    hipError_t e = hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        const int rc = step();
        e = hipStreamEndCapture(h->stream, &graph);
        if (rc == ITTS_OK && e == hipSuccess && graph) {
            e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
            ok = (e == hipSuccess && *exec);
        }
        if (graph) (void)hipGraphDestroy(graph);
    }
    if (!ok) {
        *exec = nullptr;
        (void)hipGetLastError();
        itts_set_error("%s: hipGraph capture failed (%s); rerun with use_graph=0", who, hipGetErrorString(e));
        return ITTS_ERR_HIP;
    }
    graph_insert(h, key, *exec);
    return ITTS_OK;
}

// step_limit: stop after that many generated tokens (<= max_new_tokens) -- the chunked form used for streaming; resume: continue
// the decode loop of an earlier chunk call from the device state left in the same workspace (no prefill, no state init).
static int gpt_generate_impl(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int nseq, int S,
                             const itts_gen_params* gpp, const int32_t* penalty_ids, int n_penalty_ids,
                             const double* uniforms, int64_t* codes_out, int32_t* n_steps_out, void* workspace,
                             size_t workspace_bytes, int use_graph, void* caller_stream, int step_limit, bool resume) {
    const char* who = "gpt_generate";
    if (!h || (!prefix_embeds && !resume) || !gpp || !codes_out || !n_steps_out || !workspace) { itts_set_error("gpt_generate: null pointer"); return ITTS_ERR_ARG; }
    if (!h->finalized) { itts_set_error("gpt_generate: call itts_gpt_finalize first"); return ITTS_ERR_STATE; }
    ItDevGuard dg(h->device);
    if (int rcd = check_same_device(h, resume ? (const void*)codes_out : (const void*)prefix_embeds, workspace, who)) return rcd;
    const itts_gpt_config& c = h->cfg;
    const itts_gen_params gp = *gpp;
    itts_gpt::Suspended& su = h->susp;
    if (nseq <= 0 || S <= 0 || gp.max_new_tokens <= 0) { itts_set_error("gpt_generate: nseq, S, max_new_tokens must be > 0"); return ITTS_ERR_ARG; }
    // The first call's step counter is bounded by max_new_tokens.  A resumed loop's is not: every row is bounded by its OWN step (the sampler emits
    // the stop token from the row's step max_new_tokens / its row limit on and stores nothing; a finished row's K / V stay inside its cache row), so a
    // session runs for as long as the caller keeps admitting rows (itts_gpt_admit_rows).
    const bool chunked = step_limit > 0;                               // itts_gpt_generate_chunk (itts_gpt_generate passes 0)
    if (step_limit < 1 || (step_limit > gp.max_new_tokens && !resume)) step_limit = gp.max_new_tokens;
    if (resume && (su.kind != itts_gpt::Suspended::ROWS || su.n_utts != nseq || su.S != S || su.gp.max_new_tokens != gp.max_new_tokens ||
                   su.ws != workspace)) {
        itts_set_error("gpt_generate_chunk: resume without a matching first chunk (same workspace, nseq, S, max_new_tokens)");
        return ITTS_ERR_STATE;
    }
    if (gp.num_beams != 1) { itts_set_error("gpt_generate: num_beams=%d not supported by the device loop yet (use 1)", gp.num_beams); return ITTS_ERR_ARG; }
    if (h->group_sampling) {
        itts_set_error("gpt_generate: a per-group sampling table is installed (itts_gpt_set_group_sampling): it serves beam calls only (num_beams = 1 takes itts_gpt_set_row_sampling)");
        return ITTS_ERR_STATE;
    }
    if (h->row_sampling && h->row_sampling_n != nseq) {              // never decode a batch with settings meant for another one
        itts_set_error("gpt_generate: the installed sampling table has %d entries, the call %d utterances (itts_gpt_set_row_sampling)", h->row_sampling_n, nseq);
        return ITTS_ERR_STATE;
    }
    if (int rcf = check_filter_table(h, nseq, who)) return rcf;
    if (int rcs = check_scores(h, nseq, gp.max_new_tokens, who)) return rcs;
    if (int rca = check_alignment(h, nseq, gp.max_new_tokens, who)) return rca;
    if (gp.max_new_tokens + gp.pos_offset > c.n_mel_pos + 1) {
        itts_set_error("gpt_generate: max_new_tokens=%d exceeds the mel position table (%d rows)", gp.max_new_tokens, c.n_mel_pos);
        return ITTS_ERR_ARG;
    }
    const bool pfx = h->prefix_codes && !resume;                     // an installed code prefix serves first calls: a resumed loop has its rows
    int kmax = 0;
    if (pfx) { if (int rcp = check_prefix(h, nseq, gp, who, &kmax)) return rcp; }
    int rc;
    if ((rc = check_penalty_ids(n_penalty_ids, who))) return rc;
    if ((size_t)nseq * c.heads > 2147483647u / 4 || S > 65535) { itts_set_error("gpt_generate: batch too large"); return ITTS_ERR_ARG; }
    const int Sb = s_bucket(S), Tmax = Sb + gp.max_new_tokens;      // cache stride / carve shape (bucketed prompt length)
    WsCarve wc;
    if ((rc = carve_ws(h, workspace, workspace_bytes, nseq, Sb, Tmax, 1, who, &wc))) return rc;
    const GptWs& w = wc.w;
    if (!resume) su = itts_gpt::Suspended{};                           // (whatever loop was suspended on this handle is over)
    hipStream_t st = h->stream, cs = (hipStream_t)caller_stream;
    long long* tokens = (long long*)codes_out;
    if ((rc = grow_host_fin(h, nseq))) return rc;
    if ((rc = stream_enter(h, cs))) return rc;

    int steps = resume ? su.steps : 1;
    if (!resume) {
    // ---- state init ----
    HIP_TRY(hipMemsetAsync(w.seen, 0, (size_t)nseq * c.vocab, st));
    HIP_TRY(hipMemsetAsync(w.finished, 0, nseq, st));
    HIP_TRY(hipMemsetAsync(w.row_step0, 0, (size_t)nseq * 4, st));
    HIP_TRY(hipMemsetAsync(w.row_shift, 0, (size_t)nseq * 4, st));
    if (pad_lens) HIP_TRY(hipMemcpyAsync(w.pad, pad_lens, (size_t)nseq * 4, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemsetAsync(w.pad, 0, (size_t)nseq * 4, st));
    if (n_penalty_ids > 0) {
        HIP_TRY(hipMemcpyAsync(w.pen_ids, penalty_ids, (size_t)n_penalty_ids * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mark_seen_kernel, dim3(nseq), dim3(64), 0, st, w.seen, w.pen_ids, n_penalty_ids, c.vocab);
    }
    {
        const size_t n = (size_t)nseq * gp.max_new_tokens;
        hipLaunchKernelGGL(fill_i64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tokens, (long long)c.stop_mel_token, n);
        if (h->logp_model) {                     // a first call clears its rows' scores: 0.0 wherever no token gets scored
            HIP_TRY(hipMemsetAsync(h->logp_model, 0, n * sizeof(float), st));
            HIP_TRY(hipMemsetAsync(h->logp_sampled, 0, n * sizeof(float), st));
        }
        if (h->align_out)                        // ... and its alignment rows: 0.0 in every row no decode step writes
            HIP_TRY(hipMemsetAsync(h->align_out, 0, (size_t)nseq * align_row_elems(h) * sizeof(float), st));
    }
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 0, 0);
    hipLaunchKernelGGL(set_seed_kernel, dim3(1), dim3(1), 0, st, w.state, (unsigned long long)gp.seed);
    if (h->filt_on && !h->ftab_n) hipLaunchKernelGGL(set_filter_prompt_kernel, dim3(1), dim3(1), 0, st, h->filt_dev, S);   // min_length / the n-gram prefix count from the prompt
    if (h->ftab_n) hipLaunchKernelGGL(set_filter_table_prompt_kernel, dim3((unsigned)((h->ftab_n + 255) / 256)), dim3(256), 0, st, h->ftab_dev, h->ftab_n, S);
    HIP_TRY(hipMemcpyAsync(w.x, prefix_embeds, (size_t)nseq * S * c.model_dim * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGetLastError());

    // ---- prefill: all S positions, logits of the last one, first token ----
    HIP_TRY(hipEventRecord(h->ev_t0, st));
    bool pending = false;
    rc = run_layers(h, w, nseq, S, Tmax, true, w.state + 1, w.pad, &pending, st);
    if (rc) return rc;
    h->last_prefix_chunks = 0; h->last_prefix_max = -1;              // (-1: this call ran no ingest)
    if (pfx) {
        // the rows' lengths on the device, in the compaction's gather list (unused until the first compaction); the ingest leaves every row's
        // own step / position in row_step0 / row_shift, so the decode step reads the shifts from its first step on
        HIP_TRY(hipMemcpyAsync(w.gather_src, h->prefix_lens.data(), (size_t)nseq * 4, hipMemcpyHostToDevice, st));
        if ((rc = prefix_ingest(h, w, w, nseq, S, Sb, Tmax, nullptr, 0, 0, tokens, gp.max_new_tokens, w.gather_src, kmax, st))) return rc;
        su.admitted = true;
    } else if ((rc = run_head(h, w, nseq, S, S - 1, pending, st))) return rc;
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 0, S);
    {
        SampleArgs s = make_sample(h, w, gp, nseq, tokens, uniforms, nseq, false);
        if ((rc = launch_sample(s, st))) return rc;
    }
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 1, S);
    } else {
        HIP_TRY(hipEventRecord(h->ev_t0, st));
    }
    HIP_TRY(hipEventRecord(h->ev_t1, st));

    // ---- decode loop ----
    // The running batch starts as the nseq utterances in order.  Every `check_every` steps the finished flags come to the host; when
    // enough utterances have finished, the survivors are compacted to the front (their cache rows stay where they are: the QKV
    // epilogue, the attention kernel and the sampler find an utterance's state through the slot map) and the step is replayed from
    // the graph of the smaller batch -- the step's cost follows the live rows in steps of `compact_gran`.
    if (h->map_cap < nseq) {
        if (h->host_map) (void)hipHostFree(h->host_map);
        HIP_TRY(hipHostMalloc((void**)&h->host_map, (size_t)2 * nseq * sizeof(int), hipHostMallocDefault));
        h->map_cap = nseq;
    }
    if (!resume) {
        h->cur_slots.resize(nseq);
        for (int i = 0; i < nseq; ++i) h->cur_slots[i] = i;
        h->cur_mapped = false;
        h->last_row_steps = 0;
        h->last_compactions = 0;
    }
    const bool env_off = itts_opt(OPT_GPT_COMPACT) == 0;
    const bool compact = h->compact && !env_off;
    int rows = (int)h->cur_slots.size();
    bool mapped = h->cur_mapped;
    hipGraphExec_t exec = nullptr;
    auto step = [&] { return decode_step(h, w, gp, rows, nseq, mapped, Tmax, tokens, uniforms, st, su.admitted); };
    auto get_graph = [&]() -> int {                                    // the step graph of the current (rows, mapped), or none: plain launches
        exec = nullptr;
        if (!(use_graph && gp.max_new_tokens > 1)) return ITTS_OK;
        itts_gpt::GraphEntry key = graph_key(wc.base, rows, 1, Sb, Tmax, nseq, gp);     // S: utterances of the call (uniform stride, limits)
        key.tokens = tokens; key.uniforms = uniforms;
        key.aux0 = mapped ? (const void*)w.slot_map : nullptr;
        key.aux1 = (h->row_limits && h->row_limits_n == nseq) ? (const void*)h->row_limits : nullptr;
        key.aux2 = su.admitted ? (const void*)w.row_shift : nullptr;
        key.aux3 = (const void*)h->row_sampling;                      // the step reads its sampling settings from this table, not from gp
        return step_graph(h, key, who, step, &exec);
    };
    if ((rc = get_graph())) return rc;
    const int check_every = 8;
    while (steps < step_limit) {
        if (exec) { HIP_TRY(hipGraphLaunch(exec, st)); }
        else if ((rc = step())) return rc;
        ++steps;
        h->last_row_steps += rows;
        if (steps % check_every == 0 && steps < step_limit) {
            HIP_TRY(hipMemcpyAsync(h->host_fin, w.finished, nseq, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            int live = 0;
            for (int i = 0; i < nseq; ++i) live += h->host_fin[i] ? 0 : 1;
            if (live == 0) break;
            if (chunked && h->chunk_return_finished > 0 && nseq - live >= h->chunk_return_finished) break;        // slots to refill
            const int g = h->compact_gran < 1 ? 1 : h->compact_gran;
            const int want = ((live + g - 1) / g) * g;
            if (compact && want < rows) {
                // new dense order: the live rows in their current order, then finished rows up to the bucket size (they keep emitting stop)
                int* nm = h->host_map;
                int* src = h->host_map + nseq;
                int k = 0;
                for (int i = 0; i < rows; ++i)
                    if (!h->host_fin[h->cur_slots[i]]) { nm[k] = h->cur_slots[i]; src[k] = i; ++k; }
                for (int i = 0; i < rows && k < want; ++i)
                    if (h->host_fin[h->cur_slots[i]]) { nm[k] = h->cur_slots[i]; src[k] = i; ++k; }
                HIP_TRY(hipMemcpyAsync(w.slot_map, nm, (size_t)want * sizeof(int), hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(w.gather_src, src, (size_t)want * sizeof(int), hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(gather_rows_kernel, dim3(want), dim3(256), 0, st, w.x, w.gather_src, w.qbuf, c.model_dim);
                hipLaunchKernelGGL(copy_rows_kernel, dim3(want), dim3(256), 0, st, w.qbuf, w.x, c.model_dim);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(st));                      // the pinned staging buffer is reused by the next compaction
                h->cur_slots.assign(nm, nm + want);
                rows = want;
                mapped = true;
                h->cur_mapped = true;
                ++h->last_compactions;
                if ((rc = get_graph())) return rc;
            }
        }
    }
    HIP_TRY(hipEventRecord(h->ev_t2, st));
    if ((rc = leave_timed(h, cs, steps))) return rc;
    su.kind = itts_gpt::Suspended::ROWS; su.ws = workspace; su.n_utts = nseq; su.nb = 1; su.S = S; su.gp = gp;
    su.codes = codes_out; su.uniforms = uniforms; su.steps = steps;
    *n_steps_out = steps;
    return ITTS_OK;
}

extern "C" int itts_gpt_generate(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int nseq, int S,
                                 const itts_gen_params* gpp, const int32_t* penalty_ids, int n_penalty_ids,
                                 const double* uniforms, int64_t* codes_out, int32_t* n_steps_out, void* workspace,
                                 size_t workspace_bytes, int use_graph, void* caller_stream) {
    return gpt_generate_impl(h, prefix_embeds, pad_lens, nseq, S, gpp, penalty_ids, n_penalty_ids, uniforms, codes_out, n_steps_out,
                             workspace, workspace_bytes, use_graph, caller_stream, 0, false);
}

extern "C" int itts_gpt_generate_chunk(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int nseq, int S,
                                       const itts_gen_params* gpp, const int32_t* penalty_ids, int n_penalty_ids,
                                       const double* uniforms, int64_t* codes_out, int32_t step_limit, int32_t* n_steps_out,
                                       void* workspace, size_t workspace_bytes, int use_graph, void* caller_stream) {
    return gpt_generate_impl(h, prefix_embeds, pad_lens, nseq, S, gpp, penalty_ids, n_penalty_ids, uniforms, codes_out, n_steps_out,
                             workspace, workspace_bytes, use_graph, caller_stream, step_limit, prefix_embeds == nullptr);
}

// ---- admission of new utterances into a running decode batch -------------------------------------------------------------------------
// Design reference: the reference's serving path keeps a decode batch running and puts a newly arrived request into a free slot while the other
// rows keep generating (backends/trt/serving/triton_server.py:96-305, backends/trt/pipeline/pipeline.py:459-548 on TRT-LLM's in-flight batching).
// Here: between two itts_gpt_generate_chunk calls the loop is suspended with its state on the device; the batch's position counter stands at
// pos = S + steps - 1.  A new utterance takes the cache row of a FINISHED one and keeps its OWN positions: its prompt (S_new positions, at most the
// session's prompt bucket) is prefilled on an admission workspace of its own (K / V to a scratch cache, copied to positions 0 .. S_new - 1 of the
// slot's cache rows), row_shift[slot] = pos - S_new lets the QKV epilogue and the attention kernel find the row's own position under the shared
// counter, its first token is sampled into column 0 of the slot's code row (refilled with the stop token), and row_step0[slot] = steps - 1 makes
// the sampler index the row's token column, position embedding, uniform / RNG stream and token limit by the row's OWN step.  Nothing of the row
// depends on the step it joined at -- the attention's key streams are laid out from the row's first valid key -- so the admitted row generates,
// bit for bit, the ids it generates alone (tests/test_gpu_admission.py), and a session is not bounded by the mel position table: only each row is.
__global__ void admit_state_kernel(const int* __restrict__ slots, const int* __restrict__ pad_new, unsigned char* seen, unsigned char* finished, int* pad,
                                   int* row_step0, int* row_shift, const int* __restrict__ pen_ids, int n_ids, int V, int step0, int shift,
                                   long long* tokens, int max_new, long long stop_token, int* row_limit, const int* __restrict__ limits_new,
                                   float* logp_model, float* logp_sampled) {
    const int i = blockIdx.x, u = slots[i];
    unsigned char* sr = seen + (size_t)u * V;
    for (int c = threadIdx.x; c < V; c += blockDim.x) sr[c] = 0;
    long long* tr = tokens + (size_t)u * max_new;
    for (int c = threadIdx.x; c < max_new; c += blockDim.x) tr[c] = stop_token;
    if (logp_model)                                 // the previous occupant's scores go with its codes
        for (int c = threadIdx.x; c < max_new; c += blockDim.x) { logp_model[(size_t)u * max_new + c] = 0.f; logp_sampled[(size_t)u * max_new + c] = 0.f; }
    __syncthreads();
    if ((int)threadIdx.x < n_ids) {
        const int id = pen_ids[threadIdx.x];
        if (id >= 0 && id < V) sr[id] = 1;
    }
    if (threadIdx.x == 0) {
        finished[u] = 0; pad[u] = pad_new[i]; row_step0[u] = step0; row_shift[u] = shift;
        if (row_limit && limits_new) row_limit[u] = limits_new[i];
    }
}
// K / V of positions [0, n_pos) of the admission cache's row i -> the running batch's cache row slots[i] (both [L][rows][H][T][64], own T strides)
// extra (null: none): row i copies n_pos + extra[i] positions -- an admitted row's prompt and its own code prefix
__global__ void copy_kv_rows_kernel(const char* __restrict__ src, char* __restrict__ dst, const int* __restrict__ slots, int H, int T_src, int T_dst,
                                    int n_pos, int row_bytes, size_t src_layer, size_t dst_layer, const int* __restrict__ extra = nullptr) {
    const int i = blockIdx.x / H, hd = blockIdx.x - i * H, l = blockIdx.y;
    const char* s = src + (size_t)l * src_layer + ((size_t)i * H + hd) * T_src * row_bytes;
    char* d = dst + (size_t)l * dst_layer + ((size_t)slots[i] * H + hd) * T_dst * row_bytes;
    const size_t n16 = (size_t)(n_pos + (extra ? extra[i] : 0)) * row_bytes / 16;
    for (size_t c = threadIdx.x; c < n16; c += blockDim.x) ((uint4*)d)[c] = ((const uint4*)s)[c];
}
// dense rows back to utterance order: tmp[d] = x[src[d]] (zero where the utterance is not in the running batch), then the admitted rows
__global__ void regather_rows_kernel(const float* __restrict__ x, const int* __restrict__ src, float* __restrict__ tmp, int D) {
    const int d = blockIdx.x, j = src[d];
    for (int c = threadIdx.x; c < D; c += blockDim.x) tmp[(size_t)d * D + c] = j >= 0 ? x[(size_t)j * D + c] : 0.f;
}
__global__ void place_rows_kernel(const float* __restrict__ xa, const int* __restrict__ slots, float* __restrict__ x, int D) {
    const int i = blockIdx.x;
    for (int c = threadIdx.x; c < D; c += blockDim.x) x[(size_t)slots[i] * D + c] = xa[(size_t)i * D + c];
}

// field by field: a caller's struct may carry anything in its padding bytes
static bool gp_same(const itts_gen_params& a, const itts_gen_params& b) {
    return a.do_sample == b.do_sample && a.num_beams == b.num_beams && a.top_k == b.top_k && a.min_tokens_to_keep == b.min_tokens_to_keep &&
           a.max_new_tokens == b.max_new_tokens && a.pos_offset == b.pos_offset && a.top_p == b.top_p && a.temperature == b.temperature &&
           a.repetition_penalty == b.repetition_penalty && a.length_penalty == b.length_penalty && a.typical_mass == b.typical_mass &&
           a.reserved == b.reserved && a.seed == b.seed;
}

extern "C" size_t itts_gpt_admit_workspace_bytes(const itts_gpt* h, int n_new, int S_new) {
    if (!h || n_new <= 0 || S_new <= 0) return 0;
    const int Sb = s_bucket(S_new);
    return carve(h->cfg, nullptr, n_new, Sb, Sb + 8).total + a256((size_t)n_new * 8) + 512;
}
// ... of an admission whose rows bring a code prefix of at most max_prefix codes (itts_gpt_set_code_prefix): the admission cache holds them too
extern "C" size_t itts_gpt_admit_prefix_workspace_bytes(const itts_gpt* h, int n_new, int S_new, int max_prefix) {
    if (!h || n_new <= 0 || S_new <= 0 || max_prefix < 0) return 0;
    const int Sb = s_bucket(S_new);
    return carve(h->cfg, nullptr, n_new, Sb, Sb + 8 + max_prefix).total + a256((size_t)n_new * 12) + 512;
}

// ---- what the two admissions share ----
// The admission workspace: a carve of its own for the prefill of n_new prompts (S_new positions, bucketed; 8 spare cache positions), followed by
// `ints_per` int32 per new prompt (slots, ...) that the admission's kernels read.
struct AdmitWs { GptWs w; int Ta; int* ints; };
static int carve_admit(const itts_gpt* h, void* admit_workspace, size_t admit_bytes, int n_new, int S_new, int ints_per, const char* who, AdmitWs* out,
                       int extra_pos = 0) {                            // extra_pos: cache positions of the rows' code prefix
    const int Sba = s_bucket(S_new), Ta = Sba + 8 + extra_pos;
    const size_t ints_off = carve(h->cfg, nullptr, n_new, Sba, Ta).total, need = ints_off + a256((size_t)n_new * 4 * ints_per) + 256;
    if (admit_bytes < need) { itts_set_error("%s: admission workspace too small (%zu < %zu)", who, admit_bytes, need); return ITTS_ERR_ARG; }
    char* abase = align256(admit_workspace);
    out->w = carve(h->cfg, abase, n_new, Sba, Ta);
    out->Ta = Ta;
    out->ints = (int*)(abase + ints_off);
    return ITTS_OK;
}
// the slots an admission takes over must be distinct, in range and free (is_free(slot)); `busy`: what a slot that is not free is still doing
template <class Free>
static int check_slots(const int32_t* slots, int n_new, int n_slots, Free is_free, const char* who, const char* busy) {
    std::vector<char> taken(n_slots, 0);
    for (int i = 0; i < n_new; ++i) {
        const int u = slots[i];
        if (u < 0 || u >= n_slots || taken[u] || !is_free(u)) {
            itts_set_error("%s: slot %d (entry %d) is out of range, repeated or still %s", who, u, i, busy);
            return ITTS_ERR_ARG;
        }
        taken[u] = 1;
    }
    return ITTS_OK;
}
// prefill of the n_new prompts on the admission workspace: all S_new positions, logits of the last one (wa.w.logits)
// (head = false: the stack only -- a code prefix follows, whose ingest runs the head)
static int admit_prefill(itts_gpt* h, const AdmitWs& wa, const float* prefix_embeds, int n_new, int S_new, hipStream_t st, bool head = true) {
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, wa.w.state, 0, 0);
    HIP_TRY(hipMemcpyAsync(wa.w.x, prefix_embeds, (size_t)n_new * S_new * h->cfg.model_dim * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGetLastError());
    bool pending = false;
    if (int rc = run_layers(h, wa.w, n_new, S_new, wa.Ta, true, wa.w.state + 1, wa.w.pad, &pending, st)) return rc;
    return head ? run_head(h, wa.w, n_new, S_new, S_new - 1, pending, st) : ITTS_OK;
}
// K / V of the prompts (positions 0 .. S_new - 1 of the admission cache, and extra_dev[i] more: the row's code prefix) into the running
// batch's cache rows rows_dev[i]
static void admit_copy_kv(const itts_gpt* h, const AdmitWs& wa, const GptWs& w, const int* rows_dev, int n_new, int S_new, int Tmax, hipStream_t st,
                          const int* extra_dev = nullptr) {
    const itts_gpt_config& c = h->cfg;
    const int rb = 64 * (c.precision == PREC_BF16 ? 2 : 4);
    hipLaunchKernelGGL(copy_kv_rows_kernel, dim3(n_new * c.heads, c.layers), dim3(256), 0, st, wa.w.kc, w.kc, rows_dev, c.heads, wa.Ta, Tmax, S_new, rb,
                       wa.w.layer_cache_bytes, w.layer_cache_bytes, extra_dev);
    hipLaunchKernelGGL(copy_kv_rows_kernel, dim3(n_new * c.heads, c.layers), dim3(256), 0, st, wa.w.vc, w.vc, rows_dev, c.heads, wa.Ta, Tmax, S_new, rb,
                       wa.w.layer_cache_bytes, w.layer_cache_bytes, extra_dev);
}

extern "C" int itts_gpt_admit_rows(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, const int32_t* slots, int n_new, int S_new,
                                   const int32_t* row_limits_new, const itts_gen_params* gpp, const int32_t* penalty_ids, int n_penalty_ids,
                                   const double* uniforms, int64_t* codes_out, void* workspace, size_t workspace_bytes, void* admit_workspace,
                                   size_t admit_bytes, void* caller_stream) {
    const char* who = "gpt_admit_rows";
    if (!h || !prefix_embeds || !pad_lens || !slots || !gpp || !codes_out || !workspace || !admit_workspace) { itts_set_error("gpt_admit_rows: null pointer"); return ITTS_ERR_ARG; }
    if (!h->finalized) { itts_set_error("gpt_admit_rows: call itts_gpt_finalize first"); return ITTS_ERR_STATE; }
    ItDevGuard dg(h->device);
    if (int rcd = check_same_device(h, prefix_embeds, workspace, who)) return rcd;
    const itts_gpt_config& c = h->cfg;
    const itts_gen_params gp = *gpp;
    itts_gpt::Suspended& su = h->susp;
    if (su.kind != itts_gpt::Suspended::ROWS || su.ws != workspace || gp.max_new_tokens != su.gp.max_new_tokens || gp.num_beams != 1) {
        itts_set_error("gpt_admit_rows: no suspended itts_gpt_generate_chunk loop on this workspace with these parameters");
        return ITTS_ERR_STATE;
    }
    const int nseq = su.n_utts, S = su.S, k = su.steps;
    // the suspended loop's captured step has the code buffer, the uniform stream and the sampling parameters baked in: the admitted rows' first
    // token must be sampled with the same ones
    if (su.codes != (const void*)codes_out || su.uniforms != (const void*)uniforms || !gp_same(su.gp, gp)) {
        itts_set_error("gpt_admit_rows: codes_out, uniforms and the generation parameters must be those of the suspended itts_gpt_generate_chunk loop");
        return ITTS_ERR_STATE;
    }
    const int Sb = s_bucket(S), Tmax = Sb + gp.max_new_tokens;
    if (S_new < 1 || S_new > Sb) {      // a cache row holds Sb prompt positions + max_new_tokens generated ones
        itts_set_error("gpt_admit_rows: S_new = %d outside 1 .. %d (the session's prompt bucket)", S_new, Sb);
        return ITTS_ERR_ARG;
    }
    if (h->group_sampling) {
        itts_set_error("gpt_admit_rows: a per-group sampling table is installed (itts_gpt_set_group_sampling): it serves beam sessions only");
        return ITTS_ERR_STATE;
    }
    if (h->row_sampling && h->row_sampling_n != nseq) {
        itts_set_error("gpt_admit_rows: the installed sampling table has %d entries, the session %d slots", h->row_sampling_n, nseq);
        return ITTS_ERR_STATE;
    }
    if (int rcf = check_filter_table(h, nseq, who)) return rcf;
    const bool limited = h->row_limits && h->row_limits_n == nseq;
    if (limited != (row_limits_new != nullptr)) {
        itts_set_error("gpt_admit_rows: row_limits_new must be given exactly when per-utterance limits are installed (itts_gpt_set_row_limits, %d entries)", nseq);
        return ITTS_ERR_ARG;
    }
    if (n_new < 1 || n_new > nseq) { itts_set_error("gpt_admit_rows: n_new = %d outside 1 .. %d", n_new, nseq); return ITTS_ERR_ARG; }
    if (int rcs = check_scores(h, nseq, gp.max_new_tokens, who)) return rcs;
    if (int rca = check_alignment(h, nseq, gp.max_new_tokens, who)) return rca;
    int rc;
    if ((rc = check_penalty_ids(n_penalty_ids, who))) return rc;
    const bool pfx = h->prefix_codes != nullptr;                     // the new rows bring a code prefix (itts_gpt_set_code_prefix over n_new rows)
    int kmax = 0;
    if (pfx && (rc = check_prefix(h, n_new, gp, who, &kmax))) return rc;
    WsCarve wc;
    if ((rc = carve_ws(h, workspace, workspace_bytes, nseq, Sb, Tmax, 1, who, &wc))) return rc;
    const GptWs& w = wc.w;
    AdmitWs wa;
    // slots | limits (| prefix lengths; the admission cache then holds kmax more positions: itts_gpt_admit_prefix_workspace_bytes)
    if ((rc = carve_admit(h, admit_workspace, admit_bytes, n_new, S_new, pfx ? 3 : 2, who, &wa, kmax))) return rc;
    int* slots_dev = wa.ints;
    int* limits_dev = slots_dev + n_new;
    int* lens_dev = limits_dev + n_new;
    hipStream_t st = h->stream, cs = (hipStream_t)caller_stream;
    if ((rc = stream_enter(h, cs))) return rc;
    // the slots must be distinct finished utterances of the running batch (the loop that is suspended here has sized host_fin / host_map for nseq)
    HIP_TRY(hipMemcpyAsync(h->host_fin, w.finished, nseq, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = check_slots(slots, n_new, nseq, [&](int u) { return h->host_fin[u] != 0; }, who, "generating"))) return rc;
    HIP_TRY(hipMemcpyAsync(slots_dev, slots, (size_t)n_new * 4, hipMemcpyHostToDevice, st));
    if (h->align_out)                            // the previous occupant's alignment goes with its codes
        for (int i = 0; i < n_new; ++i)
            HIP_TRY(hipMemsetAsync(h->align_out + (size_t)slots[i] * align_row_elems(h), 0, align_row_elems(h) * sizeof(float), st));
    if (limited) HIP_TRY(hipMemcpyAsync(limits_dev, row_limits_new, (size_t)n_new * 4, hipMemcpyHostToDevice, st));
    if (n_penalty_ids > 0) HIP_TRY(hipMemcpyAsync(wa.w.pen_ids, penalty_ids, (size_t)n_penalty_ids * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(wa.w.pad, pad_lens, (size_t)n_new * 4, hipMemcpyDeviceToDevice, st));
    // (the limits are written here, after every check above has passed: a rejected call leaves the running rows' caps alone)
    hipLaunchKernelGGL(admit_state_kernel, dim3(n_new), dim3(256), 0, st, slots_dev, wa.w.pad, w.seen, w.finished, w.pad, w.row_step0, w.row_shift,
                       wa.w.pen_ids, n_penalty_ids, c.vocab, k - 1, S + k - 1 - S_new, (long long*)codes_out, gp.max_new_tokens,
                       (long long)c.stop_mel_token, limited ? (int*)h->row_limits : nullptr, limited ? limits_dev : nullptr, h->logp_model,
                       h->logp_sampled);
    if ((rc = admit_prefill(h, wa, prefix_embeds, n_new, S_new, st, !pfx))) return rc;
    if (pfx) {
        // the rows' prefixes on the admission workspace (its cache holds S_new + kmax positions), into the slots' code rows and seen sets; a row
        // with lens[i] codes joins at own step lens[i]: row_step0 = k - 1 - lens[i], row_shift = S + k - 1 - S_new - lens[i]
        HIP_TRY(hipMemcpyAsync(lens_dev, h->prefix_lens.data(), (size_t)n_new * 4, hipMemcpyHostToDevice, st));
        if ((rc = prefix_ingest(h, wa.w, w, n_new, S_new, s_bucket(S_new), wa.Ta, slots_dev, k - 1, S + k - 1 - S_new, (long long*)codes_out,
                                gp.max_new_tokens, lens_dev, kmax, st))) return rc;
    }
    // first token of every new row: sampled with the running batch's per-utterance state (seen set, finished flag, code row, uniform / RNG stream),
    // into column 0 of the slot's code row: the row's own step is 0 (with a code prefix: into the column after it)
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, wa.w.state, k - 1, S_new);
    {
        SampleArgs s = make_sample(h, w, gp, n_new, (long long*)codes_out, uniforms, nseq, false);
        s.logits = wa.w.logits; s.x_next = wa.w.x; s.step_ptr = wa.w.state; s.row_slot = slots_dev; s.adv_state = nullptr;
        if ((rc = launch_sample(s, st))) return rc;
    }
    admit_copy_kv(h, wa, w, slots_dev, n_new, S_new, Tmax, st, pfx ? lens_dev : nullptr);      // K / V of the prompt (and prefix) into the slots' cache rows
    // the running batch back in utterance order (uncompacted), the admitted rows' next-step inputs in their slots
    {
        int* src = h->host_map;
        for (int d = 0; d < nseq; ++d) src[d] = -1;
        for (int j = 0; j < (int)h->cur_slots.size(); ++j) src[h->cur_slots[j]] = j;
        HIP_TRY(hipMemcpyAsync(w.gather_src, src, (size_t)nseq * sizeof(int), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(regather_rows_kernel, dim3(nseq), dim3(256), 0, st, w.x, w.gather_src, w.qbuf, c.model_dim);
        hipLaunchKernelGGL(copy_rows_kernel, dim3(nseq), dim3(256), 0, st, w.qbuf, w.x, c.model_dim);
        hipLaunchKernelGGL(place_rows_kernel, dim3(n_new), dim3(256), 0, st, wa.w.x, slots_dev, w.x, c.model_dim);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = stream_leave(h, cs))) return rc;
    h->cur_slots.resize(nseq);
    for (int i = 0; i < nseq; ++i) h->cur_slots[i] = i;
    h->cur_mapped = false;
    su.admitted = true;
    return ITTS_OK;
}

// ---- beam search / beam-sample ------------------------------------------------------------------------------------
// The beams of an utterance share ONE copy of the prompt's K/V (cache row b*nb, written by a prefill over the B unique
// prompts): prompt positions map there, generated positions to the row's own cache row.
__global__ void beam_init_kernel(int* row_map0, float* beam_scores, float* worst, int* n_hyps, unsigned char* done, int nseq, int nb,
                                 int Tmax, int S) {
    const int i = blockIdx.x;
    for (int t = threadIdx.x; t < Tmax; t += blockDim.x) row_map0[(size_t)i * Tmax + t] = t < S ? (i / nb) * nb : i;
    if (threadIdx.x == 0) {
        beam_scores[i] = (i % nb == 0) ? 0.f : -1e9f;             // generation_utils.py:3408-3410
        if (i % nb == 0) { worst[i / nb] = 1e9f; n_hyps[i / nb] = 0; done[i / nb] = 0; }
    }
}

static BeamArgs make_beam(itts_gpt* h, const GptWs& w, const itts_gen_params& gp, int B, int nb, int S, int Tmax, const double* uniforms) {
    const itts_gpt_config& c = h->cfg;
    BeamArgs a{};
    a.logits = w.logits; a.seen[0] = w.seen; a.seen[1] = w.seen2; a.row_map[0] = w.row_map[0]; a.row_map[1] = w.row_map[1];
    a.beam_scores = w.beam_scores; a.next_scores = w.next_scores; a.next_tokens = w.next_tokens; a.next_indices = w.next_indices;
    a.hyps = w.hyps; a.n_hyps = w.n_hyps; a.worst = w.worst; a.done = w.done; a.hist_tok = w.hist_tok; a.hist_par = w.hist_par;
    a.surv_idx = w.surv_idx; a.surv_val = w.surv_val; a.surv_n = w.surv_n;
    a.step_ptr = w.state; a.uniforms = uniforms; a.seed = gp.seed; a.B = B; a.nb = nb; a.V = c.vocab; a.max_new = gp.max_new_tokens;
    a.Tmax = Tmax; a.S = S; a.do_sample = gp.do_sample; a.top_k = gp.top_k;
    a.min_keep = gp.min_tokens_to_keep < 1 ? 1 : gp.min_tokens_to_keep;
    a.top_p = gp.top_p; a.temperature = gp.temperature; a.rep_penalty = gp.repetition_penalty; a.length_penalty = gp.length_penalty;
    a.typical_mass = gp.typical_mass;
    a.stop_token = c.stop_mel_token; a.mel_emb = h->mel_emb; a.mel_pos = h->mel_pos; a.x_next = w.x; a.D = c.model_dim;
    a.pos_offset = gp.pos_offset; a.n_mel_pos = c.n_mel_pos;
    a.seed_ptr = (const unsigned long long*)(w.state + 4);
    a.grp_table = (const GroupSampling*)h->group_sampling;      // (the callers have checked that it covers the call's utterances)
    a.filt = h->filt(); a.filt_table = h->filt_table();
    return a;
}

// never search a batch with settings meant for another one
static int check_group_table(const itts_gpt* h, int n_utts, const char* who) {
    if (h->group_sampling && h->group_sampling_n != n_utts) {
        itts_set_error("%s: the installed group sampling table has %d entries, the call %d utterances (itts_gpt_set_group_sampling)", who, h->group_sampling_n, n_utts);
        return ITTS_ERR_STATE;
    }
    return ITTS_OK;
}

// shifted: a group has been admitted into the session (itts_gpt_admit_beam_groups) -- the QKV epilogue and the attention read the per-row shifts
static int decode_step_beam(itts_gpt* h, const GptWs& w, const BeamArgs& ba, int nseq, int Tmax, hipStream_t st, bool shifted = false) {
    bool pending = false;
    float* xc = w.x;
    int rc = run_layers(h, w, nseq, 1, Tmax, false, w.state + 1, w.pad, &pending, st, true, 1, nullptr, &xc, shifted ? w.row_shift : nullptr);
    if (rc) return rc;
    if ((rc = run_head(h, w, nseq, 1, 0, pending, st, xc))) return rc;
    if ((rc = launch_beam_step(ba, st))) return rc;
    BeamArgs bb = ba;
    bb.adv_state = w.state;                     // the apply kernel's last block advances step / pos
    return launch_beam_apply(bb, st);
}

// the search state of every group to the caller's buffers (the host finalises groups as they finish)
static int beam_copy_out(const GptWs& w, int B, int nseq, int max_new, int32_t* hist_tok_out, int32_t* hist_par_out, float* beam_scores_out,
                         float* hyps_out, int32_t* n_hyps_out, uint8_t* done_out, hipStream_t st) {
    HIP_TRY(hipMemcpyAsync(hist_tok_out, w.hist_tok, (size_t)max_new * nseq * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(hist_par_out, w.hist_par, (size_t)max_new * nseq * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(beam_scores_out, w.beam_scores, (size_t)nseq * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(hyps_out, w.hyps, (size_t)B * BEAM_MAX * sizeof(BeamHyp), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(n_hyps_out, w.n_hyps, (size_t)B * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(done_out, w.done, (size_t)B, hipMemcpyDeviceToDevice, st));
    return ITTS_OK;
}

// a beam session's kernels: every group on its own step, its rows on their own positions, its own cap (see "beam sessions" below)
static BeamArgs make_beam_session(itts_gpt* h, const GptWs& w, const itts_gen_params& gp, int B, int nb, int S, int Tmax) {
    BeamArgs a = make_beam(h, w, gp, B, nb, S, Tmax, nullptr);
    a.row_step0 = w.row_step0; a.row_shift = w.row_shift; a.grp_cap = w.grp_cap;
    return a;
}

static int check_no_row_table(const itts_gpt* h, const char* who) {
    if (h->row_sampling) {
        itts_set_error("%s: a per-slot sampling table is installed (itts_gpt_set_row_sampling): the beam kernels take one set of sampling settings per call", who);
        return ITTS_ERR_STATE;
    }
    return ITTS_OK;
}

// what the two beam entries check of their sizes alike; session: the chunk entry, whose parameters must name the beams as well
static int beam_check_sizes(const itts_gpt* h, const itts_gen_params& gp, int B, int nb, int S, int n_penalty_ids, bool session, const char* who) {
    const itts_gpt_config& c = h->cfg;
    if (B <= 0 || nb < 2 || nb > BEAM_MAX || S <= 0 || gp.max_new_tokens <= 0 || (session && gp.num_beams != nb)) { itts_set_error("%s: bad sizes", who); return ITTS_ERR_ARG; }
    if (int rc = check_group_table(h, B, who)) return rc;
    if (int rc = refuse_prefix(h, who)) return rc;
    if (h->filt_on && !h->ftab_n && h->filt_ngram > 0) {
        itts_set_error("%s: no_repeat_ngram_size = %d is installed (itts_gpt_set_logits_filters): the n-gram filter serves num_beams = 1 only "
                       "(a beam's history is not kept per row)", who, h->filt_ngram);
        return ITTS_ERR_ARG;
    }
    if (int rc = check_filter_table_beam(h, B, who)) return rc;
    if (gp.max_new_tokens + gp.pos_offset > c.n_mel_pos + 1) { itts_set_error("%s: max_new_tokens exceeds the mel position table", who); return ITTS_ERR_ARG; }
    if (int rc = check_penalty_ids(n_penalty_ids, who)) return rc;
    if (session && ((size_t)B * nb * c.heads > 2147483647u / 4 || S > 65535)) { itts_set_error("%s: batch too large", who); return ITTS_ERR_ARG; }
    return ITTS_OK;
}

// The start of a beam loop: the search state as beam_init leaves it, the prefill of the B unique prompts (the nb rows of an utterance carry the
// same prompt, repeat_interleave), beam step 0 from the one logits row per utterance; leaves the counters at (step 1, position S) and ev_t0
// recorded before the prefill.  group_caps (host [B]): a session's per-group caps -- its per-row tables are initialised with them; null: one-shot.
static int beam_start(itts_gpt* h, const GptWs& w, const BeamArgs& ba, const itts_gen_params& gp, const float* prefix_embeds, const int32_t* pad_lens,
                      const int32_t* penalty_ids, int n_penalty_ids, const int* group_caps, hipStream_t st) {
    const itts_gpt_config& c = h->cfg;
    const int B = ba.B, nb = ba.nb, nseq = B * nb, S = ba.S, Tmax = ba.Tmax, max_new = gp.max_new_tokens;
    int rc;
    HIP_TRY(hipMemsetAsync(w.seen, 0, (size_t)nseq * c.vocab, st));
    HIP_TRY(hipMemsetAsync(w.seen2, 0, (size_t)nseq * c.vocab, st));
    HIP_TRY(hipMemsetAsync(w.hist_tok, 0, (size_t)max_new * nseq * 4, st));
    HIP_TRY(hipMemsetAsync(w.hist_par, 0, (size_t)max_new * nseq * 4, st));
    HIP_TRY(hipMemsetAsync(w.hyps, 0, (size_t)B * BEAM_MAX * sizeof(BeamHyp), st));
    if (group_caps) {
        HIP_TRY(hipMemsetAsync(w.row_step0, 0, (size_t)nseq * 4, st));
        HIP_TRY(hipMemsetAsync(w.row_shift, 0, (size_t)nseq * 4, st));
        HIP_TRY(hipMemcpyAsync(w.grp_cap, group_caps, (size_t)B * 4, hipMemcpyHostToDevice, st));
    }
    if (pad_lens) HIP_TRY(hipMemcpyAsync(w.pad, pad_lens, (size_t)nseq * 4, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemsetAsync(w.pad, 0, (size_t)nseq * 4, st));
    if (n_penalty_ids > 0) {
        HIP_TRY(hipMemcpyAsync(w.pen_ids, penalty_ids, (size_t)n_penalty_ids * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(mark_seen_kernel, dim3(nseq), dim3(64), 0, st, w.seen, w.pen_ids, n_penalty_ids, c.vocab);
    }
    hipLaunchKernelGGL(beam_init_kernel, dim3(nseq), dim3(256), 0, st, w.row_map[0], w.beam_scores, w.worst, w.n_hyps, w.done, nseq, nb, Tmax, S);
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 0, 0);
    hipLaunchKernelGGL(set_seed_kernel, dim3(1), dim3(1), 0, st, w.state, (unsigned long long)gp.seed);
    const size_t row_bytes = (size_t)S * c.model_dim * 4;           // (per sequence row, beams adjacent: the B unique prompts are prefilled)
    HIP_TRY(hipMemcpy2DAsync(w.x, row_bytes, prefix_embeds, row_bytes * nb, row_bytes, B, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGetLastError());

    HIP_TRY(hipEventRecord(h->ev_t0, st));
    bool pending = false;
    if ((rc = run_layers(h, w, B, S, Tmax, true, w.state + 1, w.pad, &pending, st, false, nb))) return rc;
    if ((rc = run_head(h, w, B, S, S - 1, pending, st))) return rc;
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 0, S);
    BeamArgs ba0 = ba;
    ba0.logits_shared = 1;                       // one logits row per utterance after the shared prefill
    if ((rc = launch_beam_step(ba0, st))) return rc;
    if ((rc = launch_beam_apply(ba, st))) return rc;
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 1, S);
    return ITTS_OK;
}

extern "C" int itts_gpt_generate_beam(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int n_utts, int num_beams,
                                      int S, const itts_gen_params* gpp, const int32_t* penalty_ids, int n_penalty_ids,
                                      const double* uniforms, int32_t* hist_tok_out, int32_t* hist_par_out, float* beam_scores_out,
                                      float* hyps_out, int32_t* n_hyps_out, uint8_t* done_out, int32_t* n_steps_out,
                                      void* workspace, size_t workspace_bytes, int use_graph, void* caller_stream) {
    const char* who = "gpt_generate_beam";
    if (!h || !prefix_embeds || !gpp || !hist_tok_out || !hist_par_out || !beam_scores_out || !hyps_out || !n_hyps_out || !done_out ||
        !n_steps_out || !workspace) { itts_set_error("gpt_generate_beam: null pointer"); return ITTS_ERR_ARG; }
    if (!h->finalized) { itts_set_error("gpt_generate_beam: call itts_gpt_finalize first"); return ITTS_ERR_STATE; }
    if (int rct = check_no_row_table(h, who)) return rct;
    if (int rcs = refuse_scores_beam(h, who)) return rcs;
    if (int rca = refuse_alignment_beam(h, who)) return rca;
    ItDevGuard dg(h->device);
    if (int rcd = check_same_device(h, prefix_embeds, workspace, who)) return rcd;
    const itts_gen_params gp = *gpp;
    const int nb = num_beams, B = n_utts, nseq = B * nb, max_new = gp.max_new_tokens;
    int rc;
    if ((rc = beam_check_sizes(h, gp, B, nb, S, n_penalty_ids, false, who))) return rc;
    const int Sb = s_bucket(S), Tmax = Sb + max_new;
    WsCarve wc;
    if ((rc = carve_ws(h, workspace, workspace_bytes, nseq, Sb, Tmax, nb, who, &wc))) return rc;
    const GptWs& w = wc.w;
    h->susp = itts_gpt::Suspended{};                                    // (whatever loop was suspended on this handle is over; this call leaves none)
    hipStream_t st = h->stream, cs = (hipStream_t)caller_stream;
    if ((rc = grow_host_fin(h, nseq))) return rc;
    if ((rc = stream_enter(h, cs))) return rc;
    const BeamArgs ba = make_beam(h, w, gp, B, nb, S, Tmax, uniforms);
    if ((rc = beam_start(h, w, ba, gp, prefix_embeds, pad_lens, penalty_ids, n_penalty_ids, nullptr, st))) return rc;
    HIP_TRY(hipEventRecord(h->ev_t1, st));

    int steps = 1;
    hipGraphExec_t exec = nullptr;
    auto step = [&] { return decode_step_beam(h, w, ba, nseq, Tmax, st); };
    if (use_graph && max_new > 1) {
        itts_gpt::GraphEntry key = graph_key(wc.base, nseq, nb, Sb, Tmax, S, gp);
        key.uniforms = uniforms;
        key.aux3 = (const void*)h->group_sampling;                    // the step reads its groups' settings from this table (its contents may differ)
        if ((rc = step_graph(h, key, who, step, &exec))) return rc;
    }
    // the reference loop stops when every utterance is done (checked right after the scorer) or at max_length
    auto all_done = [&](bool* out) -> int {
        HIP_TRY(hipMemcpyAsync(h->host_fin, w.done, B, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bool all = true;
        for (int i = 0; i < B; ++i) all = all && h->host_fin[i];
        *out = all;
        return ITTS_OK;
    };
    bool fin = false;
    if ((rc = all_done(&fin))) return rc;
    while (!fin && steps < max_new) {
        if (exec) { HIP_TRY(hipGraphLaunch(exec, st)); }
        else if ((rc = step())) return rc;
        ++steps;
        // finished utterances are frozen on the device (their block returns early), so a late check only costs idle
        // steps; the host reports min(steps, the step at which the last utterance finished) like the reference loop
        if (steps % 4 == 0 && (rc = all_done(&fin))) return rc;
    }
    HIP_TRY(hipEventRecord(h->ev_t2, st));
    if ((rc = beam_copy_out(w, B, nseq, max_new, hist_tok_out, hist_par_out, beam_scores_out, hyps_out, n_hyps_out, done_out, st))) return rc;
    if ((rc = leave_timed(h, cs, steps))) return rc;
    *n_steps_out = steps;
    return ITTS_OK;
}

// ---- beam sessions: the beam loop suspended between calls, finished groups replaced by new utterances --------------------------------------
// A beam GROUP is one utterance's nb adjacent sequence rows -- the slot of a beam session.  The loop of itts_gpt_generate_beam, resumable
// (itts_gpt_generate_beam_chunk) and with every group on its OWN step and its rows on their OWN positions: row_step0[b*nb] is the session step of
// the group's step 0, row_shift[row] the distance between the session's position counter and the row's own position, grp_cap[b] the group's cap on
// own steps.  The beam kernels index the history, gen_len / length penalty, the mel position and the RNG stream by the own step; the QKV epilogue
// and attn_kernel<.., RMAP = true> find the row's own position through row_shift as on the non-beam path.  The seen / row-map parity stays on the
// session step: an admission initialises both buffers, runs the group's first beam step under the parity of session step k - 1 (which writes the
// buffers step k reads) and so hands the group over in the state a group of the first batch has after its step 0.  Nothing a group computes
// depends on the session step it joined at, so it finds, bit for bit, the hypotheses it finds in a batch decoded from step 0
// (tests/test_gpu_beam_session.py).  A group past its cap or long done idles: scores, hypotheses and history keep their values, its rows emit the
// stop token inside their own cache rows (the QKV epilogue drops positions past Tmax - 1, the row map is written below Tmax only).
__global__ void beam_admit_state_kernel(const int* __restrict__ slots, const int* __restrict__ pad_new, const int* __restrict__ caps_new, int nb, int V,
                                        int Tmax, int S_new, int max_new, int nseq, int step0, int shift, const int* __restrict__ pen_ids, int n_ids,
                                        unsigned char* seen0, unsigned char* seen1, int* map0, int* map1, float* beam_scores, float* worst, int* n_hyps,
                                        unsigned char* done, BeamHyp* hyps, int* hist_tok, int* hist_par, int* pad, int* row_step0, int* row_shift,
                                        int* grp_cap) {
    const int g = blockIdx.x / nb, j = blockIdx.x - g * nb, b = slots[g], i = b * nb + j;
    unsigned char* s0 = seen0 + (size_t)i * V;
    unsigned char* s1 = seen1 + (size_t)i * V;
    for (int c = threadIdx.x; c < V; c += blockDim.x) { s0[c] = 0; s1[c] = 0; }
    for (int t = threadIdx.x; t < Tmax; t += blockDim.x) {
        const int r = t < S_new ? b * nb : i;                 // prompt positions: the group's shared prompt row; generated ones: the row itself
        map0[(size_t)i * Tmax + t] = r; map1[(size_t)i * Tmax + t] = r;
    }
    for (int s = threadIdx.x; s < max_new; s += blockDim.x) { hist_tok[(size_t)s * nseq + i] = 0; hist_par[(size_t)s * nseq + i] = 0; }
    __syncthreads();
    if ((int)threadIdx.x < n_ids) {
        const int id = pen_ids[threadIdx.x];
        if (id >= 0 && id < V) { s0[id] = 1; s1[id] = 1; }
    }
    if (threadIdx.x == 0) {
        beam_scores[i] = j == 0 ? 0.f : -1e9f;                // generation_utils.py:3408-3410
        pad[i] = pad_new[g]; row_step0[i] = step0; row_shift[i] = shift;
        if (j == 0) {
            worst[b] = 1e9f; n_hyps[b] = 0; done[b] = 0; grp_cap[b] = caps_new[g];
            for (int q = 0; q < BEAM_MAX; ++q) hyps[(size_t)b * BEAM_MAX + q] = BeamHyp{0.f, 0, 0, 0};
        }
    }
}

extern "C" int itts_gpt_generate_beam_chunk(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int n_utts, int num_beams, int S,
                                            const itts_gen_params* gpp, const int32_t* penalty_ids, int n_penalty_ids, const int32_t* group_caps,
                                            int32_t* hist_tok_out, int32_t* hist_par_out, float* beam_scores_out, float* hyps_out,
                                            int32_t* n_hyps_out, uint8_t* done_out, int32_t step_limit, int32_t* n_steps_out, void* workspace,
                                            size_t workspace_bytes, int use_graph, void* caller_stream) {
    const char* who = "gpt_generate_beam_chunk";
    const bool resume = prefix_embeds == nullptr;
    if (!h || !gpp || !hist_tok_out || !hist_par_out || !beam_scores_out || !hyps_out || !n_hyps_out || !done_out || !n_steps_out || !workspace) {
        itts_set_error("gpt_generate_beam_chunk: null pointer"); return ITTS_ERR_ARG;
    }
    if (!h->finalized) { itts_set_error("gpt_generate_beam_chunk: call itts_gpt_finalize first"); return ITTS_ERR_STATE; }
    if (int rct = check_no_row_table(h, who)) return rct;
    if (int rcs = refuse_scores_beam(h, who)) return rcs;
    if (int rca = refuse_alignment_beam(h, who)) return rca;
    ItDevGuard dg(h->device);
    if (int rcd = check_same_device(h, resume ? (const void*)hist_tok_out : (const void*)prefix_embeds, workspace, who)) return rcd;
    const itts_gen_params gp = *gpp;
    const int nb = num_beams, B = n_utts, nseq = B * nb, max_new = gp.max_new_tokens;
    itts_gpt::Suspended& su = h->susp;
    int rc;
    if ((rc = beam_check_sizes(h, gp, B, nb, S, n_penalty_ids, true, who))) return rc;
    if (resume && (su.kind != itts_gpt::Suspended::BEAM_GROUPS || su.n_utts != B || su.nb != nb || su.S != S || su.ws != workspace || !gp_same(su.gp, gp))) {
        itts_set_error("gpt_generate_beam_chunk: resume without a matching first chunk (same workspace, n_utts, num_beams, S, generation parameters)");
        return ITTS_ERR_STATE;
    }
    // The first call's step counter is bounded by max_new_tokens.  A resumed session's is not: every group is bounded by its OWN step, and everything
    // in the workspace (history rows, row map, cache rows) is indexed by own steps / own positions, so the workspace of one batch serves a session of
    // any length.
    if (step_limit < 1 || (step_limit > max_new && !resume)) step_limit = max_new;
    const int Sb = s_bucket(S), Tmax = Sb + max_new;
    WsCarve wc;
    if ((rc = carve_ws(h, workspace, workspace_bytes, nseq, Sb, Tmax, nb, who, &wc))) return rc;
    const GptWs& w = wc.w;
    hipStream_t st = h->stream, cs = (hipStream_t)caller_stream;
    if ((rc = grow_host_fin(h, nseq))) return rc;
    if ((rc = stream_enter(h, cs))) return rc;
    const BeamArgs ba = make_beam_session(h, w, gp, B, nb, S, Tmax);
    int steps = resume ? su.steps : 1;
    if (!resume) {
        su = itts_gpt::Suspended{};                                     // (whatever loop was suspended on this handle is over)
        su.step0.assign(B, 0);
        su.cap.assign(B, max_new);
        if (group_caps)
            for (int b = 0; b < B; ++b) su.cap[b] = group_caps[b] < 1 ? 1 : group_caps[b] > max_new ? max_new : group_caps[b];
        if ((rc = beam_start(h, w, ba, gp, prefix_embeds, pad_lens, penalty_ids, n_penalty_ids, su.cap.data(), st))) return rc;
    } else {
        HIP_TRY(hipEventRecord(h->ev_t0, st));
    }
    HIP_TRY(hipEventRecord(h->ev_t1, st));

    hipGraphExec_t exec = nullptr;
    auto step = [&] { return decode_step_beam(h, w, ba, nseq, Tmax, st, su.admitted); };
    if (use_graph && max_new > 1) {
        itts_gpt::GraphEntry key = graph_key(wc.base, nseq, nb, Sb, Tmax, S, gp);
        key.aux0 = w.row_step0;                                         // the session's step: per-group tables in the beam kernels
        key.aux2 = su.admitted ? (const void*)w.row_shift : nullptr;
        key.aux3 = (const void*)h->group_sampling;
        if ((rc = step_graph(h, key, who, step, &exec))) return rc;
    }
    while (steps < step_limit) {
        if (exec) { HIP_TRY(hipGraphLaunch(exec, st)); }
        else if ((rc = step())) return rc;
        ++steps;
        if (steps % 4 == 0 && steps < step_limit) {
            // groups that are done or have used up their cap idle on the device; enough of them (or all) end the call
            HIP_TRY(hipMemcpyAsync(h->host_fin, w.done, B, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            int fin = 0;
            for (int b = 0; b < B; ++b) fin += (h->host_fin[b] || steps - su.step0[b] >= su.cap[b]) ? 1 : 0;
            if (fin == B) break;
            if (h->chunk_return_finished > 0 && fin >= h->chunk_return_finished) break;          // slots to refill
        }
    }
    HIP_TRY(hipEventRecord(h->ev_t2, st));
    if ((rc = beam_copy_out(w, B, nseq, max_new, hist_tok_out, hist_par_out, beam_scores_out, hyps_out, n_hyps_out, done_out, st))) return rc;
    if ((rc = leave_timed(h, cs, steps))) return rc;
    su.kind = itts_gpt::Suspended::BEAM_GROUPS; su.ws = workspace; su.n_utts = B; su.nb = nb; su.S = S; su.gp = gp; su.steps = steps;
    *n_steps_out = steps;
    return ITTS_OK;
}

extern "C" size_t itts_gpt_admit_beam_workspace_bytes(const itts_gpt* h, int n_new, int S_new) {
    if (!h || n_new <= 0 || S_new <= 0) return 0;
    const int Sb = s_bucket(S_new);
    return carve(h->cfg, nullptr, n_new, Sb, Sb + 8).total + a256((size_t)n_new * 12) + 512;
}

extern "C" int itts_gpt_admit_beam_groups(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, const int32_t* slots, int n_new, int S_new,
                                          const int32_t* group_caps_new, const itts_gen_params* gpp, const int32_t* penalty_ids, int n_penalty_ids,
                                          void* workspace, size_t workspace_bytes, void* admit_workspace, size_t admit_bytes, void* caller_stream) {
    const char* who = "gpt_admit_beam_groups";
    if (!h || !prefix_embeds || !pad_lens || !slots || !gpp || !workspace || !admit_workspace) { itts_set_error("gpt_admit_beam_groups: null pointer"); return ITTS_ERR_ARG; }
    if (!h->finalized) { itts_set_error("gpt_admit_beam_groups: call itts_gpt_finalize first"); return ITTS_ERR_STATE; }
    if (int rct = check_no_row_table(h, who)) return rct;
    if (int rcs = refuse_scores_beam(h, who)) return rcs;
    if (int rca = refuse_alignment_beam(h, who)) return rca;
    if (int rcp = refuse_prefix(h, who)) return rcp;
    ItDevGuard dg(h->device);
    if (int rcd = check_same_device(h, prefix_embeds, workspace, who)) return rcd;
    const itts_gpt_config& c = h->cfg;
    const itts_gen_params gp = *gpp;
    itts_gpt::Suspended& su = h->susp;
    if (su.kind != itts_gpt::Suspended::BEAM_GROUPS || su.ws != workspace || !gp_same(su.gp, gp)) {
        itts_set_error("gpt_admit_beam_groups: no suspended itts_gpt_generate_beam_chunk loop on this workspace with these generation parameters");
        return ITTS_ERR_STATE;
    }
    const int B = su.n_utts, nb = su.nb, nseq = B * nb, S = su.S, k = su.steps, max_new = gp.max_new_tokens;
    int rc;
    if ((rc = check_group_table(h, B, who))) return rc;
    if ((rc = check_filter_table_beam(h, B, who))) return rc;
    const int Sb = s_bucket(S), Tmax = Sb + max_new;
    if (S_new < 1 || S_new > Sb) {      // a cache row holds Sb prompt positions + max_new_tokens generated ones
        itts_set_error("gpt_admit_beam_groups: S_new = %d outside 1 .. %d (the session's prompt bucket)", S_new, Sb);
        return ITTS_ERR_ARG;
    }
    if (n_new < 1 || n_new > B) { itts_set_error("gpt_admit_beam_groups: n_new = %d outside 1 .. %d", n_new, B); return ITTS_ERR_ARG; }
    if ((rc = check_penalty_ids(n_penalty_ids, who))) return rc;
    WsCarve wc;
    if ((rc = carve_ws(h, workspace, workspace_bytes, nseq, Sb, Tmax, nb, who, &wc))) return rc;
    const GptWs& w = wc.w;
    AdmitWs wa;
    if ((rc = carve_admit(h, admit_workspace, admit_bytes, n_new, S_new, 3, who, &wa))) return rc;      // slots | prompt cache rows | caps
    int* slots_dev = wa.ints;
    int* kvrows_dev = slots_dev + n_new;
    int* caps_dev = kvrows_dev + n_new;
    hipStream_t st = h->stream, cs = (hipStream_t)caller_stream;
    if ((rc = stream_enter(h, cs))) return rc;
    // the slots must be distinct groups of the session that are done or at their cap; a rejected call touches nothing of the running state
    HIP_TRY(hipMemcpyAsync(h->host_fin, w.done, B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = check_slots(slots, n_new, B, [&](int u) { return h->host_fin[u] || k - su.step0[u] >= su.cap[u]; }, who, "searching"))) return rc;
    std::vector<int> ints((size_t)3 * n_new);
    for (int i = 0; i < n_new; ++i) {
        const int u = slots[i], cap = group_caps_new ? group_caps_new[i] : max_new;
        ints[i] = u; ints[n_new + i] = u * nb; ints[2 * n_new + i] = cap < 1 ? 1 : cap > max_new ? max_new : cap;
    }
    HIP_TRY(hipMemcpyAsync(slots_dev, ints.data(), (size_t)3 * n_new * 4, hipMemcpyHostToDevice, st));
    if (n_penalty_ids > 0) HIP_TRY(hipMemcpyAsync(wa.w.pen_ids, penalty_ids, (size_t)n_penalty_ids * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(wa.w.pad, pad_lens, (size_t)n_new * 4, hipMemcpyDeviceToDevice, st));
    if ((rc = admit_prefill(h, wa, prefix_embeds, n_new, S_new, st))) return rc;      // the n_new unique prompts
    admit_copy_kv(h, wa, w, kvrows_dev, n_new, S_new, Tmax, st);      // ... into the group's shared prompt row (cache row slot * nb)
    // the groups' search state as beam_init leaves it, under the session's counters: own step 0 = session step k - 1, and the session's position
    // counter (S + k - 1 at the next step) runs S + k - 1 - S_new ahead of the rows' own positions
    const int step0 = k - 1, shift = S + k - 1 - S_new;
    hipLaunchKernelGGL(beam_admit_state_kernel, dim3(n_new * nb), dim3(256), 0, st, slots_dev, wa.w.pad, caps_dev, nb, c.vocab, Tmax, S_new, max_new, nseq,
                       step0, shift, wa.w.pen_ids, n_penalty_ids, w.seen, w.seen2, w.row_map[0], w.row_map[1], w.beam_scores, w.worst, w.n_hyps, w.done,
                       w.hyps, w.hist_tok, w.hist_par, w.pad, w.row_step0, w.row_shift, w.grp_cap);
    // the groups' first beam step (own step 0) from the shared logits row, under the parity of session step k - 1: it writes the seen / row-map
    // buffers session step k reads, and the nb next-step input rows straight into the session's x rows
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, wa.w.state, k - 1, S_new);
    hipLaunchKernelGGL(set_seed_kernel, dim3(1), dim3(1), 0, st, wa.w.state, (unsigned long long)gp.seed);
    {
        BeamArgs a = make_beam_session(h, w, gp, B, nb, S, Tmax);
        a.logits = wa.w.logits; a.logits_shared = 1; a.step_ptr = wa.w.state; a.seed_ptr = (const unsigned long long*)(wa.w.state + 4);
        a.grp_map = slots_dev; a.n_grp = n_new; a.adv_state = nullptr;
        if ((rc = launch_beam_step(a, st))) return rc;
        if ((rc = launch_beam_apply(a, st))) return rc;
    }
    HIP_TRY(hipGetLastError());
    if ((rc = stream_leave(h, cs))) return rc;                          // (synchronises: `ints` is pageable host memory)
    for (int i = 0; i < n_new; ++i) { su.step0[slots[i]] = step0; su.cap[slots[i]] = ints[2 * n_new + i]; }
    su.admitted = true;                                                 // the next chunk call takes the step graph that reads the row shifts
    return ITTS_OK;
}

// Row compaction of ragged decode batches: on by default; granularity = rows per bucket (the decode graph is captured once per bucket).
extern "C" int itts_gpt_set_compaction(itts_gpt* h, int enable, int granularity) {
    if (!h) { itts_set_error("gpt_set_compaction: null"); return ITTS_ERR_ARG; }
    h->compact = enable != 0;
    if (granularity > 0) h->compact_gran = granularity;
    return ITTS_OK;
}

// In-flight batching: a chunk call returns early -- at one of the finished-flag checks the loop makes every 8 steps anyway -- once at least
// `finished_rows` utterances of the batch have finished (counting the ones that had finished before the call), so the caller can refill their slots
// (itts_gpt_admit_rows) without polling in short chunks.  0 = off (run to step_limit).
extern "C" int itts_gpt_set_chunk_return(itts_gpt* h, int finished_rows) {
    if (!h || finished_rows < 0) { itts_set_error("gpt_set_chunk_return: bad args"); return ITTS_ERR_ARG; }
    h->chunk_return_finished = finished_rows;
    return ITTS_OK;
}

// Per-utterance caps on the generated tokens for the following itts_gpt_generate / _chunk calls whose batch has exactly n utterances
// (a batch merges requests that carry their own max_mel_tokens): limits is a DEVICE int32 [n] the caller keeps alive; null clears.
// Per-token log-probabilities (what output_scores / compute_transition_scores give in the vendored generation utils): caller-owned DEVICE f32
// arrays [n][max_new] the sampler writes next to the tokens; sticky like the row limits; NULL, NULL, 0, 0 clears.
extern "C" int itts_gpt_set_token_scores(itts_gpt* h, float* logp_model, float* logp_sampled, int n, int max_new) {
    if (!h || (logp_model == nullptr) != (logp_sampled == nullptr) || (logp_model && (n <= 0 || max_new <= 0))) {
        itts_set_error("gpt_set_token_scores: logp_model and logp_sampled are given together with n, max_new > 0, or both NULL");
        return ITTS_ERR_ARG;
    }
    h->logp_model = logp_model;
    h->logp_sampled = logp_sampled;
    h->scores_n = logp_model ? n : 0;
    h->scores_max_new = logp_model ? max_new : 0;
    return ITTS_OK;
}

// Alignment export (no counterpart in the vendored generation utils beyond `output_attentions`, which returns every layer's whole matrix): the
// decode steps write the softmax weights of a few (layer, head) pairs over each utterance's text span; sticky; all-NULL / zero uninstalls.
extern "C" int itts_gpt_set_alignment(itts_gpt* h, const int32_t* pairs, int n_pairs, const int32_t* span, float* out, int n, int max_new,
                                      int text_cap) {
    if (!h) { itts_set_error("gpt_set_alignment: null handle"); return ITTS_ERR_ARG; }
    if (!pairs && !span && !out && n_pairs == 0 && n == 0 && max_new == 0 && text_cap == 0) {
        h->align_span = nullptr; h->align_out = nullptr;
        h->align_n_pairs = h->align_n = h->align_max_new = h->align_text_cap = 0;
        return ITTS_OK;             // (a step without the export is keyed by epoch 0 and null arrays, whatever was installed before)
    }
    if (!pairs || !span || !out || n <= 0 || max_new <= 0) {
        itts_set_error("gpt_set_alignment: pairs, span and out are given together with n, max_new > 0, or everything NULL / 0");
        return ITTS_ERR_ARG;
    }
    if (n_pairs < 1 || n_pairs > ALIGN_MAX_PAIRS) { itts_set_error("gpt_set_alignment: n_pairs = %d outside 1 .. %d", n_pairs, ALIGN_MAX_PAIRS); return ITTS_ERR_ARG; }
    if (text_cap < 4 || text_cap > ALIGN_MAX_TEXT || (text_cap & 3)) {
        itts_set_error("gpt_set_alignment: text_cap = %d must be a multiple of 4 in 4 .. %d", text_cap, ALIGN_MAX_TEXT);
        return ITTS_ERR_ARG;
    }
    for (int k = 0; k < n_pairs; ++k) {
        const int l = pairs[2 * k], hd = pairs[2 * k + 1];
        if (l < 0 || l >= h->cfg.layers || hd < 0 || hd >= h->cfg.heads) {
            itts_set_error("gpt_set_alignment: pair %d = (layer %d, head %d) outside %d layers x %d heads", k, l, hd, h->cfg.layers, h->cfg.heads);
            return ITTS_ERR_ARG;
        }
        for (int j = 0; j < k; ++j)
            if (pairs[2 * j] == l && pairs[2 * j + 1] == hd) { itts_set_error("gpt_set_alignment: pair (layer %d, head %d) is listed twice", l, hd); return ITTS_ERR_ARG; }
    }
    for (int k = 0; k < n_pairs; ++k) { h->align_pairs[k][0] = pairs[2 * k]; h->align_pairs[k][1] = pairs[2 * k + 1]; }
    h->align_n_pairs = n_pairs; h->align_span = span; h->align_out = out; h->align_n = n; h->align_max_new = max_new; h->align_text_cap = text_cap;
    // What a captured step bakes in of the export beside the two arrays (which are in the key themselves): which launches exist (the pair
    // list) and their sizes.  The same list and sizes again -- the next call or session of a caller that installs per call -- keep the epoch,
    // so the steps captured under the previous install replay; anything else gets a new one.
    int keyed[4 + 2 * ALIGN_MAX_PAIRS] = {n_pairs, n, max_new, text_cap};
    for (int k = 0; k < n_pairs; ++k) { keyed[4 + 2 * k] = pairs[2 * k]; keyed[5 + 2 * k] = pairs[2 * k + 1]; }
    if (memcmp(keyed, h->align_keyed, sizeof(keyed)) != 0) {
        memcpy(h->align_keyed, keyed, sizeof(keyed));
        ++h->align_epoch;
    }
    return ITTS_OK;
}

extern "C" int itts_gpt_set_row_limits(itts_gpt* h, const int32_t* limits, int n) {
    if (!h || (limits && n <= 0)) { itts_set_error("gpt_set_row_limits: bad args"); return ITTS_ERR_ARG; }
    h->row_limits = limits;
    h->row_limits_n = limits ? n : 0;
    return ITTS_OK;
}

extern "C" int itts_gpt_set_code_prefix(itts_gpt* h, const int64_t* codes, const int32_t* lens, int n, int width, int prefix_pos_offset, int chunk) {
    if (!h) { itts_set_error("gpt_set_code_prefix: null"); return ITTS_ERR_ARG; }
    if (!codes && !lens && n == 0) {                                 // uninstall
        h->prefix_codes = nullptr; h->prefix_lens.clear();
        h->prefix_n = h->prefix_width = h->prefix_pos_offset = h->prefix_chunk = 0;
        return ITTS_OK;
    }
    if (!codes || !lens || n < 1 || n > 65535 || width < 1 || width > (1 << 24) || prefix_pos_offset < 0 || chunk < 1 || chunk > 65535) {
        itts_set_error("gpt_set_code_prefix: codes, lens, 1 <= n <= 65535, width >= 1, prefix_pos_offset >= 0 and chunk in 1 .. 65535 -- or NULL, NULL, 0 to clear "
                       "(n=%d width=%d prefix_pos_offset=%d chunk=%d)", n, width, prefix_pos_offset, chunk);
        return ITTS_ERR_ARG;
    }
    for (int b = 0; b < n; ++b)
        if (lens[b] < 0 || lens[b] > width) { itts_set_error("gpt_set_code_prefix: lens[%d] = %d outside 0 .. width = %d", b, lens[b], width); return ITTS_ERR_ARG; }
    // the ids index the embedding table and the seen set: read them back and check them here, once (the table is small; the call synchronises)
    ItDevGuard dg(h->device);
    const int dc = itts_ptr_device(codes);
    if (dc >= 0 && dc != h->device) { itts_set_error("gpt_set_code_prefix: codes are on device %d but the engine was created on device %d", dc, h->device); return ITTS_ERR_ARG; }
    std::vector<int64_t> host((size_t)n * width);
    HIP_TRY(hipMemcpy(host.data(), codes, host.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < n; ++b)
        for (int j = 0; j < lens[b]; ++j) {
            const int64_t v = host[(size_t)b * width + j];
            if (v < 0 || v >= h->cfg.vocab) { itts_set_error("gpt_set_code_prefix: codes[%d][%d] = %lld outside the %d codes", b, j, (long long)v, h->cfg.vocab); return ITTS_ERR_ARG; }
        }
    h->prefix_codes = codes; h->prefix_lens.assign(lens, lens + n);
    h->prefix_n = n; h->prefix_width = width; h->prefix_pos_offset = prefix_pos_offset; h->prefix_chunk = chunk;
    return ITTS_OK;
}

extern "C" int itts_gpt_last_prefix(const itts_gpt* h, int32_t* max_len, int32_t* chunks) {
    if (!h || !max_len || !chunks) { itts_set_error("gpt_last_prefix: null"); return ITTS_ERR_ARG; }
    *max_len = h->last_prefix_max; *chunks = h->last_prefix_chunks;
    return ITTS_OK;
}

// What both per-request sampling tables (rows: itts_row_sampling, beam groups: itts_group_sampling) check and do: the DEVICE table is copied to
// the host ONCE, here, to reject what the scalar path rejects in launch_sample / launch_beam_step -- the kernels never check -- and installed.
// beam: a beam keeps 64 (BEAM_CAP) survivors, so max(top_k, min_tokens_to_keep) is what must fit.
template <class Entry>
static int set_sampling_table(itts_gpt* h, const Entry* table, int n, bool beam, const char* who, const Entry** installed, int* installed_n) {
    if (!h || (table && n <= 0)) { itts_set_error("%s: bad args", who); return ITTS_ERR_ARG; }
    if (!table) { *installed = nullptr; *installed_n = 0; return ITTS_OK; }
    ItDevGuard dg(h->device);
    std::vector<Entry> host((size_t)n);
    HIP_TRY(hipMemcpy(host.data(), table, (size_t)n * sizeof(Entry), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        const Entry& e = host[(size_t)i];
        const int k = beam && e.min_tokens_to_keep > e.top_k ? e.min_tokens_to_keep : e.top_k;
        if (e.do_sample && (e.top_k <= 0 || k > 64)) {
            itts_set_error("%s: entry %d: %stop_k must be in 1..64 on the device path (got %d)", who, i, beam ? "beam-sample: " : "", e.top_k);
            return ITTS_ERR_ARG;
        }
        if (e.typical_mass != 0.f && !(e.typical_mass > 0.f && e.typical_mass < 1.f)) {
            itts_set_error("%s: entry %d: `typical_mass` has to be a float > 0 and < 1, but is %g", who, i, (double)e.typical_mass);
            return ITTS_ERR_ARG;
        }
        if (!(e.repetition_penalty > 0.f) || !(e.temperature > 0.f)) {
            itts_set_error("%s: entry %d: repetition_penalty (%g) and temperature (%g) must be > 0", who, i, (double)e.repetition_penalty,
                           (double)e.temperature);
            return ITTS_ERR_ARG;
        }
        if (e.min_tokens_to_keep < 0 || e.min_tokens_to_keep > 2) {         // (the typical filter keeps 1 or 2)
            itts_set_error("%s: entry %d: min_tokens_to_keep (%d) must be in 0..2", who, i, e.min_tokens_to_keep);
            return ITTS_ERR_ARG;
        }
    }
    *installed = table;
    *installed_n = n;
    return ITTS_OK;
}

// Per-slot sampling settings (design reference: per-request settings in one batch, backends/trt/serving/triton_server.py:96-305).  table is a
// DEVICE array the caller keeps alive; it is copied to the host ONCE here to reject what the scalar path rejects in launch_sample / cannot do --
// the kernel itself never checks.  A host that rewrites a finished slot's entry later (before itts_gpt_admit_rows) keeps to the same domain.
static_assert(sizeof(itts_row_sampling) == sizeof(RowSampling) && sizeof(RowSampling) == 40, "itts_row_sampling layout");
static_assert(offsetof(itts_row_sampling, typical_mass) == offsetof(RowSampling, typical_mass) && offsetof(itts_row_sampling, stream) == offsetof(RowSampling, stream) &&
              offsetof(itts_row_sampling, seed) == offsetof(RowSampling, seed), "itts_row_sampling layout");
extern "C" int itts_gpt_set_row_sampling(itts_gpt* h, const itts_row_sampling* table, int n) {
    return set_sampling_table(h, table, n, false, "gpt_set_row_sampling", h ? &h->row_sampling : nullptr, h ? &h->row_sampling_n : nullptr);
}

// Per-group sampling settings of the beam kernels (design reference: per-request settings in one batch, backends/trt/serving/triton_server.py:96-305,
// in the reference's default 3-beam mode, indextts/infer_v2_5.py:732-740).  As itts_gpt_set_row_sampling: table is a DEVICE array the caller keeps
// alive, copied to the host ONCE here to reject what launch_beam_step rejects of the scalars -- the kernels never check.  A host that rewrites a
// finished group's entry later (before itts_gpt_admit_beam_groups) keeps to the same domain.
static_assert(sizeof(itts_group_sampling) == sizeof(GroupSampling) && sizeof(GroupSampling) == 48, "itts_group_sampling layout");
static_assert(offsetof(itts_group_sampling, typical_mass) == offsetof(GroupSampling, typical_mass) &&
              offsetof(itts_group_sampling, length_penalty) == offsetof(GroupSampling, length_penalty) &&
              offsetof(itts_group_sampling, stream) == offsetof(GroupSampling, stream) && offsetof(itts_group_sampling, seed) == offsetof(GroupSampling, seed),
              "itts_group_sampling layout");
extern "C" int itts_gpt_set_group_sampling(itts_gpt* h, const itts_group_sampling* table, int n_groups) {
    return set_sampling_table(h, table, n_groups, true, "gpt_set_group_sampling", h ? &h->group_sampling : nullptr, h ? &h->group_sampling_n : nullptr);
}

// Logits filters: what GenerationMixin._get_logits_processor (transformers_generation_utils.py:843-1070) builds from the generate() kwargs beyond
// the engine's defaults.  The arguments are checked here, as HF's processor constructors check them; the arrays are copied into handle-owned
// device buffers sized once (V ids, n_mel_pos + 1 steps) and the scalars into ONE device record, all at addresses that never change: the
// selection kernels read every setting from device memory, so a captured step graph serves any later installation.
// what both filter setters check of one record (who: the entry's name in the messages) and the [V] mask bytes it builds; *any: a bit is set
static int check_filter_record(const itts_gpt_config& c, const itts_logits_filters* f, const char* who, std::vector<unsigned char>& mask, bool* any_out) {
    const int V = c.vocab, cap = c.n_mel_pos + 1;
    if (f->min_new_tokens < 0 || f->min_length < 0) {
        itts_set_error("%s: `min_new_tokens` (%d) and `min_length` (%d) have to be non-negative integers", who, f->min_new_tokens, f->min_length);
        return ITTS_ERR_ARG;
    }
    if (f->no_repeat_ngram_size < 0) {
        itts_set_error("%s: `ngram_size` has to be a strictly positive integer (0 = off), but is %d", who, f->no_repeat_ngram_size);
        return ITTS_ERR_ARG;
    }
    if (!(f->min_p < 0.f) && !(f->min_p >= 0.f && f->min_p <= 1.f)) {
        itts_set_error("%s: `min_p` has to be a float in the [0, 1] interval (negative = off), but is %g", who, (double)f->min_p);
        return ITTS_ERR_ARG;
    }
    if ((f->epsilon_cutoff != 0.f && !(f->epsilon_cutoff > 0.f && f->epsilon_cutoff < 1.f)) || (f->eta_cutoff != 0.f && !(f->eta_cutoff > 0.f && f->eta_cutoff < 1.f))) {
        itts_set_error("%s: `epsilon_cutoff` (%g) and `eta_cutoff` (%g) have to be floats > 0 and < 1 (0 = off)", who, (double)f->epsilon_cutoff, (double)f->eta_cutoff);
        return ITTS_ERR_ARG;
    }
    if (f->n_suppress < 0 || f->n_begin_suppress < 0 || f->n_decay < 0 || (f->n_suppress > 0 && !f->suppress_ids) ||
        (f->n_begin_suppress > 0 && !f->begin_suppress_ids) || (f->n_decay > 0 && !f->decay_table)) {
        itts_set_error("%s: a count without its array", who);
        return ITTS_ERR_ARG;
    }
    if (f->n_decay > cap) { itts_set_error("%s: decay table of %d steps, the mel position table bounds a row at %d", who, f->n_decay, cap); return ITTS_ERR_ARG; }
    if (f->n_decay > 0 && f->decay_start < 0) { itts_set_error("%s: exponential_decay_length_penalty start index %d < 0", who, f->decay_start); return ITTS_ERR_ARG; }
    mask.assign((size_t)V, 0);
    bool any = false;
    for (int kind = 0; kind < 2; ++kind) {
        const int32_t* ids = kind ? f->begin_suppress_ids : f->suppress_ids;
        const int n = kind ? f->n_begin_suppress : f->n_suppress;
        for (int i = 0; i < n; ++i) {
            if (ids[i] < 0 || ids[i] >= V) {
                itts_set_error("%s: %s id %d (entry %d) outside 0 .. %d", who, kind ? "begin-suppress" : "suppress", ids[i], i, V - 1);
                return ITTS_ERR_ARG;
            }
            mask[(size_t)ids[i]] |= (unsigned char)(1 << kind);
            any = true;
        }
    }
    *any_out = any;
    return ITTS_OK;
}
// the device record of a checked host record; mask / decay: the device rows it reads; prompt_len: what the generate prologue will overwrite
static LogitsFilters filter_record(const itts_gpt_config& c, const itts_logits_filters* f, bool any, int prompt_len, const unsigned char* mask, const float* decay) {
    LogitsFilters r{};
    r.min_new_tokens = f->min_new_tokens; r.min_length = f->min_length; r.ngram = f->no_repeat_ngram_size;
    r.decay_start = f->n_decay > 0 ? f->decay_start : -1; r.n_decay = f->n_decay; r.has_mask = any ? 1 : 0;
    r.prompt_len = prompt_len; r.start_mel = c.start_mel_token;
    r.min_p = f->min_p < 0.f ? -1.f : f->min_p; r.epsilon = f->epsilon_cutoff; r.eta = f->eta_cutoff;
    r.mask = mask; r.decay = decay;
    return r;
}

extern "C" int itts_gpt_set_logits_filters(itts_gpt* h, const itts_logits_filters* f) {
    const char* who = "gpt_set_logits_filters";
    if (!h) { itts_set_error("%s: null handle", who); return ITTS_ERR_ARG; }
    if (!f) { h->filt_on = false; h->filt_ngram = 0; return ITTS_OK; }
    const itts_gpt_config& c = h->cfg;
    const int V = c.vocab, cap = c.n_mel_pos + 1;
    std::vector<unsigned char> mask;
    bool any = false;
    if (int rc = check_filter_record(c, f, who, mask, &any)) return rc;
    ItDevGuard dg(h->device);
    if (!h->filt_dev) {
        void *d = nullptr, *m = nullptr, *t = nullptr;
        HIP_TRY(hipMalloc(&d, sizeof(LogitsFilters))); h->owned.push_back(d);
        HIP_TRY(hipMalloc(&m, (size_t)V)); h->owned.push_back(m);
        HIP_TRY(hipMalloc(&t, (size_t)cap * sizeof(float))); h->owned.push_back(t);
        h->filt_dev = (LogitsFilters*)d; h->filt_mask = (unsigned char*)m; h->filt_decay = (float*)t; h->filt_decay_cap = cap;
    }
    if (h->stream) HIP_TRY(hipStreamSynchronize(h->stream));          // (no step of an earlier call is still reading the record)
    const LogitsFilters r = filter_record(c, f, any, 1, h->filt_mask, h->filt_decay);
    HIP_TRY(hipMemcpy(h->filt_mask, mask.data(), (size_t)V, hipMemcpyHostToDevice));
    if (f->n_decay > 0) HIP_TRY(hipMemcpy(h->filt_decay, f->decay_table, (size_t)f->n_decay * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->filt_dev, &r, sizeof(r), hipMemcpyHostToDevice));
    h->filt_on = true;
    h->filt_ngram = r.ngram;
    return ITTS_OK;
}

// Per-slot logits filters: a table of the records above, one per utterance slot (rows) or beam group, each with its own row of a [slots][V]
// mask array and a [slots][n_mel_pos + 1] decay array.  The three arrays are allocated at the first installation (kept and reused while they are
// large enough; a larger table gets new ones and the old stay allocated until itts_gpt_destroy) and do not move while the table is installed: a
// captured step bakes the table's address in.
extern "C" int itts_gpt_set_row_filters(itts_gpt* h, const itts_logits_filters* entries, const int32_t* slots, int n, int n_slots) {
    const char* who = "gpt_set_row_filters";
    if (!h) { itts_set_error("%s: null handle", who); return ITTS_ERR_ARG; }
    const bool suspended = h->susp.kind != itts_gpt::Suspended::NONE;
    if (!entries) {                                                   // uninstall: the call-wide record, if any, rules again
        h->ftab_n = 0; h->ftab_ngram.clear();
        return ITTS_OK;
    }
    if (n < 1 || n_slots < 1 || n > n_slots || n_slots > 65535) {
        itts_set_error("%s: 1 <= n <= n_slots <= 65535 -- or entries == NULL to uninstall (n=%d n_slots=%d)", who, n, n_slots);
        return ITTS_ERR_ARG;
    }
    // (every generate entry leaves its loop resumable, so a handle without a table can always take one: a resume is then held to the table's
    // size by the entry's own check.  What a suspended loop cannot have is the table it runs under resized beneath it.)
    if (h->ftab_n && h->ftab_n != n_slots && suspended) {
        itts_set_error("%s: a decode loop is suspended on the handle under a table of %d slots: its size cannot change to %d (uninstall first: entries == NULL)",
                       who, h->ftab_n, n_slots);
        return ITTS_ERR_STATE;
    }
    const itts_gpt_config& c = h->cfg;
    const int V = c.vocab, cap = c.n_mel_pos + 1;
    std::vector<std::vector<unsigned char>> masks((size_t)n);
    std::vector<char> any((size_t)n, 0);
    std::vector<char> named((size_t)n_slots, 0);
    for (int i = 0; i < n; ++i) {
        const int u = slots ? slots[i] : i;
        if (u < 0 || u >= n_slots || named[(size_t)u]) {
            itts_set_error("%s: slots[%d] = %d is outside 0 .. %d or named twice", who, i, u, n_slots - 1);
            return ITTS_ERR_ARG;
        }
        named[(size_t)u] = 1;
        char name[64];
        snprintf(name, sizeof name, "%s: entry %d", who, i);
        bool a = false;
        if (int rc = check_filter_record(c, &entries[i], name, masks[(size_t)i], &a)) return rc;
        any[(size_t)i] = a ? 1 : 0;
    }
    ItDevGuard dg(h->device);
    if (h->stream) HIP_TRY(hipStreamSynchronize(h->stream));          // (no step of an earlier call is still reading the table)
    const bool fresh = h->ftab_n != n_slots;                          // first installation after an uninstall (or another size): every slot is written
    if (fresh && n_slots > h->ftab_cap) {
        // Grow by NEW arrays; the old ones stay allocated until the handle is destroyed (`owned`).  Cached step graphs have the old table's
        // address baked in and keyed: while that address stays allocated no later allocation -- the call-wide record's among them -- can be
        // handed it, so such a graph is never matched again.  The capacity at least doubles, which bounds what is kept at the final size.
        const int want = n_slots > 2 * h->ftab_cap ? n_slots : (2 * h->ftab_cap > 65535 ? 65535 : 2 * h->ftab_cap);
        void *d = nullptr, *m = nullptr, *t = nullptr;
        if (hipMalloc(&d, (size_t)want * sizeof(LogitsFilters)) != hipSuccess || hipMalloc(&m, (size_t)want * V) != hipSuccess ||
            hipMalloc(&t, (size_t)want * cap * sizeof(float)) != hipSuccess) {
            (void)hipGetLastError();
            if (d) (void)hipFree(d);
            if (m) (void)hipFree(m);
            if (t) (void)hipFree(t);
            itts_set_error("%s: out of device memory for a table of %d slots", who, want);
            return ITTS_ERR_HIP;
        }
        h->owned.push_back(d); h->owned.push_back(m); h->owned.push_back(t);      // freed by itts_gpt_destroy, like the call-wide record's buffers
        h->ftab_dev = (LogitsFilters*)d; h->ftab_mask = (unsigned char*)m; h->ftab_decay = (float*)t; h->ftab_cap = want;
    }
    // a rewrite while a row loop is suspended keeps the prompt length its prologue wrote; a first call's prologue writes its own
    const int S = h->susp.kind == itts_gpt::Suspended::ROWS ? h->susp.S : 1;
    if (fresh) {
        itts_logits_filters off{};
        off.min_p = -1.f;
        std::vector<LogitsFilters> tab((size_t)n_slots);
        for (int u = 0; u < n_slots; ++u)
            tab[(size_t)u] = filter_record(c, &off, false, S, h->ftab_mask + (size_t)u * V, h->ftab_decay + (size_t)u * cap);
        HIP_TRY(hipMemcpy(h->ftab_dev, tab.data(), tab.size() * sizeof(LogitsFilters), hipMemcpyHostToDevice));
        h->ftab_ngram.assign((size_t)n_slots, 0);
    }
    for (int i = 0; i < n; ++i) {
        const int u = slots ? slots[i] : i;
        const itts_logits_filters* f = &entries[i];
        unsigned char* m = h->ftab_mask + (size_t)u * V;
        float* t = h->ftab_decay + (size_t)u * cap;
        const LogitsFilters r = filter_record(c, f, any[(size_t)i] != 0, S, m, t);
        if (r.has_mask) HIP_TRY(hipMemcpy(m, masks[(size_t)i].data(), (size_t)V, hipMemcpyHostToDevice));
        if (f->n_decay > 0) HIP_TRY(hipMemcpy(t, f->decay_table, (size_t)f->n_decay * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->ftab_dev + u, &r, sizeof(r), hipMemcpyHostToDevice));
        h->ftab_ngram[(size_t)u] = r.ngram;
    }
    h->ftab_n = n_slots;
    return ITTS_OK;
}

// Of the last generate call: sum over its decode steps of the rows each step ran, and the number of compactions.
extern "C" int itts_gpt_compaction_stats(const itts_gpt* h, int64_t* row_steps, int32_t* compactions) {
    if (!h) return ITTS_ERR_ARG;
    if (row_steps) *row_steps = h->last_row_steps;
    if (compactions) *compactions = h->last_compactions;
    return ITTS_OK;
}

extern "C" int itts_gpt_graph_stats(const itts_gpt* h, int32_t* captures, int32_t* hits) {
    if (!h) return ITTS_ERR_ARG;
    if (captures) *captures = h->graph_captures;
    if (hits) *hits = h->graph_hits;
    return ITTS_OK;
}

extern "C" int itts_gpt_last_timing(const itts_gpt* h, float* prefill_ms, float* decode_ms, int32_t* steps) {
    if (!h) return ITTS_ERR_ARG;
    if (prefill_ms) *prefill_ms = h->last_prefill_ms;
    if (decode_ms) *decode_ms = h->last_decode_ms;
    if (steps) *steps = h->last_steps;
    return ITTS_OK;
}

// Teacher-forced pass over full sequences: out = final_norm(ln_f(stack(x)))  (UnifiedVoice.forward / get_logits,
// indextts/gpt/model_v2.py:528-554,596-646).  x [nseq][S][D] f32 device, out [nseq][S][D] f32 device.
extern "C" int itts_gpt_forward_latent(itts_gpt* h, const float* x, int nseq, int S, float* out, void* workspace,
                                       size_t workspace_bytes, void* caller_stream) {
    if (!h || !x || !out || !workspace) { itts_set_error("gpt_forward_latent: null pointer"); return ITTS_ERR_ARG; }
    if (!h->finalized) { itts_set_error("gpt_forward_latent: call itts_gpt_finalize first"); return ITTS_ERR_STATE; }
    ItDevGuard dg(h->device);
    if (int rcd = check_same_device(h, x, workspace, "gpt_forward_latent")) return rcd;
    const itts_gpt_config& c = h->cfg;
    if (nseq <= 0 || S <= 0 || S > 65535) { itts_set_error("gpt_forward_latent: bad shape"); return ITTS_ERR_ARG; }
    WsCarve wc;
    if (int rcw = carve_ws(h, workspace, workspace_bytes, nseq, S, S, 1, "gpt_forward_latent", &wc)) return rcw;
    const GptWs& w = wc.w;
    hipStream_t st = h->stream, cs = (hipStream_t)caller_stream;
    if (int rcs = stream_enter(h, cs)) return rcs;
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 0, 0);
    HIP_TRY(hipMemcpyAsync(w.x, x, (size_t)nseq * S * c.model_dim * 4, hipMemcpyDeviceToDevice, st));
    bool pending = false;
    int rc = run_layers(h, w, nseq, S, S, true, w.state + 1, nullptr, &pending, st);
    if (rc) return rc;
    LnArgs ln{};
    ln.x = w.x; ln.g1 = h->lnf_g; ln.b1 = h->lnf_b; ln.g2 = h->fn_g; ln.b2 = h->fn_b; ln.out = out; ln.out_f32 = 1;
    ln.rows = nseq * S; ln.D = c.model_dim; ln.in_row_mul = 1; ln.in_row_add = 0; ln.eps = c.ln_eps; ln.nsplit = 1;
    if ((rc = launch_ln(ln, c.precision, st))) return rc;
    if ((rc = stream_leave(h, cs))) return rc;
    return ITTS_OK;
}

// ---- teacher-forced latent session ------------------------------------------------------------------------------------------------
// The pass of itts_gpt_forward_latent with its KV cache KEPT: the prefix (conds | [start_text, ids, stop_text]) is prefilled once, then every
// append runs only the new mel positions against the cache -- O(chunk) per chunk of a streamed utterance instead of the whole sequence again
// (replaces, per chunk: UnifiedVoice.forward(..., return_latent=True), model_v2.py:528-554,596-646; the reference's streaming pipeline gets its
// per-chunk latent from the TRT-LLM session instead, backends/trt/runtime/gpt_trtllm_runtime.py:381-519).  The pass is causal and has no mask, so
// the latents of a code prefix are the latents the finished utterance has at those positions.
// Everything the session owns lives in ITS workspace (cache, activations, position counter, per-row shifts, last codes): it shares the handle's
// weights, stream and ev_in / ev_out only, and touches none of the handle's suspended-loop record / cur_* / host_* fields -- a decode loop suspended between two
// itts_gpt_generate_chunk calls on the same handle resumes with the bits it would have produced without the session (tests/test_gpu_latent_session.py).
// Rows may have different prefix lengths: row b's mel position j sits at cache index prefix_lens[b] + j.  The launches run under ONE position
// counter (max_prefix + appended) with pos_shift[b] = max_prefix - prefix_lens[b], the convention of itts_gpt_admit_rows.
struct itts_gpt_latent {
    itts_gpt* h = nullptr;
    int nseq = 0, max_prefix = 0, max_codes = 0, max_append = 0, Smax = 0, Tmax = 0;
    int appended = 0;                    // mel positions in the cache, the same for every row
    char* base = nullptr;                // 256-byte aligned start of the session's workspace
    int* shift = nullptr;                // device [nseq]: max_prefix - prefix_lens[b]
    long long* last = nullptr;           // device [2][nseq]: every row's last appended code, double-buffered by append parity
    int parity = 0;
};
static std::mutex g_latent_mu;
static std::set<itts_gpt_latent*> g_latent_live;      // open sessions: a closed (freed) one is recognised without being dereferenced

void itts_gpt_latent_drop_handle(itts_gpt* h) {       // itts_gpt_destroy: sessions of a dying handle are closed with it
    std::lock_guard<std::mutex> lk(g_latent_mu);
    for (auto it = g_latent_live.begin(); it != g_latent_live.end();) {
        if ((*it)->h == h) { delete *it; it = g_latent_live.erase(it); }
        else ++it;
    }
}

struct LatentCarve { GptWs w; size_t shift_off, last_off, total; };
static LatentCarve latent_carve(const itts_gpt_config& c, char* base, int nseq, int Smax, int Tmax) {
    LatentCarve lc;
    lc.w = carve(c, base, nseq, Smax, Tmax);
    lc.shift_off = lc.w.total;
    lc.last_off = lc.shift_off + a256((size_t)nseq * 4);
    lc.total = lc.last_off + a256((size_t)2 * nseq * 8);
    return lc;
}

static bool latent_shape_ok(const itts_gpt* h, int nseq, int max_prefix, int max_codes, int max_append) {
    return h && nseq > 0 && max_prefix > 0 && max_codes > 0 && max_append > 0 && max_prefix <= 65535 && max_append <= 65535 &&
           (long long)max_prefix + max_codes <= (1 << 24) && (size_t)nseq * h->cfg.heads <= 2147483647u / 4;
}

extern "C" size_t itts_gpt_latent_workspace_bytes(const itts_gpt* h, int nseq, int max_prefix, int max_codes, int max_append) {
    if (!latent_shape_ok(h, nseq, max_prefix, max_codes, max_append)) return 0;
    return latent_carve(h->cfg, nullptr, nseq, max_prefix > max_append ? max_prefix : max_append, max_prefix + max_codes).total + 512;
}

// x[b][i] = mel_emb[code before mel position j0 + i] + mel_pos[j0 + i]: start_mel before position 0, the row's last appended code before the first
// position of a later append, codes[b][i - 1] inside the call (what forward_latent's host code builds for the whole utterance at once).  Ids outside
// the table are clamped (the codes live on the device: nothing to validate on the host).  The block of the last position keeps the row's last code.
__global__ __launch_bounds__(256) void latent_embed_kernel(const long long* __restrict__ codes, int n, const long long* __restrict__ last_in,
                                                           long long* __restrict__ last_out, int j0, int start_tok, int V, const float* __restrict__ mel_emb,
                                                           const float* __restrict__ mel_pos, float* __restrict__ x, int D) {
    const int i = blockIdx.x, b = blockIdx.y, j = j0 + i;
    long long tok = j == 0 ? (long long)start_tok : i == 0 ? last_in[b] : codes[(size_t)b * n + i - 1];
    tok = tok < 0 ? 0 : tok >= V ? V - 1 : tok;
    const float* e = mel_emb + (size_t)tok * D;
    const float* p = mel_pos + (size_t)j * D;
    float* o = x + ((size_t)b * n + i) * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) o[c] = e[c] + p[c];
    if (i == n - 1 && threadIdx.x == 0) last_out[b] = codes[(size_t)b * n + n - 1];
}

extern "C" int itts_gpt_latent_open(itts_gpt* h, const float* prefix_x, const int32_t* prefix_lens, int nseq, int max_prefix, int max_codes,
                                    int max_append, void* workspace, size_t workspace_bytes, void* caller_stream, itts_gpt_latent** out) {
    if (out) *out = nullptr;
    if (!h || !prefix_x || !prefix_lens || !workspace || !out) { itts_set_error("gpt_latent_open: null pointer"); return ITTS_ERR_ARG; }
    if (!h->finalized) { itts_set_error("gpt_latent_open: call itts_gpt_finalize first"); return ITTS_ERR_STATE; }
    if (!latent_shape_ok(h, nseq, max_prefix, max_codes, max_append)) {
        itts_set_error("gpt_latent_open: bad shape (nseq=%d max_prefix=%d max_codes=%d max_append=%d)", nseq, max_prefix, max_codes, max_append);
        return ITTS_ERR_ARG;
    }
    ItDevGuard dg(h->device);
    if (int rcd = check_same_device(h, prefix_x, workspace, "gpt_latent_open")) return rcd;
    const itts_gpt_config& c = h->cfg;
    if (max_codes > c.n_mel_pos) {
        itts_set_error("gpt_latent_open: max_codes=%d exceeds the mel position table (%d rows)", max_codes, c.n_mel_pos);
        return ITTS_ERR_ARG;
    }
    std::vector<int> shift(nseq);
    for (int b = 0; b < nseq; ++b) {
        if (prefix_lens[b] < 1 || prefix_lens[b] > max_prefix) {
            itts_set_error("gpt_latent_open: prefix_lens[%d] = %d outside 1 .. max_prefix = %d", b, prefix_lens[b], max_prefix);
            return ITTS_ERR_ARG;
        }
        shift[b] = max_prefix - prefix_lens[b];
    }
    const int Smax = max_prefix > max_append ? max_prefix : max_append, Tmax = max_prefix + max_codes;
    char* base = align256(workspace);
    const LatentCarve lc0 = latent_carve(c, nullptr, nseq, Smax, Tmax);
    if (workspace_bytes < lc0.total + (size_t)(base - (char*)workspace)) {
        itts_set_error("gpt_latent_open: workspace too small (%zu < %zu)", workspace_bytes, lc0.total + 256);
        return ITTS_ERR_ARG;
    }
    const LatentCarve lc = latent_carve(c, base, nseq, Smax, Tmax);
    const GptWs& w = lc.w;
    int* shift_dev = (int*)(base + lc.shift_off);
    long long* last_dev = (long long*)(base + lc.last_off);
    hipStream_t st = h->stream, cs = (hipStream_t)caller_stream;
    if (int rcs = stream_enter(h, cs)) return rcs;
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 0, 0);
    HIP_TRY(hipMemcpyAsync(shift_dev, shift.data(), (size_t)nseq * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(last_dev, 0, (size_t)2 * nseq * 8, st));
    HIP_TRY(hipMemcpyAsync(w.x, prefix_x, (size_t)nseq * max_prefix * c.model_dim * 4, hipMemcpyDeviceToDevice, st));
    // The prefix is right-padded to max_prefix and prefilled at every row's own positions 0 .. max_prefix - 1 (no shift): row b's pad positions
    // land in the cache at prefix_lens[b] .. max_prefix - 1.  They are never seen: a causal query reads no key past its own position, and the
    // row's mel positions, appended from prefix_lens[b] on, overwrite each of them before any query reaches that far.
    bool pending = false;
    int rc = run_layers(h, w, nseq, max_prefix, Tmax, true, w.state + 1, nullptr, &pending, st);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    if ((rc = stream_leave(h, cs))) return rc;                          // (synchronises: `shift` is pageable host memory)
    itts_gpt_latent* s = new itts_gpt_latent();
    s->h = h; s->nseq = nseq; s->max_prefix = max_prefix; s->max_codes = max_codes; s->max_append = max_append; s->Smax = Smax; s->Tmax = Tmax;
    s->base = base; s->shift = shift_dev; s->last = last_dev;
    { std::lock_guard<std::mutex> lk(g_latent_mu); g_latent_live.insert(s); }
    *out = s;
    return ITTS_OK;
}

extern "C" int itts_gpt_latent_append(itts_gpt_latent* s, const int64_t* codes, int n, float* out, void* caller_stream) {
    if (!s || !codes || !out) { itts_set_error("gpt_latent_append: null pointer"); return ITTS_ERR_ARG; }
    {
        std::lock_guard<std::mutex> lk(g_latent_mu);
        if (!g_latent_live.count(s)) { itts_set_error("gpt_latent_append: the session is closed"); return ITTS_ERR_STATE; }
    }
    itts_gpt* h = s->h;
    const itts_gpt_config& c = h->cfg;
    if (n < 1 || n > s->max_append) { itts_set_error("gpt_latent_append: n = %d outside 1 .. max_append = %d", n, s->max_append); return ITTS_ERR_ARG; }
    if (s->appended + n > s->max_codes) {
        itts_set_error("gpt_latent_append: %d + %d codes exceed the session's max_codes = %d", s->appended, n, s->max_codes);
        return ITTS_ERR_ARG;
    }
    if (s->appended + n > c.n_mel_pos) {
        itts_set_error("gpt_latent_append: mel position %d is past the mel position table (%d rows)", s->appended + n - 1, c.n_mel_pos);
        return ITTS_ERR_ARG;
    }
    ItDevGuard dg(h->device);
    if (int rcd = check_same_device(h, codes, out, "gpt_latent_append")) return rcd;
    const GptWs w = carve(c, s->base, s->nseq, s->Smax, s->Tmax);
    hipStream_t st = h->stream, cs = (hipStream_t)caller_stream;
    if (int rcs = stream_enter(h, cs)) return rcs;
    // one shared counter for every row; row b's own position of query i is max_prefix + appended + i - shift[b] = prefix_lens[b] + appended + i
    hipLaunchKernelGGL(set_state_kernel, dim3(1), dim3(1), 0, st, w.state, 0, s->max_prefix + s->appended);
    hipLaunchKernelGGL(latent_embed_kernel, dim3(n, s->nseq), dim3(256), 0, st, (const long long*)codes, n, s->last + (size_t)s->parity * s->nseq,
                       s->last + (size_t)(s->parity ^ 1) * s->nseq, s->appended, c.start_mel_token, c.vocab, h->mel_emb, h->mel_pos, w.x, c.model_dim);
    HIP_TRY(hipGetLastError());
    bool pending = false;
    int rc = run_layers(h, w, s->nseq, n, s->Tmax, true, w.state + 1, nullptr, &pending, st, false, 1, nullptr, nullptr, s->shift);
    if (rc) return rc;
    LnArgs ln{};
    ln.x = w.x; ln.g1 = h->lnf_g; ln.b1 = h->lnf_b; ln.g2 = h->fn_g; ln.b2 = h->fn_b; ln.out = out; ln.out_f32 = 1;
    ln.rows = s->nseq * n; ln.D = c.model_dim; ln.in_row_mul = 1; ln.in_row_add = 0; ln.eps = c.ln_eps; ln.nsplit = 1;
    if ((rc = launch_ln(ln, c.precision, st))) return rc;
    if ((rc = stream_leave(h, cs))) return rc;
    s->appended += n;
    s->parity ^= 1;
    return ITTS_OK;
}

extern "C" int itts_gpt_latent_appended(const itts_gpt_latent* s) {
    std::lock_guard<std::mutex> lk(g_latent_mu);
    return (s && g_latent_live.count(const_cast<itts_gpt_latent*>(s))) ? s->appended : -1;
}

extern "C" int itts_gpt_latent_close(itts_gpt_latent* s) {
    if (!s) { itts_set_error("gpt_latent_close: null"); return ITTS_ERR_ARG; }
    std::lock_guard<std::mutex> lk(g_latent_mu);
    if (!g_latent_live.erase(s)) { itts_set_error("gpt_latent_close: the session is already closed"); return ITTS_ERR_STATE; }
    delete s;
    return ITTS_OK;
}

// ---- teacher-forced rescoring pass ---------------------------------------------------------------------------------------------------
// Per-token log-probabilities and text attention of GIVEN codes: the prompt is prefilled as itts_gpt_generate prefills it, then the codes run
// through the stack `chunk` positions at a time with the decode step's inputs (mel_emb[code i - 1] + mel_pos[i - 1 + pos_offset] at cache
// position S - 1 + i), each chunk through run_layers(prefill = true), ln_f -> final_norm, the head GEMM on the chunk's rows and logp_gather;
// attn_align_mq after each listed layer's QKV GEMM (replaces UnifiedVoice.forward / get_logits teacher forcing, model_v2.py:528-554,596-646,
// with compute_transition_scores, transformers_generation_utils.py:1132, and output_attentions=True, transformers_gpt2.py:189, over them).
// Everything the pass owns lives in ITS workspace (cache, activations, position counters, chunk logits): like the latent session it shares the
// handle's weights, stream and ev_in / ev_out only and touches none of the suspended-loop record / cur_* / host_* fields or the installed
// score / alignment arrays -- a decode or beam loop suspended on the handle resumes with the bits it would have produced without the call.
struct RescoreCarve { GptWs w; size_t hl_off, logits_off, tgt_off, lp_off, qlen_off, clen_off, total; };
static RescoreCarve rescore_carve(const itts_gpt_config& c, char* base, int nseq, int S, int max_codes, int chunk) {
    RescoreCarve rc;
    const size_t esz = c.precision == PREC_BF16 ? 2 : 4, rows = (size_t)nseq * chunk;
    rc.w = carve(c, base, nseq, S > chunk ? S : chunk, S + max_codes);
    rc.hl_off = rc.w.total;
    rc.logits_off = rc.hl_off + a256(rows * c.model_dim * esz);
    rc.tgt_off = rc.logits_off + a256(rows * c.vocab * 4);
    rc.lp_off = rc.tgt_off + a256(rows * 8);
    rc.qlen_off = rc.lp_off + a256(rows * 4);
    rc.clen_off = rc.qlen_off + a256((size_t)nseq * 4);
    rc.total = rc.clen_off + a256((size_t)nseq * 4);
    return rc;
}
static int rescore_chunk(int chunk, int max_codes) { return chunk < max_codes ? chunk : max_codes; }      // no chunk is longer than the codes
static bool rescore_shape_ok(const itts_gpt* h, int nseq, int S, int max_codes, int chunk) {
    // nseq is grid.y of rescore_embed_kernel; the rows of a pass (nseq * S, nseq * chunk) are ints inside run_layers and the launchers
    return h && nseq > 0 && nseq <= 65535 && S > 0 && S <= 65535 && max_codes > 0 && chunk >= 1 && chunk <= 65535 &&
           (long long)S + max_codes <= (1 << 24) && (size_t)nseq * h->cfg.heads <= 2147483647u / 4 &&
           (long long)nseq * S <= (1 << 24) && (long long)nseq * rescore_chunk(chunk, max_codes) <= (1 << 24) &&
           (long long)nseq * rescore_chunk(chunk, max_codes) * h->cfg.vocab <= 0x7fffffffLL;      // (the chunk's logits are indexed row * V)
}

extern "C" size_t itts_gpt_rescore_workspace_bytes(const itts_gpt* h, int nseq, int S, int max_codes, int chunk) {
    if (!rescore_shape_ok(h, nseq, S, max_codes, chunk)) return 0;
    return rescore_carve(h->cfg, nullptr, nseq, S, max_codes, rescore_chunk(chunk, max_codes)).total + 512;
}

__global__ void rescore_state_kernel(int* state, int pos, int qpos) { state[0] = 0; state[1] = pos; state[2] = 0; state[6] = qpos; }
// code 0 is predicted by the prompt's last position: its target and whether the row has it at all
__global__ void rescore_first_kernel(const long long* __restrict__ codes, int max_codes, const int* __restrict__ code_lens, long long* __restrict__ targets,
                                     int* __restrict__ q_len, int nseq) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nseq) return;
    const bool on = code_lens[b] > 0;
    q_len[b] = on ? 1 : 0;
    targets[b] = on ? codes[(size_t)b * max_codes] : -1;
}
// chunk rows i0 .. i0 + n - 1: x[b][qi] = mel_emb[codes[b][i - 1]] + mel_pos[i - 1 + pos_offset], i = i0 + qi (the decode step's next-step
// embedding, sample_kernel's x_next; ids outside the table clamped), the row's target codes[b][i] (-1 from code_lens[b] on: scored 0.0)
// and the sequence's valid queries in this chunk
__global__ __launch_bounds__(256) void rescore_embed_kernel(const long long* __restrict__ codes, int max_codes, const int* __restrict__ code_lens, int i0,
                                                            int n, int pos_offset, int V, const float* __restrict__ mel_emb,
                                                            const float* __restrict__ mel_pos, float* __restrict__ x, int D,
                                                            long long* __restrict__ targets, int* __restrict__ q_len) {
    const int qi = blockIdx.x, b = blockIdx.y, i = i0 + qi;
    long long tok = codes[(size_t)b * max_codes + i - 1];
    tok = tok < 0 ? 0 : tok >= V ? V - 1 : tok;
    const float* e = mel_emb + (size_t)tok * D;
    const float* p = mel_pos + (size_t)(i - 1 + pos_offset) * D;
    float* o = x + ((size_t)b * n + qi) * D;
    for (int c = threadIdx.x; c < D; c += blockDim.x) o[c] = e[c] + p[c];
    if (threadIdx.x == 0) {
        const int len = code_lens[b];
        targets[(size_t)b * n + qi] = i < len ? codes[(size_t)b * max_codes + i] : -1;
        if (qi == 0) { const int v = len - i0; q_len[b] = v < 0 ? 0 : v > n ? n : v; }
    }
}
__global__ void rescore_scatter_kernel(const float* __restrict__ lp, int n, float* __restrict__ out, int max_codes, int i0) {
    const int b = blockIdx.x;
    for (int qi = threadIdx.x; qi < n; qi += blockDim.x) out[(size_t)b * max_codes + i0 + qi] = lp[(size_t)b * n + qi];
}

extern "C" int itts_gpt_rescore(itts_gpt* h, const float* prefix_embeds, const int32_t* pad_lens, int nseq, int S, const int64_t* codes,
                                const int32_t* code_lens, int max_codes, int pos_offset, float* logp_out, const int32_t* pairs, int n_pairs,
                                const int32_t* span, float* align_out, int text_cap, int chunk, void* workspace, size_t workspace_bytes,
                                void* caller_stream) {
    const char* who = "gpt_rescore";
    if (!h || !prefix_embeds || !codes || !code_lens || !logp_out || !workspace) { itts_set_error("gpt_rescore: null pointer"); return ITTS_ERR_ARG; }
    if (!h->finalized) { itts_set_error("gpt_rescore: call itts_gpt_finalize first"); return ITTS_ERR_STATE; }
    if (!rescore_shape_ok(h, nseq, S, max_codes, chunk)) {
        itts_set_error("gpt_rescore: bad shape (nseq=%d S=%d max_codes=%d chunk=%d; chunk in 1 .. 65535)", nseq, S, max_codes, chunk);
        return ITTS_ERR_ARG;
    }
    const itts_gpt_config& c = h->cfg;
    if (pos_offset < 0 || max_codes + pos_offset > c.n_mel_pos + 1) {
        itts_set_error("gpt_rescore: max_codes=%d with pos_offset=%d exceeds the mel position table (%d rows)", max_codes, pos_offset, c.n_mel_pos);
        return ITTS_ERR_ARG;
    }
    const bool align = pairs || n_pairs || span || align_out || text_cap;
    int pr[ALIGN_MAX_PAIRS][2] = {};
    const int Tmax = S + max_codes;
    if (align) {                                                   // the rules of itts_gpt_set_alignment
        if (!pairs || !span || !align_out) { itts_set_error("gpt_rescore: pairs, span and align_out are given together, or all NULL / 0"); return ITTS_ERR_ARG; }
        if (n_pairs < 1 || n_pairs > ALIGN_MAX_PAIRS) { itts_set_error("gpt_rescore: n_pairs = %d outside 1 .. %d", n_pairs, ALIGN_MAX_PAIRS); return ITTS_ERR_ARG; }
        if (text_cap < 4 || text_cap > ALIGN_MAX_TEXT || (text_cap & 3)) {
            itts_set_error("gpt_rescore: text_cap = %d must be a multiple of 4 in 4 .. %d", text_cap, ALIGN_MAX_TEXT);
            return ITTS_ERR_ARG;
        }
        if (Tmax > ALIGN_MAX_KEYS) { itts_set_error("gpt_rescore: S + max_codes = %d cache positions, the alignment export takes %d", Tmax, ALIGN_MAX_KEYS); return ITTS_ERR_ARG; }
        for (int k = 0; k < n_pairs; ++k) {
            const int l = pairs[2 * k], hd = pairs[2 * k + 1];
            if (l < 0 || l >= c.layers || hd < 0 || hd >= c.heads) {
                itts_set_error("gpt_rescore: pair %d = (layer %d, head %d) outside %d layers x %d heads", k, l, hd, c.layers, c.heads);
                return ITTS_ERR_ARG;
            }
            for (int j = 0; j < k; ++j)
                if (pairs[2 * j] == l && pairs[2 * j + 1] == hd) { itts_set_error("gpt_rescore: pair (layer %d, head %d) is listed twice", l, hd); return ITTS_ERR_ARG; }
            pr[k][0] = l; pr[k][1] = hd;
        }
    }
    int Lmax = 0;
    for (int b = 0; b < nseq; ++b) {
        if (code_lens[b] < 0 || code_lens[b] > max_codes) {
            itts_set_error("gpt_rescore: code_lens[%d] = %d outside 0 .. max_codes = %d", b, code_lens[b], max_codes);
            return ITTS_ERR_ARG;
        }
        Lmax = code_lens[b] > Lmax ? code_lens[b] : Lmax;
    }
    ItDevGuard dg(h->device);
    if (int rcd = check_same_device(h, prefix_embeds, workspace, who)) return rcd;
    if (int rcd = check_same_device(h, codes, logp_out, who)) return rcd;
    chunk = rescore_chunk(chunk, max_codes);
    char* base = align256(workspace);
    const size_t need = rescore_carve(c, nullptr, nseq, S, max_codes, chunk).total + (size_t)(base - (char*)workspace);
    if (workspace_bytes < need) { itts_set_error("gpt_rescore: workspace too small (%zu < %zu)", workspace_bytes, need); return ITTS_ERR_ARG; }
    const RescoreCarve rcv = rescore_carve(c, base, nseq, S, max_codes, chunk);
    const GptWs& w = rcv.w;
    char* hl = base + rcv.hl_off;
    float* logits = (float*)(base + rcv.logits_off);
    long long* tgt = (long long*)(base + rcv.tgt_off);
    float* lp = (float*)(base + rcv.lp_off);
    int* qlen = (int*)(base + rcv.qlen_off);
    int* clen = (int*)(base + rcv.clen_off);
    const int D = c.model_dim, V = c.vocab, prec = c.precision;
    hipStream_t st = h->stream, cs = (hipStream_t)caller_stream;
    int rc;
    if ((rc = stream_enter(h, cs))) return rc;
    HIP_TRY(hipMemsetAsync(logp_out, 0, (size_t)nseq * max_codes * sizeof(float), st));
    if (align) HIP_TRY(hipMemsetAsync(align_out, 0, (size_t)nseq * max_codes * n_pairs * text_cap * sizeof(float), st));
    HIP_TRY(hipMemcpyAsync(clen, code_lens, (size_t)nseq * 4, hipMemcpyHostToDevice, st));
    if (pad_lens) HIP_TRY(hipMemcpyAsync(w.pad, pad_lens, (size_t)nseq * 4, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(hipMemsetAsync(w.pad, 0, (size_t)nseq * 4, st));
    if (Lmax > 0) {
        // ---- the prompt: its last position is the query that predicts code 0 ----
        HIP_TRY(hipMemcpyAsync(w.x, prefix_embeds, (size_t)nseq * S * D * 4, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(rescore_state_kernel, dim3(1), dim3(1), 0, st, w.state, 0, S - 1);
        hipLaunchKernelGGL(rescore_first_kernel, dim3((nseq + 255) / 256), dim3(256), 0, st, (const long long*)codes, max_codes, clen, tgt, qlen, nseq);
        HIP_TRY(hipGetLastError());
        MqAlign mq{};
        mq.pairs = pr; mq.n_pairs = n_pairs; mq.span = span; mq.out = align_out; mq.out_rows = max_codes; mq.text_cap = text_cap;
        mq.q_len = qlen; mq.qpos_ptr = w.state + 6; mq.q_row0 = S - 1; mq.nq = 1; mq.row0 = 0;
        bool pending = false;
        if ((rc = run_layers(h, w, nseq, S, Tmax, true, w.state + 1, w.pad, &pending, st, false, 1, nullptr, nullptr, nullptr, align ? &mq : nullptr))) return rc;
        if ((rc = run_head(h, w, nseq, S, S - 1, pending, st))) return rc;
        LogpGatherArgs lg{};
        lg.logits = w.logits; lg.ldl = V; lg.targets = tgt; lg.out = lp; lg.rows = nseq; lg.V = V;
        if ((rc = launch_logp_gather(lg, st))) return rc;
        hipLaunchKernelGGL(rescore_scatter_kernel, dim3(nseq), dim3(64), 0, st, lp, 1, logp_out, max_codes, 0);
        // ---- the codes, `chunk` positions at a time ----
        for (int i0 = 1; i0 < Lmax; i0 += chunk) {
            const int n = Lmax - i0 < chunk ? Lmax - i0 : chunk, rows = nseq * n;
            hipLaunchKernelGGL(rescore_state_kernel, dim3(1), dim3(1), 0, st, w.state, S - 1 + i0, S - 1 + i0);
            hipLaunchKernelGGL(rescore_embed_kernel, dim3(n, nseq), dim3(256), 0, st, (const long long*)codes, max_codes, clen, i0, n, pos_offset, V,
                               h->mel_emb, h->mel_pos, w.x, D, tgt, qlen);
            HIP_TRY(hipGetLastError());
            mq.q_row0 = 0; mq.nq = n; mq.row0 = i0;
            if ((rc = run_layers(h, w, nseq, n, Tmax, true, w.state + 1, w.pad, &pending, st, false, 1, nullptr, nullptr, nullptr, align ? &mq : nullptr))) return rc;
            LnArgs ln{};
            ln.x = w.x; ln.g1 = h->lnf_g; ln.b1 = h->lnf_b; ln.g2 = h->fn_g; ln.b2 = h->fn_b; ln.out = hl; ln.out_f32 = 0;
            ln.rows = rows; ln.D = D; ln.in_row_mul = 1; ln.in_row_add = 0; ln.eps = c.ln_eps; ln.nsplit = 1;
            if ((rc = launch_ln(ln, prec, st))) return rc;
            GemmArgs g{};
            g.A = hl; g.lda = D; g.Wp = h->w_head; g.bias = h->b_head; g.M = rows; g.N = V; g.K = D; g.nsplit = 1;
            g.epi = EPI_STORE_F32; g.out_f32 = logits; g.ldo = V; g.D = D;
            if ((rc = launch_gemm(g, prec, rows >= 32, st))) return rc;      // the tile kernels from 32 rows on, the decode kernels below
            lg.logits = logits; lg.rows = rows;
            if ((rc = launch_logp_gather(lg, st))) return rc;
            hipLaunchKernelGGL(rescore_scatter_kernel, dim3(nseq), dim3(64), 0, st, lp, n, logp_out, max_codes, i0);
            HIP_TRY(hipGetLastError());
        }
    }
    HIP_TRY(hipGetLastError());
    if ((rc = stream_leave(h, cs))) return rc;                          // (synchronises: `code_lens` is pageable host memory)
    return ITTS_OK;
}

// the two kernels of the rescoring pass as unit ops (tests/test_gpu_rescore_kernels.py)
extern "C" int itts_gpt_logp_gather_forward(const float* logits, const int64_t* targets, float* out, int rows, int V, int ldl, void* stream) {
    if (rows < 0) { itts_set_error("gpt_logp_gather_forward: rows = %d", rows); return ITTS_ERR_ARG; }
    LogpGatherArgs lg{};
    lg.logits = logits; lg.ldl = ldl; lg.targets = (const long long*)targets; lg.out = out; lg.rows = rows; lg.V = V;
    return launch_logp_gather(lg, (hipStream_t)stream);
}

extern "C" int itts_gpt_attention_align_mq_forward(const float* q, const void* kcache, float* out, const int32_t* span, const int32_t* heads, int n_heads,
                                                   const int32_t* pos_ptr, const int32_t* pad, const int32_t* pos_shift, const int32_t* seq_map,
                                                   const int32_t* q_len, int nseq, int n_heads_model, int nq, int Tmax, int seq_mul, int row0,
                                                   int out_rows, int text_cap, int precision, void* stream) {
    if (!q || !kcache || !out || !span || !heads || !pos_ptr) { itts_set_error("gpt_attention_align_mq_forward: null pointer"); return ITTS_ERR_ARG; }
    if (precision != PREC_F32 && precision != PREC_BF16) {
        itts_set_error("gpt_attention_align_mq_forward: precision %d (0 f32 or 1 bf16)", precision);
        return ITTS_ERR_ARG;
    }
    if (nseq < 1 || n_heads_model < 1 || n_heads < 1 || n_heads > ALIGN_MAX_PAIRS || nq < 1 || Tmax < 1 || seq_mul < 0) {
        itts_set_error("gpt_attention_align_mq_forward: nseq=%d heads=%d n_heads=%d (1..%d) nq=%d Tmax=%d seq_mul=%d out of range", nseq, n_heads_model,
                       n_heads, ALIGN_MAX_PAIRS, nq, Tmax, seq_mul);
        return ITTS_ERR_ARG;
    }
    AlignMqArgs am{};
    for (int i = 0; i < n_heads; ++i) {
        for (int j = 0; j < i; ++j)
            if (heads[j] == heads[i]) { itts_set_error("gpt_attention_align_mq_forward: head %d is listed twice", heads[i]); return ITTS_ERR_ARG; }
        am.head[i] = heads[i]; am.kidx[i] = i;
    }
    am.n_heads = am.n_pairs = n_heads;
    am.qbuf = q; am.q_stride = nq; am.kcache = kcache; am.pad = pad; am.pos_ptr = pos_ptr; am.pos_shift = pos_shift; am.seq_map = seq_map;
    am.seq_mul = seq_mul; am.q_len = q_len; am.span = span; am.out = out; am.nseq = nseq; am.nq = nq; am.row0 = row0; am.out_rows = out_rows;
    am.H = n_heads_model; am.Tmax = Tmax; am.D = n_heads_model * 64; am.text_cap = text_cap;
    return launch_attention_align_mq(am, precision, (hipStream_t)stream);
}

extern "C" int itts_gemm_tile_occupancy(int precision, int32_t* blocks_per_cu) {
    if (!blocks_per_cu) { itts_set_error("gemm_tile_occupancy: null"); return ITTS_ERR_ARG; }
    int n = 0;
    const int rc = gemm_tile_occupancy(precision, &n);
    *blocks_per_cu = n;
    return rc;
}

// ---- which kernel the calling thread's last GEMM launch took (gpt_kernels.h GemmPath) ----
extern "C" const char* itts_gemm_last_path(void) {
    const char* n = gemm_path_name(gemm_last_path());
    return n ? n : "none";
}
extern "C" int itts_gemm_path_count(void) { return GP_COUNT; }
extern "C" const char* itts_gemm_path_name(int index) { return gemm_path_name(index); }

// ---- unit-level entry points (parity tests) --------------------------------------------------------------------
extern "C" int itts_gemm_forward(const void* A, const void* Wp, const float* bias, float* out, int M, int N, int K,
                                 int precision, int prefill_tiles, int gelu, void* stream) {
    if (!A || !Wp || !out) { itts_set_error("gemm_forward: null pointer"); return ITTS_ERR_ARG; }
    GemmArgs g{};
    g.A = A; g.lda = K; g.Wp = Wp; g.bias = bias; g.M = M; g.N = N; g.K = K; g.nsplit = 1; g.D = N;
    g.epi = EPI_STORE_F32; g.out_f32 = out; g.ldo = N;
    (void)gelu;
    return launch_gemm(g, precision, prefill_tiles != 0, (hipStream_t)stream);
}

// ---- which kernel the calling thread's last attention launch took (gpt_kernels.h AttnPath) ----
extern "C" const char* itts_attention_last_path(void) {
    const char* n = attention_path_name(attention_last_path());
    return n ? n : "none";
}
extern "C" int itts_attention_path_count(void) { return AP_COUNT; }
extern "C" const char* itts_attention_path_name(int index) { return attention_path_name(index); }

extern "C" int itts_gpt_attention_forward(const float* q, const void* kcache, const void* vcache, void* out, const int32_t* pos_ptr,
                                          const int32_t* pad, const int32_t* pos_shift, const int32_t* seq_map, const int32_t* row_map,
                                          const int32_t* row_map_alt, const int32_t* step_ptr, int nseq, int heads, int nq, int Tmax, int seq_mul,
                                          int precision, void* stream) {
    if (!q || !kcache || !vcache || !out || !pos_ptr) { itts_set_error("gpt_attention_forward: null pointer"); return ITTS_ERR_ARG; }
    if (precision != PREC_F32 && precision != PREC_BF16) {
        itts_set_error("gpt_attention_forward: precision %d (0 f32 or 1 bf16; the KV-cache attention has no fp32x3 form)", precision);
        return ITTS_ERR_ARG;
    }
    if (nseq < 1 || heads < 1 || nq < 1 || nq > 65535 || Tmax < 1 || seq_mul < 0) {
        itts_set_error("gpt_attention_forward: nseq=%d heads=%d nq=%d (1..65535) Tmax=%d seq_mul=%d out of range", nseq, heads, nq, Tmax, seq_mul);
        return ITTS_ERR_ARG;
    }
    if ((long long)nseq * heads > 0x7fffffffLL) { itts_set_error("gpt_attention_forward: nseq * heads = %lld blocks", (long long)nseq * heads); return ITTS_ERR_ARG; }
    if ((row_map_alt || step_ptr) && !(row_map && row_map_alt && step_ptr)) {
        itts_set_error("gpt_attention_forward: row_map_alt and step_ptr come together, and with a row_map");
        return ITTS_ERR_ARG;
    }
    AttnArgs at{};
    at.qbuf = q; at.kcache = kcache; at.vcache = vcache; at.pad = pad; at.pos_ptr = pos_ptr; at.pos_shift = pos_shift;
    at.row_map = row_map; at.row_map_alt = row_map_alt; at.step_ptr = step_ptr;
    at.out = out; at.nseq = nseq; at.H = heads; at.nq = nq; at.Tmax = Tmax; at.D = heads * 64; at.seq_mul = seq_mul; at.seq_map = seq_map;
    return launch_attention(at, precision, (hipStream_t)stream);
}

// The alignment export as a unit op: the launcher run_layers calls, on caller-supplied operands (tests/test_gpu_align_matrix.py)
extern "C" int itts_gpt_attention_align_forward(const float* q, const void* kcache, float* out, const int32_t* span, const int32_t* heads, int n_heads,
                                                const int32_t* pos_ptr, const int32_t* pad, const int32_t* pos_shift, const int32_t* seq_map,
                                                const int32_t* row_slot, const int32_t* step_ptr, const int32_t* row_step0, const int32_t* row_limit,
                                                const uint8_t* finished, int nseq, int n_heads_model, int Tmax, int seq_mul, int max_new, int text_cap,
                                                int precision, void* stream) {
    if (!q || !kcache || !out || !span || !heads || !pos_ptr || !step_ptr) { itts_set_error("gpt_attention_align_forward: null pointer"); return ITTS_ERR_ARG; }
    if (precision != PREC_F32 && precision != PREC_BF16) {
        itts_set_error("gpt_attention_align_forward: precision %d (0 f32 or 1 bf16)", precision);
        return ITTS_ERR_ARG;
    }
    if (nseq < 1 || n_heads_model < 1 || n_heads < 1 || n_heads > ALIGN_MAX_PAIRS || Tmax < 1 || seq_mul < 0 || max_new < 1) {
        itts_set_error("gpt_attention_align_forward: nseq=%d heads=%d n_heads=%d (1..%d) Tmax=%d seq_mul=%d max_new=%d out of range", nseq, n_heads_model,
                       n_heads, ALIGN_MAX_PAIRS, Tmax, seq_mul, max_new);
        return ITTS_ERR_ARG;
    }
    AlignArgs al{};
    for (int i = 0; i < n_heads; ++i) {
        for (int j = 0; j < i; ++j)
            if (heads[j] == heads[i]) { itts_set_error("gpt_attention_align_forward: head %d is listed twice", heads[i]); return ITTS_ERR_ARG; }
        al.head[i] = heads[i]; al.kidx[i] = i;
    }
    al.n_heads = al.n_pairs = n_heads;
    al.qbuf = q; al.kcache = kcache; al.pad = pad; al.pos_ptr = pos_ptr; al.pos_shift = pos_shift; al.seq_map = seq_map; al.seq_mul = seq_mul;
    al.row_slot = row_slot; al.step_ptr = step_ptr; al.row_step0 = row_step0; al.row_limit = row_limit; al.finished = finished;
    al.span = span; al.out = out; al.nseq = nseq; al.H = n_heads_model; al.Tmax = Tmax; al.D = n_heads_model * 64; al.max_new = max_new;
    al.text_cap = text_cap;
    return launch_attention_align(al, precision, (hipStream_t)stream);
}

extern "C" int itts_gemm_ln_forward(const float* x, const float* partial, const float* bias_prev, const float* ln_gamma, const float* ln_beta,
                                    float eps, const void* Wp, const float* bias, float* out, float* x_out, int M, int N, int K, void* stream) {
    if (!x || !ln_gamma || !ln_beta || !Wp || !out) { itts_set_error("gemm_ln_forward: null pointer"); return ITTS_ERR_ARG; }
    if (!gemm_decode_ln_ok(M, K, EPI_STORE_F32)) { itts_set_error("gemm_ln_forward: M = %d (1..16), K = %d (256, 512, 1280) unsupported", M, K); return ITTS_ERR_ARG; }
    GemmArgs g{};
    g.Wp = Wp; g.bias = bias; g.M = M; g.N = N; g.K = K; g.nsplit = 1; g.D = N;
    g.epi = EPI_STORE_F32; g.out_f32 = out; g.ldo = N;
    g.ln_x = x; g.ln_partial = partial; g.ln_bias_prev = bias_prev; g.ln_g = ln_gamma; g.ln_b = ln_beta; g.ln_eps = eps; g.ln_x_out = x_out;
    return launch_gemm_decode_ln(g, (hipStream_t)stream);
}

extern "C" int itts_layernorm_forward(const float* x, const float* gamma, const float* beta, const float* gamma2,
                                      const float* beta2, float* out, int rows, int D, float eps, void* stream) {
    if (!x || !gamma || !beta || !out) { itts_set_error("layernorm_forward: null pointer"); return ITTS_ERR_ARG; }
    LnArgs ln{};
    ln.x = const_cast<float*>(x); ln.g1 = gamma; ln.b1 = beta; ln.g2 = gamma2; ln.b2 = beta2; ln.out = out; ln.out_f32 = 1;
    ln.rows = rows; ln.D = D; ln.in_row_mul = 1; ln.in_row_add = 0; ln.eps = eps; ln.nsplit = 1;
    return launch_ln(ln, PREC_F32, (hipStream_t)stream);
}
