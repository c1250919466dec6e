// librdx internals shared by the api_*.hip translation units: the context, the weight registry and the host-side GEMM dispatch.
// (The public C ABI is include/rdx.h; the kernel launchers are rdx_kernels.h.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/rdx.h"
#include "rdx_common.h"
#include "rdx_kernels.h"

using namespace rdx;

// decoder rows per context: batch 1-2 chained launches, 3-16 xs16.hip, 3-32 xstat32.hip, 33-128 the row-block family (NB = ceil(rows / 32) row blocks per
// tile walker sharing an XCD's L2: xstat32_k / xsplit32_k<.., BLK>; fp8 weights: the 32-row fp8 kernels per block). 128 rows x 512 slots of KV = 68 GB of the 288.
constexpr int RDX_MAX_ROWS = 128;

struct GemmW {
    void* w = nullptr; int N = 0, K = 0, Npad = 0; void* w8 = nullptr; float* scale = nullptr;   // w8/scale: fp8 copy
    void* wc = nullptr; unsigned* wch = nullptr;     // coded bf16 copy of w (13 bits per weight, exact) and its per-tile header words: what the batch <= 2 GEMV streams
    // RDX_W_GEMM_W4: w is the packed copy of the DEQUANTISED weight W' (what every kernel but the batch <= 16 steps' QKV, gate/up and down_proj reads); w4 / w4h: the int4 stream and
    // its per-tile header words (bit 8: a raw tile, the LoRA-A rows of wqkv). A weight with an int4 stream gets no coded copy.
    void* w4 = nullptr; unsigned* w4h = nullptr;
};
struct RawW { void* p = nullptr; int64_t rows = 0, cols = 0; };

struct LlamaLayer {
    const void *attn_norm, *mlp_norm, *lora_bq, *lora_bv;
    GemmW wqkv, wo, wgu, wdown;
};
struct QLayer {
    GemmW s_wqkv, s_wo, c_wq, c_wo, w1, w2;
    const float *s_bqkv, *s_bo, *s_g, *s_b, *c_bq, *c_bo, *c_g, *c_b, *b1, *b2, *f_g, *f_b;
    int cross_idx;     // -1 = no cross attention in this layer
};
struct VBlock {
    GemmW c1, c2, c3, ds;
    const float *b1, *b2, *b3, *bds;
    bool has_ds;
    int planes, stride;
};

struct PoolBlock {          // one VisionTransformerPooler block (two-image mode)
    const float *n1_g, *n1_b, *n2_g, *n2_b, *bo, *b1, *b2;
    GemmW wqkv, wo, w1, w2;
};

struct GraphKey {
    int B = -1, max_new = 0, eos = 0, pad = 0;
    const void* tokens = nullptr; const void* scores = nullptr;
    bool fixed = false;             // logits always to `scores` itself (beam search) instead of scores + step * stride
    rdx_logits_rules rules = {1.0f, 0, 0};      // the captured step selects through select_step_k unless neutral
    rdx_sampling sampling = {0, 1.0f, 0, 1.0f, 0};      // do_sample: through sample_step_k, t / k / p its arguments; the seed is no part of the key (a device word)
    int logprobs = -1;              // rdx_set_logprobs: >= 0: logprob_step_k rides behind the selection with this top_n
    const void* lookup = nullptr;   // rdx_generate_lookup's plain step: the context's corpus buffer (never null there); the selection is lookup_accept_k
    bool operator==(const GraphKey& o) const {
        return lookup == o.lookup && logprobs == o.logprobs && B == o.B && max_new == o.max_new && eos == o.eos && pad == o.pad && tokens == o.tokens && scores == o.scores && fixed == o.fixed &&
               rules.repetition_penalty == o.rules.repetition_penalty && rules.no_repeat_ngram_size == o.rules.no_repeat_ngram_size &&
               rules.min_new_tokens == o.rules.min_new_tokens && sampling.do_sample == o.sampling.do_sample &&
               sampling.temperature == o.sampling.temperature && sampling.top_k == o.sampling.top_k && sampling.top_p == o.sampling.top_p;
    }
};

// The runtime switches of one context, one int each (a bool holds 0 / 1). What each selects, its environment variable, default, range and when it may be
// set stand in ONE table: api_options.hip. The environment is read once, at rdx_create; after that only rdx_set_option changes a value.
struct Switches {
    int fuse_ao, chain, flash_min, xs16, prompt_blk, blk_down, pconv, pconv_ksplit, kperm, wcode, w4, kv_fp8, score_chunk;
    int att_tp, att_mid, xdup, ws_cfg, beam_fullcopy, eos_poll;
};

struct rdx_ctx {
    rdx_config cfg;
    Switches sw = {};                // defaults and the environment: options_from_env (api_options.hip), called by rdx_create
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool finalized = false;
    std::vector<void*> allocs;

    std::map<std::string, GemmW> gemm;
    std::map<std::string, RawW> tens;     // model dtype
    std::map<std::string, RawW> f32;

    // ---- llama ----
    std::vector<LlamaLayer> ll;
    const void *embed = nullptr, *final_norm = nullptr, *rope_cos = nullptr, *rope_sin = nullptr;
    GemmW lm_head, img_proj_w;
    const float* img_proj_b = nullptr;
    LlamaDims ld;
    void *kcache = nullptr, *vcache = nullptr;     // [layers][B][heads][max_len][D]
    size_t kv_layer_elems = 0;
    // fp8 KV cache (sw.kv_fp8; the format: radialog_amd/kv8.py): kcache / vcache then hold the e4m3 codes, one BYTE
    // per element (K in the kperm8 order of rdx_common.h, V row-major), kexp / vexp the row exponents [layers][B][heads][max_len]; kv_kstage / kv_vstage:
    // the prompt's K / V rows of ONE layer in the model dtype, [B][heads][ceil16(T)][128] row-major -- what the prompt's own attention reads
    signed char *kexp = nullptr, *vexp = nullptr;
    void *kv_kstage = nullptr, *kv_vstage = nullptr;
    size_t kv_alloc_bytes = 0;                     // bytes of the KV allocation (caches, exponents; the staging buffer is not part of it): rdx_kv_bytes
    uint8_t* key_mask = nullptr;                   // [B][max_len]
    int *d_img_pos = nullptr, *d_pos_ids = nullptr, *d_pos = nullptr, *d_slot = nullptr, *d_step = nullptr, *d_unf = nullptr;
    float* part_val = nullptr; int* part_idx = nullptr; int n_vtiles = 0;
    // decode-step activations ([max_batch] rows) and prefill activations (grown on demand)
    void *dx = nullptr, *dxn = nullptr, *dqkv = nullptr, *datt = nullptr, *dgu = nullptr;
    float* dxs = nullptr;            // fp8 path, batch 3-128 decode: xscale[rows in 32-row blocks] of the e4m3 activation block(s) in dxn (ACT_BLK64_E4M3)
    void* pxq = nullptr; float* pxs = nullptr;   // fp8 path, prefill: e4m3 activations [rows][max(hidden, inter)] and their scales [rows][4]
    std::string unsupported;         // set by the dispatch when a shape has no kernel in the current mode (fp8 weights); reported by the entry points
    float* kslab = nullptr;          // batch 3-32 decode: fp32 partial slabs [<= 4 groups][32][hidden] of a K-split projection
    int pend_groups = 0;             // launch-time state: slabs written by the last xsplit32 launch, not yet added into dx
    void *px = nullptr, *pxn = nullptr, *pqkv = nullptr, *pq = nullptr, *patt = nullptr, *pgu = nullptr, *pqe = nullptr, *pimg = nullptr;
    size_t prefill_rows = 0;
    float* pslab = nullptr;          // one prompt's prefill (<= 192 rows): fp32 slabs [4][rows][hidden] of the K-split down_proj (xsplit32_k<.., BLK>)
    int cur_B = 0, cur_T = 0, cur_max_new = 0, cur_eos = -1, cur_pad = 0;
    int cur_steps = 0;               // tokens selected since the last prefill (1 after it): bounds rdx_decode_step
    int32_t* cur_tokens = nullptr;
    hipGraphExec_t graph = nullptr;
    int* w4_bad = nullptr;           // device flag of the int4 quantiser: the weight held an Inf / NaN
    bool has_fp8_w = false, has_w4_w = false;     // kinds of GEMM weights set so far (RDX_W_GEMM_FP8 and RDX_W_GEMM_W4 do not mix)
    // launches this context issued, by kernel and by the copy it streamed, counted where the choice is made (api_dispatch.hip skinny / launch_chain /
    // launch_xs16; a captured graph counts once). The coded and int4 columns are what rdx_wcode_stats, rdx_w4_stats and rdx_w4_rows_stats report.
    enum WKernel { WK_GEMV, WK_CHAIN, WK_XSTAT16, WK_XROW16, WK_COUNT };
    long long n_stream[WK_COUNT][3] = {};         // [kernel][WStream]
    int chain_naps = 1;             // poll back-off of the chained launch (x s_sleep(8) between polls)
    long long* chain_trace = nullptr; int chain_trace_layer = -1;     // rdx_gemv_trace(7): device timeline buffer of ONE chained launch of the next step
    long long* ao_trace = nullptr; int ao_trace_layer = -1;           // rdx_gemv_trace(8): the same for ONE fused attention + o_proj launch
    GemmW cls_fc1, cls_fc2; const float *cls_fc1_b = nullptr, *cls_fc2_b = nullptr;   // findings classifier head
    void *cls_pooled = nullptr, *cls_h = nullptr, *cls_out = nullptr;
    void* zero16 = nullptr;          // 16 zero bytes: source of padding taps in the DMA conv gather
    void* d_cur_rope = nullptr;      // [B][2][128] cos | sin row of each row's current position (written by greedy_step_k)
    int* d_cctr = nullptr;
    int *d_ctr = nullptr, *d_err = nullptr;   // hand-off counters of the chained launches (= d_cctr), sticky error flag
    void* d_gran = nullptr; int *d_hint = nullptr, *d_epoch = nullptr;   // fused attention + o_proj launch: tagged-granule buffer [2][hidden] x 4 B, hint words, step epoch (handoff.h)
    bool ws_ok = false;              // set while the image encoder runs: its many-row GEMMs / convolutions may take wsgemm_k
    float* gemm_ws = nullptr; size_t gemm_ws_floats = 0;      // split-K slabs of gemm_dma_k
    GraphKey gkey;
    // ---- logits rules of the greedy search (rdx_set_logits_rules); the buffers exist from the first active rule on ----
    rdx_logits_rules rules = {1.0f, 0, 0};
    bool hist_ready = false;                        // the last prefill ran under the current rules and filled the history
    bool rules_on = false;                          // any rule differs from neutral: the step selects through select_step_k (elem.hip)
    int *d_hist = nullptr, *d_hist_len = nullptr;   // [max_batch][max_len] token history (index = cache slot), [max_batch] its lengths
    void* rule_logits = nullptr;                    // [max_batch][vocab]: where the lm_head writes when the caller passes no logits / scores buffer
    // ---- sampled decoding (rdx_set_sampling): do_sample == 0 = off; on: the step selects through sample_step_k (elem.hip), rules included ----
    rdx_sampling sampling = {0, 1.0f, 0, 1.0f, 0};
    unsigned long long* d_seed = nullptr;           // the seed word sample_step_k reads (rewritten in stream order by every rdx_set_sampling call)

    // ---- generation log-probs (rdx_set_logprobs): -1 = off; 0 .. 8 = on with that many alternatives: logprob_step_k (logprob.hip) behind every selection ----
    int logprobs = -1;
    float* lp_chosen = nullptr;                     // [max_batch][max_len]: entry [row][step] of the current conversation
    int* lp_top_ids = nullptr; float* lp_top_lp = nullptr;      // [max_batch][max_len][RDX_MAX_TOP_LOGPROBS]; allocated once, so a captured graph keeps its pointers

    // ---- prompt-lookup decoding (rdx_set_lookup / rdx_generate_lookup, api_lookup.hip; kernel: lookup.hip); the buffers exist from the first rdx_set_lookup on ----
    rdx_lookup lookup = {0, 0, 0};                  // draft_len 0 = off
    bool lk_run = false;                            // inside rdx_generate_lookup: lm_head_and_greedy selects through lookup_accept_k, the prefill starts the history
    int *lk_tail = nullptr, *lk_status = nullptr, *lk_trace = nullptr, *lk_par = nullptr;      // rdx_kernels.h LookupArgs
    int* lk_corpus = nullptr; size_t lk_corpus_cap = 0;      // the caller's corpus, grown on demand
    float* lk_part_val = nullptr; int* lk_part_idx = nullptr;      // argmax partials [16][n_vtiles] of a verify pass
    void* lk_logits = nullptr;                      // [16][vocab]: a verify pass's logits rows when the caller wants scores
    void* lk_scores = nullptr;                      // the running call's scores buffer
    int lk_par_host[LKP_INTS] = {};                 // source of the asynchronous copy into lk_par

    // ---- scoring pass (rdx_score), sized on first use ----
    void *sc_x = nullptr, *sc_xn = nullptr;         // [rows][hidden]: the gathered residual rows and their final RMSNorm
    void* sc_logits = nullptr;                      // [chunk rows][lm_head.Npad]: the one chunk of logits the library ever holds
    int* sc_idx = nullptr;                          // rows[n] | target[n] | dst[n] | ldst[n]: the host-built index lists of one call
    float* sc_lp = nullptr; int* sc_t1 = nullptr;   // [rows] compact results, scattered to [batch][T] by one launch
    size_t sc_rows = 0, sc_ws_rows = 0;

    // ---- beam search workspaces (rdx_beam_search), sized on first use ----
    void* bm_logits = nullptr; float* bm_scores = nullptr; float* bm_cand_s = nullptr; int* bm_cand_i = nullptr;
    int *bm_tok = nullptr, *bm_src = nullptr; int32_t* bm_out = nullptr; void* bm_scratch = nullptr;
    size_t bm_scratch_bytes = 0; int bm_rows = 0, bm_new = 0;

    // ---- row session (rdx_rows_*, api_rows.hip): `rs_rows` live rows refilled one by one through `rs_stage` staging rows above them ----
    bool rs_on = false;
    int rs_rows = 0, rs_stage = 0, rs_cap = 0;
    int32_t* rs_stage_tok = nullptr; size_t rs_stage_tok_ints = 0;     // [stage][cap]: where the staged prompts' token 0 lands
    // the host mirror of every live row: deterministic (slot = T at refill, + 1 per step; step = tokens selected), only `unfinished` needs the poll
    std::vector<int> rs_slot, rs_step, rs_state;                       // rs_state: RS_PARKED / RS_LIVE / RS_DONE (a poll saw the row finished)

    void* tf_ws = nullptr; size_t tf_bytes = 0;      // rdx_transform_image: coefficient tables + the horizontal pass's uint8 rows (grown on demand)

    // ---- data-parallel collective (RCCL over xGMI): the one all-gather of generated token ids ----
    void* comm = nullptr; int comm_rank = 0, comm_world = 0;

    // ---- q-former ----
    std::vector<QLayer> ql;
    const void* q_query_ln = nullptr;
    GemmW q_wkv; const float* q_bkv = nullptr; int n_cross = 0;
    // ---- vision ----
    GemmW v_conv1, v_b2v, v_p1, v_p2;
    const float *v_conv1_b = nullptr, *v_p1_b = nullptr, *v_p2_b = nullptr, *v_ln_g = nullptr, *v_ln_b = nullptr;
    std::vector<VBlock> vb;
    std::vector<PoolBlock> pool;                    // optional: present when the pooler weights were uploaded
    const void* pool_emb = nullptr;                 // [2*P][b2v] pos + type embedding (model dtype)
    const float *pool_ng = nullptr, *pool_nb = nullptr, *v_p1f_b = nullptr;
    GemmW v_p1f;                                    // projector conv-1 over the full 2*b2v channels (two-image mode)
    float pool_eps = 1e-6f;
    int enc_batch = 0;
    void *vin = nullptr, *vbuf[4] = {nullptr, nullptr, nullptr, nullptr}, *v_imgemb = nullptr;
    void *qx = nullptr, *qt = nullptr, *qqkv = nullptr, *qctx = nullptr, *qh = nullptr, *qkvx = nullptr;
};

int fail(rdx_ctx* c, int code, const char* fmt, ...);
const char* create_error();
int options_from_env(rdx_ctx* c);      // (api_options.hip) every switch to its default or its environment variable's value; nonzero: a value out of range, c->err says which
inline DecAttnSw attn_sw(const rdx_ctx* c) { return DecAttnSw{c->sw.att_tp, c->sw.att_mid}; }

#define HIPCHK(c, call)                                                                         \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return fail((c), -2, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

inline size_t esz(const rdx_ctx* c) { (void)c; return 2; }

int dalloc(rdx_ctx* c, void** p, size_t bytes);
#define ALLOC(c, ptr, bytes) do { int rc_ = dalloc((c), (void**)&(ptr), (bytes)); if (rc_) return rc_; } while (0)

// release a buffer obtained with ALLOC before it is replaced (workspaces that grow with the batch / prompt length)
template <typename P>
inline void dfree(rdx_ctx* c, P*& p) {
    if (!p) return;
    auto it = std::find(c->allocs.begin(), c->allocs.end(), (void*)p);
    if (it != c->allocs.end()) c->allocs.erase(it);
    hipFree((void*)p);
    p = nullptr;
}

// ---- host-side GEMM dispatch (api_dispatch.hip) ----
GemmArgs gargs(const void* X, int ldx, const GemmW& W, const float* bias, void* out, int ldo, int M);
// the switches that travel in the arguments: every GemmArgs that may reach xstat32_k / xsplit32_k passes here (the decode and prompt unit builders, skinny(), the hooks that launch those kernels)
inline GemmArgs with_switches(const rdx_ctx* c, GemmArgs a) { a.xdup_off = c->sw.xdup ? 0 : 1; return a; }
GemmArgs skinny_prenorm(rdx_ctx* c, GemmArgs a, int epi);
void skinny(rdx_ctx* c, GemmArgs a, int epi);
void launch_ksplit(rdx_ctx* c, const GemmArgs& a);
// ---- the decode step's units (api_dispatch.hip): ONE definition of each unit's arguments for the step (api_llama.hip), the probes, the timers (rdx_time) and the trace hooks ----
enum DecUnit { UNIT_QKV, UNIT_O, UNIT_GATE_UP, UNIT_DOWN, UNIT_LM_HEAD };
// the kernel family the step takes at B rows: batch <= 2 chained (both switches on), generic (GEMV; from 3 rows the 32-row xstat32 / xsplit32 kernels), 3-16 rows
// xs16.hip, 33-128 rows the row blocks in the model dtype or with fp8 weights
enum DecFamily { DEC_UNSUPPORTED, DEC_CHAINED, DEC_GENERIC, DEC_XS16, DEC_BLK, DEC_BLK8 };
DecFamily decode_family(rdx_ctx* c, int B);
DecAttnArgs dec_attn_args(rdx_ctx* c, int layer);                                  // decode attention; callers set out_packed / out_mt / trace
// a unit in its base form: row-major activations, the RMSNorm in front of QKV / gate-up / lm_head as the kernel's prologue (norm_w), the residual of o_proj /
// down_proj as its epilogue. L may be null for UNIT_LM_HEAD, whose callers set X (when not dx), out and out_step.
GemmArgs unit_args(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B);
// Which copy of a unit's weight a family streams (WStream, rdx_kernels.h): ONE table, stream_wants in api_dispatch.hip ("Which copy of
// a weight each unit streams"). unit_stream: the table's entry for (family, unit, layer), narrowed to what the options ("w4", "wcode"; bf16 only) allow and W
// holds. Of the chained family, UNIT_DOWN and UNIT_QKV of layers >= 1 are the two roles of the chained launch (chain_args), UNIT_QKV of layer 0 the
// stand-alone launch. The table says what a family wants; whether a kernel takes the arguments stays with its own *_supported predicate.
WStream unit_stream(rdx_ctx* c, DecFamily fam, DecUnit u, int layer, const GemmW& W);
bool stream_wanted(DecUnit u, int layer, WStream s);      // some family's entry for (unit, layer) names s: what rdx_finalize_weights keeps and encodes
struct StreamW { DecUnit u; int layer; GemmW* W; };
std::vector<StreamW> stream_weights(rdx_ctx* c);           // (api.hip) every decoder weight that can hold a stream: the lm_head, then each layer's four projections
// ... and in the layout of a family, with the copy that family streams attached (what its probe checks IS what its step function, the timers and the trace
// hooks launch). A family's builder is for code that has decided the family: it does not ask decode_family.
// the chained family's stand-alone launches: layer 0's QKV (the timers run that launch on every layer's weight), gate/up and the step's lm_head; o_proj (in
// the fused launch) and down_proj (a role of the chained launch) have none and come back in their base form
GemmArgs chained_unit(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B);
GemmArgs xs16_unit(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B);      // one row tile: gate/up writes, o_proj / down_proj read the fragment-packed block
ChainArgs chain_args(rdx_ctx* c, int l, int B);           // the chained launch of layer l: down_proj(l), norm + QKV(l + 1) (none behind the last layer), their stream
// The launches that choose between copies of a weight choose once and count what they chose (rdx_ctx::n_stream), for the step, the timers and the trace hooks:
// skinny() (launch_skinny_gemm's choice: the raw, coded or int4 GEMV, or xstat32_k) and
void launch_chain(rdx_ctx* c, int l, int B);                                // launch_decode_chain on chain_args (+ the trace pointer of rdx_gemv_trace 7)
void launch_xs16(rdx_ctx* c, const GemmArgs& a, int epi);                   // xstat16_k (norm-prologue units) / xrow16_k (EPI_RESID), or their int4 forms
GemmArgs blk_unit(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B);       // row blocks: fragment-packed row tiles of 16 in and (gate/up) out
GemmArgs blk8_unit(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B);      // ... fp8 weights: e4m3 blocks + xscale in; 64-deep model-dtype blocks into the K-split o_proj / down_proj
GemmArgs ksplit_args(GemmArgs a);                  // o_proj / down_proj K-split at 3-32 rows: X is the fragment-packed 32-row block (fp8 weights: 64-deep)
GemmArgs prenormed(rdx_ctx* c, GemmArgs a);        // the unit's RMSNorm is a launch of its own: the kernel reads the normalised rows from dxn
// The RMSNorm in front of a unit whose kernel does not fuse it: a.X normalised by a.norm_w into dxn, in the layout a.xpacked / a.mtiles name. Slabs that a K-split
// projection left pending on dx are folded in (dx += T(sum of slabs)) and pend_groups is cleared. Returns prenormed(c, a), the arguments of the GEMM proper.
GemmArgs norm_in_front(rdx_ctx* c, GemmArgs a);
void run_rmsnorm(rdx_ctx* c, const NormArgs& n);      // launch_rmsnorm; a combination without a kernel is reported through c->unsupported (take_unsupported)
bool down_split_ok(rdx_ctx* c, const LlamaLayer& L, int B);
void launch_down(rdx_ctx* c, const LlamaLayer& L, int B, bool split);
bool blk64_ok(rdx_ctx* c, int B);      // 33-128 rows: the row-block decode family (model-dtype weights, or fp8 weights: blk64_fp8)
bool blk64_fp8(rdx_ctx* c);            // ... its fp8 form is the one in use (e4m3 decoder weights)
bool xs16_ok(rdx_ctx* c, int B);       // batch 3-16, model-dtype weights, hidden 4096: the step's projections on xs16.hip (no stand-alone RMSNorm, no K-split slabs)
// ---- the prompt's units (api_dispatch.hip), the step's idea once more: the family is decided once per prompt, and what a family's layer loop (api_llama.hip)
// launches is what the builder returned ----
// PROMPT_FP8: fp8 weights, every projection on gemm8 over e4m3 rows. PROMPT_TILES: one or two prompts on fragment-packed row tiles of 16 (wstat_k, the row-block
// xstat32_k, the K-split xsplit32_k). PROMPT_ROWS: everything else, row-major rows through run_gemm.
enum PromptFamily { PROMPT_ROWS, PROMPT_TILES, PROMPT_FP8 };
struct PromptPlan {
    PromptFamily family;
    int M, mtiles;       // rows = B x T, their row tiles of 16
    bool blk;            // PROMPT_TILES: the K = 4096 projections take the row-block kernel ("prompt_blk" on and xstat_blk_supported), else wstat_k
    bool down_split;     // PROMPT_TILES: down_proj K-split into fp32 slabs that the next RMSNorm folds in, else wstat_k
};
PromptPlan prompt_plan(rdx_ctx* c, int B, int T);
// QKV, o_proj, gate/up or down_proj of layer L on the prompt buffers (px .. pgu; fp8: pxq / pxs), in the plan's family's layout
GemmArgs prompt_unit(rdx_ctx* c, const PromptPlan& p, const LlamaLayer* L, DecUnit u);
// the RMSNorm of the residual stream px by w, in the layout the projection behind it reads; `pend` slab groups of a K-split down_proj are folded in first
void prompt_norm(rdx_ctx* c, const PromptPlan& p, const void* w, int pend);
// layer l behind its QKV projection: RoPE + the K / V rows of T prompt tokens into the cache behind `keep` kept slots, rows row0 .. row0 + B - 1, then the causal
// attention over them into patt (PROMPT_TILES: fragment-packed); an fp8 KV cache goes through its staging buffer and is quantised last
void prompt_attention(rdx_ctx* c, const PromptPlan& p, int l, int B, int T, int keep, int row0);
void run_gemm(rdx_ctx* c, GemmArgs a, int epi);
void conv_gemm(rdx_ctx* c, const void* X, const GemmW& W, const float* bias, const void* resid, void* out, int B,
               int Hin, int Win, int Cin, int KH, int KW, int stride, int pad, int Hout, int Wout, int epi);
// the fused stem (stem.hip) as the encoder runs it, packed: with the pad-row zeroing of the fragment-packed output (api_encode.hip)
int run_stem_pool(rdx_ctx* c, const void* vin, const GemmW& W, const float* bias, void* out, int B, int S, bool packed);
int v_grid(const rdx_config& f);      // side of the trunk's output grid
inline bool fp8_weights(const GemmW& W) { return W.w8 && W.scale && !W.w; }       // the engine's fp8 mode keeps no model-dtype copy
int take_unsupported(rdx_ctx* c);     // nonzero (and rdx_last_error set) when a launch since the last call had no kernel for its shape

// ---- decoder (api_llama.hip) ----
inline void* kv_ptr(rdx_ctx* c, void* base, int layer) { return (char*)base + (size_t)layer * c->kv_layer_elems * (c->sw.kv_fp8 ? 1 : 2); }
inline signed char* kvx_ptr(rdx_ctx* c, signed char* base, int layer) { return base + (size_t)layer * (c->kv_layer_elems / 128); }      // fp8 KV cache: a layer's row exponents
// decode attention of one layer on whichever cache the context holds (at from dec_attn_args)
void run_decode_attention(rdx_ctx* c, const DecAttnArgs& at, int layer, int B);
// every entry point that needs the cached rows in the model dtype refuses on an fp8 KV cache (-1, a message naming "kv_fp8")
inline int kv8_refuse(rdx_ctx* c, const char* who, const char* why) {
    return c->sw.kv_fp8 ? fail(c, -1, "%s: not built for the fp8 KV cache (kv_fp8): %s", who, why) : 0;
}
int prefill_impl(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int B, int T, const float* qformer_embs, int keep,
                 int max_new, int eos_id, int pad_id, int32_t* out_tokens, void* logits);
StepTail step_tail_args(rdx_ctx* c, int advance);
void prompt_embed_layers(rdx_ctx* c, const int32_t* ids, int B, int T, int keep, bool splice, int row0);
// (api_lookup.hip) lookup_accept_k behind a forward of d + 1 rows whose argmax partials are pv / pi; logits: the rows of a verify pass (null: written in place)
void lookup_accept(rdx_ctx* c, StepTail t, int d, const float* pv, const int* pi, const void* logits);
// evs (timing only, eager launches): a pair of events recorded around every chained down(l) -> QKV(l+1) launch of this step
bool decode_step_launch(rdx_ctx* c, void* logits, const int* out_step, long step_stride, std::vector<hipEvent_t>* evs = nullptr);
int build_graph(rdx_ctx* c, void* scores, bool fixed = false);
// R prompts of T tokens through the prompt path into rows row0 .. row0 + R - 1 of every per-row array (KV cache, decode state), token 0 of prompt r into
// tokens[r * cur_max_new]: the launches of rdx_prefill(B = R, T) on offset bases. The caller has set cur_max_new / cur_eos / cur_pad.
int prefill_rows_at(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int R, int T, const float* qformer_embs, int row0, int32_t* tokens, void* logits);
enum { RS_PARKED = 0, RS_LIVE = 1, RS_DONE = 2 };
// every conversation entry point refuses while a row session is open (-1, "rdx_rows_end first")
inline int rows_refuse(rdx_ctx* c, const char* who) { return c->rs_on ? fail(c, -1, "%s: a row session is open on this context; rdx_rows_end first", who) : 0; }

