// Host-visible launchers of librdx's HIP kernels (internal header; the public C ABI is include/rdx.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdx {

enum Epilogue {
    EPI_NONE = 0,        // out = T(acc + bias)
    EPI_RELU = 1,        // out = T(relu(acc + bias))
    EPI_GELU = 2,        // out = T(gelu_erf(acc + bias))
    EPI_RESID = 3,       // out = T(resid + T(acc + bias))
    EPI_SILU_MUL = 4,    // gate/up interleaved tiles: out[:, N/2] = T(T(silu(T(g))) * T(u))
    EPI_LOGITS = 5,      // skinny only: out = T(acc) for n < n_valid, plus per-tile argmax partials
    EPI_RESID_RELU = 6,  // tiled only: out = T(relu(resid + T(acc + bias)))   (Bottleneck tail)
};

// The memory orders of the decoder's activations, [rows][H] in the model dtype unless said otherwise. A "fragment" is what one MFMA B operand holds:
// 64 lanes x 8 elements, lane = 16 g + r with r = row % 16; a thread's 8 consecutive elements k .. k + 8 of a row are exactly one lane's piece
// (act_offset in rdx_common.h is this arithmetic). Rows past the real ones are zero.
enum ActLayout : int {
    ACT_ROWS = 0,        // row-major [rows][H]
    ACT_BLK32 = 1,       // one 32-row block in 32-deep fragments, [k / 32][2 row tiles][lane][8], g = (k % 32) / 8: ACT_TILES32 at mtiles = 2
    ACT_BLK64 = 2,       // the 32-row block in the fp8 weights' 64-deep order, [f = 2 (k / 64) + (k % 16) / 8][2][lane][8], g = (k % 64) / 16; beyond 32 rows
                         // one such block per 32 rows at a stride of 32 H elements
    ACT_TILES32 = 3,     // `mtiles` row tiles of 16 in 32-deep fragments, [k / 32][mtiles][lane][8]
    ACT_BLK64_E4M3 = 4,  // e4m3 bytes + xscale[row] (absmax / 448): chunk k / 64 = [2 row tiles][lane, g = (k % 64) / 16][16 bytes], one 32-row block per 32
                         // rows at a stride of 32 H bytes; pad rows have scale 1
    ACT_ROWS_E4M3 = 5,   // e4m3 bytes row-major [rows][H] + xscale[row] (RMSNorm output only; the input of gemm8)
};

struct GemmArgs {
    const void* X; int ldx;          // activations [M][K], row stride in elements
    const void* W;                   // fragment-packed weights (see gemm.hip)
    const float* bias;               // nullable [N]
    const void* resid; int ldr;      // nullable [M][N]
    void* out; int ldo;              // [M][N]  ([M][N/2] for EPI_SILU_MUL)
    int M, N, K;
    const void* norm_w; float eps;   // fused RMSNorm prologue (skinny): weight [K] or null
    float* part_val; int* part_idx;  // EPI_LOGITS: [M][n_tiles]
    int n_valid;                     // EPI_LOGITS: real vocab size (N is padded to 16)
    const int* out_step; long out_step_stride;   // optional: out += (*out_step) * stride elements (per-step score rows)
    // fp8 weights: e4m3 bytes in the 64-deep fragment order (gemm.hip) + one fp32 scale per output row; `W` is null in the engine (no
    // model-dtype copy exists: api_dispatch.hip refuses shapes without an fp8 kernel), only the kernel test hooks set both
    const void* W8; const float* wscale;
    ActLayout out_packed;            // EPI_SILU_MUL: the order the output is written in (see ActLayout)
    ActLayout xpacked;               // the order X is in (see ActLayout)
    int mtiles;                      // row tiles of 16 of the packed orders
    int xdup_off;                    // the context's switch "xdup" off (set by the argument builders): padding rows of a 32-row block load their own (zero / stale) lines instead of re-reading real rows
    // fp8 activations (W8A8: gemm8.hip, xstat32_k<.., A8>): X holds e4m3 bytes, xscale[row][xgroups] their absmax / 448 scales over `xgroups`
    // equal K ranges (1 behind an RMSNorm, 2 o_proj, 4 down_proj); see ActLayout
    const float* xscale; int xgroups;
    long long* trace;                // debug: [tile][8] timestamps (100 MHz ticks) written by thread 0 of every workgroup (skinny_tile)
    // coded bf16 weights (rdx_common.h WcChunk): the planes of launch_encode_wc and one header word per tile; the batch <= 2 GEMV streams them
    // instead of W (13 bits per weight, decoded exactly), W stays what the tiles flagged in their header read. Null: W is streamed.
    const void* WC; const unsigned* wchdr;
    // int4 group-quantised weights (rdx_common.h W4Chunk): the stream of launch_quant_w4 and one header word per tile (bit 8: the tile streams its
    // packed bf16 bytes from W). W is the packed bf16 copy of the dequantised weight W': the same bits, four times the bytes. Null: not streamed.
    const void* W4; const unsigned* w4hdr;
};
// which of these copies a launch streams: W, WC or W4 (the values double as ChainArgs::wc)
enum WStream { WS_RAW = 0, WS_CODED = 1, WS_W4 = 2 };

// int4 group-quantised weights (radialog_amd/w4.py): groups of 128 k of one row, per (tile, 128 k) one chunk of 1 KiB of nibbles + 16 bf16 scales
constexpr int W4_CHUNK_K = 128, W4_CHUNK_BYTES = 64 * 16 + 16 * 2;
inline size_t w4_bytes(int npad, int k) { return (size_t)(npad / 16) * (size_t)(k / W4_CHUNK_K) * W4_CHUNK_BYTES; }
// bf16 only: quantises W fp32 [N][K] (the 16-row tiles of rows [raw_lo, raw_hi), both multiples of 16, are raw: W' = bf16(W)) and
// writes the packed bf16 copy of W' (the order of launch_pack_weight, rows padded to npad with zeros), the stream and hdr[npad / 16] = raw << 8.
// *bad (device, zeroed by the caller) is set when W holds an Inf or a NaN. K % 128 == 0
void launch_quant_w4(const float* W, void* packed, void* stream, unsigned* hdr, int* bad, int N, int K, int npad, int raw_lo, int raw_hi, hipStream_t s);
// the batch <= 2 GEMV has an int4 form for these arguments (a.W4 set, bf16, LDS-staged activations, K % 128 == 0); the 3-16-row kernels' int4 forms
// are xstat16_w4_supported / xrow16_w4_supported below
bool skinny_w4_supported(int dtype, const GemmArgs& a, int epi);

// coded bf16 weights: 128 k-values per chunk; per (tile, chunk) three planes of whole-wave contiguous loads (rdx_common.h)
constexpr int WC_CHUNK_K = 128, WC_CHUNK_BYTES = 64 * 52;
inline size_t wc_bytes(int npad, int k) { return (size_t)(npad / 16) * (size_t)(k / WC_CHUNK_K) * WC_CHUNK_BYTES; }
// bf16 only: reads the PACKED buffer of launch_pack_weight, writes the planes, hdr[npad / 16] = base | raw << 8 and, behind them, the dense words
// hdr[npad / 16 + tile] (hdr holds wc_hdr_words(npad) words); K % 128 == 0
inline size_t wc_hdr_words(int npad) { return (size_t)(npad / 16) * 2; }
void launch_encode_wc(const void* packed, void* planes, unsigned* hdr, int npad, int K, hipStream_t s);
// the batch <= 2 GEMV has a coded form for these arguments (a.WC set, bf16, LDS-staged activations, K % 128 == 0)
bool skinny_wc_supported(int dtype, const GemmArgs& a, int epi);

struct ConvGeom {        // mode 0: plain row-major A.  mode 1: im2col gather from NHWC, K ordered (kh, kw, c)
    int mode;
    int Hin, Win, Cin, Hout, Wout, KH, KW, stride, pad;
};

// fragment-packed convolution / GEMM (pconv.hip): X, resid and out are packed activation tensors [C / 32][mtiles][64 lanes][8]
// (m = NHWC pixel index), W the usual fragment-packed weight with K ordered (kh, kw, c)
struct PConvArgs {
    const void* X; const void* W; const float* bias; const void* resid; void* out;
    const void* zero16;              // >= 16 zero bytes: what taps in the padding read
    int Hin, Win, Cin, Hout, Wout, N;
    int M;                           // output pixels = B x Hout x Wout
    int mt_in, mt_out;               // 16-row tiles of the packed input / output tensors
    int ldo;                         // row stride (elements) when the output is written row-major
    int clog;                        // log2(Cin / 32), filled by launch_pconv
    int no_ksplit;                   // experiments: never let a workgroup's waves split K (the switch "pconv_ksplit" off)
    int tile_m, tile_n, tile_k;      // experiments: forced register tile (MTW x NTW, K split over tile_k waves; 0 = pick; tools/pconv_check.py)
};

struct AttnArgs {        // generic softmax(QK^T/sqrt(D)) V over strided tensors
    const void* Q; const void* K; const void* V; void* O;
    long q_bs, q_ts, q_hs;           // element strides: batch, token, head
    long k_bs, k_ts, k_hs;
    long v_bs, v_ts, v_hs;
    long o_bs, o_ts, o_hs;
    int B, H, Tq, Tk;
    int causal;                      // query i attends keys j <= i + (Tk - Tq)
    int k_perm;                      // K is a decode KV-cache slab in the 16-position fragment order (rdx_common.h kperm), D = 128
    const uint8_t* key_mask; long km_bs;   // nullable [B][>=Tk], 1 = attend
    int flash_min;                   // causal head_dim-128 prefill: take flash_prefill_k from this many 64-query workgroups (0 = never); rdx_ctx::flash_min
    int o_packed_mt;                 // != 0: O is written fragment-packed for wstat_k, [(h D + d) / 32][o_packed_mt][lane][8], row = b Tq + q
};

// Decode-loop state lives in device memory, per batch row (slot_b[b] = KV slot the next token is written to,
// step_b[b] = tokens generated so far, pos[b] = position id of the next token), so that one captured step graph can
// be replayed with identical kernel arguments.

struct LlamaDims {
    int hidden, heads, head_dim, qkv_ld, lora_r;
    float lora_scale;
    int max_len;         // KV slots per (b, head)
    int max_pos;
    int k_perm;          // K cache slabs in the 16-position fragment order (rdx_common.h kperm) instead of row-major
    int kv_fp8 = 0;      // the context's KV cache holds e4m3 codes + row exponents (radialog_amd/kv8.py): decode attention through launch_decode_attention_kv8,
                         // never inside the fused attention + o_proj launch
};

void launch_pack_weight(int dtype, const float* src, void* dst, int N, int K, int Npad, const int* rowmap, hipStream_t s);
// per-row absmax e4m3 quantisation: dst8 = fp8 bytes in the 64-deep fragment order, scale[Npad]; dst (nullable; test hooks only) = the
// dequantised weights in the model dtype, standard fragment order (K % 64 == 0)
void launch_pack_weight_fp8(int dtype, const float* src, void* dst8, float* scale, void* dst, int N, int K, int Npad, hipStream_t s);
// skinny GEMM. A fused RMSNorm (a.norm_w != null) is only honoured when skinny_fits_lds(M, K); otherwise the caller
// must normalise first (launch_rmsnorm) and pass norm_w = null. Returns the copy the kernel it chose streams: WS_W4 (skinny_gemm_w4_k) or WS_CODED
// (skinny_gemm_wc_k) where the arguments carry that copy and its predicate accepts them, else WS_RAW (the GEMV on W / W8, or xstat32_k).
bool skinny_fits_lds(int M, int K);
WStream launch_skinny_gemm(int dtype, const GemmArgs& a, int epi, hipStream_t s);
bool xstat32_supported(const GemmArgs& a, int epi);
void launch_xstat32(int dtype, const GemmArgs& a, int epi, hipStream_t s);
// K-split activation-stationary GEMM for the 256-tile projections at 16 < M <= 32: fp32 partial slabs [groups][32][N], combined
// (+ residual, rounding) by the following RMSNorm (NormArgs::slab). groups = 0: shape not supported
int xsplit32_groups(const GemmArgs& a);
void launch_xsplit32(int dtype, const GemmArgs& a, float* slab, hipStream_t s);
int xs_min_rows();        // smallest batch on the xstat32 / xsplit32 path (3)
// one prompt's K = 4096 projections in row blocks of 32, the row blocks of a tile walker sharing an XCD's L2 (xstat32_k<.., BLK>): X ACT_TILES32
bool xstat_blk_supported(const GemmArgs& a, int epi);
void launch_xstat_blk(int dtype, const GemmArgs& a, int epi, hipStream_t s);
// batch 3-16 decode (xs16.hip): activation-stationary K = 4096 projection over ONE row tile with the RMSNorm as its prologue (a.norm_w: X is the
// row-major residual stream; otherwise X is ACT_BLK32), and the un-split o_proj / down_proj with the residual
// epilogue (X ACT_BLK32; resid / out row-major)
bool xs16_rows_ok(int M);
bool xstat16_supported(const GemmArgs& a, int epi);
void launch_xstat16(int dtype, const GemmArgs& a, int epi, hipStream_t s);
bool xrow16_supported(const GemmArgs& a);
void launch_xrow16(int dtype, const GemmArgs& a, hipStream_t s);
// ... their int4 forms (bf16; a.W4 / a.w4hdr set, a.W the packed copy of W' that raw-flagged tiles stream): xstat16_w4_k for EPI_NONE / EPI_SILU_MUL,
// xrow16_w4_k for K % 128 == 0. The weight fragments are decoded in registers to exactly the bits of W', in the bf16 kernels' MFMA order: same output bits
bool xstat16_w4_supported(int dtype, const GemmArgs& a, int epi);
void launch_xstat16_w4(const GemmArgs& a, int epi, hipStream_t s);
bool xrow16_w4_supported(int dtype, const GemmArgs& a);
void launch_xrow16_w4(const GemmArgs& a, hipStream_t s);
void launch_tiled_gemm(int dtype, const GemmArgs& a, const ConvGeom& cg, int epi, hipStream_t s);
// LDS-DMA GEMM for plain row-major activations (M > 32, K % 64 == 0); `ws` = fp32 split-K workspace (nullable)
bool gemm_dma_supported(const GemmArgs& a);
void launch_gemm_dma(int dtype, const GemmArgs& a, int epi, float* ws, size_t ws_floats, hipStream_t s);
// the same kernel with the activation operand gathered from an NHWC tensor (3x3 / strided convolutions, Cin % 8 == 0, K % 64 == 0,
// epilogues NONE / RELU); `zero16` = 16 zero bytes in device memory for taps that fall into the padding
bool gemm_dma_conv_supported(const GemmArgs& a, const ConvGeom& cg, int epi);
void launch_gemm_dma_conv(int dtype, const GemmArgs& a, const ConvGeom& cg, int epi, const void* zero16, float* ws, size_t ws_floats,
                          hipStream_t s);

// weight-stationary streaming 1x1 convolution (conv1x1.hip): K <= 256, many rows (the trunk's layer1 / layer2 at batch); cg.mode 0 =
// plain rows, mode 1 with KH = KW = 1 = strided row gather (downsample)
bool conv1x1_stream_supported(const GemmArgs& a, const ConvGeom& cg, int epi);
void launch_conv1x1_stream(int dtype, const GemmArgs& a, const ConvGeom& cg, int epi, hipStream_t s);

// many-row GEMM / implicit-GEMM convolution with the weight slice in an LDS ring and the activation fragments fetched straight into
// registers by the wave that owns the rows (wsgemm.hip): K % 64 == 0; convolutions need Cin % 64 == 0
// weight-stationary GEMM for one prompt's prefill: activations ACT_TILES32 and streamed past register-resident weights (wstat.hip)
bool wstat_supported(const GemmArgs& a, int epi);
void launch_wstat(int dtype, const GemmArgs& a, int epi, hipStream_t s);
// K-split down_proj / o_proj over 33-128 rows (xsplit32_k<.., BLK>): X ACT_TILES32 over a.mtiles row tiles, slabs [groups][16 mtiles][N]
bool xsplit_blk_supported(const GemmArgs& a);
void launch_xsplit_blk(int dtype, const GemmArgs& a, float* slab, hipStream_t s);
// ... and with fp8 weights (fp8 x fp8): every 32-row block keeps the layouts of the 32-row fp8 kernels at a block stride -- xstat: X = ACT_BLK64_E4M3 + xscale[rows];
// xsplit: X = ACT_BLK64, slabs [groups][32 blocks][N], groups = 2 (K = 4096) or 4 (K = 11008)
bool xstat_blk8_supported(const GemmArgs& a, int epi);
void launch_xstat_blk8(int dtype, const GemmArgs& a, int epi, hipStream_t s);
int xsplit_blk8_groups(const GemmArgs& a);
void launch_xsplit_blk8(int dtype, const GemmArgs& a, float* slab, hipStream_t s);
bool wsgemm_supported(const GemmArgs& a, const ConvGeom& cg, int epi);
void launch_wsgemm(int dtype, const GemmArgs& a, const ConvGeom& cg, int epi, const void* zero16, int ws_cfg, hipStream_t s);      // ws_cfg: the context's switch (0 = by shape, 1..5 = tile shapes A..E)

// fragment-packed convolution (pconv.hip): taps 1 | 9 (3 x 3 pad 1), stride 1 | 2, epilogues NONE / RELU / RESID_RELU; rowout = row-major output
bool pconv_supported(const PConvArgs& a, int taps, int stride, int epi);
bool launch_pconv(int dtype, PConvArgs a, int taps, int stride, int epi, bool rowout, hipStream_t s);      // false: refused (1 x 1 stride-1 with mt_in != mt_out), nothing launched
// LayerNorm / broadcast on packed tensors (the Q-Former on packed activations)
bool layernorm_packed_supported(int H);
void launch_layernorm_packed(int dtype, const void* x, const float* gamma, const float* beta, void* out, float* out_f32, int M, int H, float eps, hipStream_t s);
void launch_broadcast_packed(int dtype, const void* src, void* dst, int rows, int H, int B, hipStream_t s);
void launch_pack_rows(int dtype, const void* X, int ldx, void* P, int M, int C, hipStream_t s);      // row-major [M][C] -> packed
void launch_unpack_rows(int dtype, const void* P, void* X, int ldx, int M, int C, hipStream_t s);

// fused ResNet stem (stem.hip): 7x7/2 conv + bias + ReLU + 3x3/2 max pool from the padded NHWC4 image to [B][Ho][Ho][stem]
bool stem_pool_supported(int stem_channels);
// packed_mt != 0: the output is written fragment-packed [stem / 32][packed_mt][64][8] (the layout pconv_k reads) instead of NHWC
void launch_stem_pool(int dtype, const void* in, const void* Wp, const float* bias, void* out, int B, int Hp, int Hc, int Ho, int stem,
                      int packed_mt, hipStream_t s);

void launch_l2_bench(int mode, const void* buf, size_t bytes_per_wg, int shared, int reps, int wgs, unsigned* sink, hipStream_t s);

void launch_attention(int dtype, int head_dim, const AttnArgs& a, hipStream_t s);
// 64-query flash-style blocks for head_dim 128 (flash.hip); launch_attention takes it when the grid fills the chip (RDX_FLASH_MIN workgroups)
bool flash_prefill_supported(int head_dim, const AttnArgs& a);
void launch_flash_prefill(int dtype, const AttnArgs& a, hipStream_t s);
// prefill: LoRA add + RoPE + KV-cache write for T tokens of B rows; q -> qout [B*T][hidden]
void launch_rope_kv_prefill(int dtype, const LlamaDims& d, const void* qkv, const void* lora_bq, const void* lora_bv,
                            const void* cos_t, const void* sin_t, const int* pos_ids, void* qout, void* kcache,
                            void* vcache, int B, int T, int slot0, hipStream_t s);     // rows land at cache slots slot0 + t
void launch_k_unperm(const void* kc, void* out, size_t slabs, int max_len, int perm, hipStream_t s);
// decode: LoRA + RoPE + KV append + attention over the cache for one new token per row
struct DecAttnArgs {
    LlamaDims d;
    const void *qkv, *lbq, *lbv, *cos_t, *sin_t;
    const void* cur_rope = nullptr;  // optional [B][2][128]: cos | sin row of each batch row's CURRENT position (else pos -> tables)
    const int *pos, *slot_b;
    const uint8_t* key_mask;
    void *kcache, *vcache, *out;
    long long* trace = nullptr;      // debug: 8 timestamps (100 MHz ticks) of workgroup (b=0,h=0); the fused launch: [workgroup][8] (attn_body.h, chain.hip)
    ActLayout out_packed = ACT_ROWS; // stand-alone launches, from 3 rows: the order `out` is written in for the projection behind it (ACT_BLK32 / ACT_BLK64 / ACT_TILES32)
    int out_mt = 2;                  // ACT_TILES32: its row tiles
    // the fused attention + o_proj launch only: `out` is the tagged-granule buffer (handoff.h), tag = handoff_tag(*epoch, layers, layer)
    const int* epoch = nullptr;
    int layers = 0, layer = 0;
};
// host only, beside the arguments: the context's switches "att_tp" (1 forces the 4-wave throughput build, 2 the 8-wave one) and "att_mid" (api_options.hip)
struct DecAttnSw { int att_tp = 0, att_mid = 1; };
void launch_decode_attention(int dtype, const DecAttnArgs& a, int B, DecAttnSw sw, hipStream_t s);
// fp8 KV cache (the format: radialog_amd/kv8.py; device side: rdx_common.h "kv8"). a.kcache / a.vcache are the code slabs [B][heads][max_len][128] bytes (K in
// the kperm8 order, V row-major; a.d.k_perm is not looked at), kexp / vexp the row exponents [B][heads][max_len]. Same variants and output bits as
// launch_decode_attention on a T cache holding the stored values.
void launch_decode_attention_kv8(int dtype, const DecAttnArgs& a, signed char* kexp, signed char* vexp, int B, DecAttnSw sw, hipStream_t s);
// staged T rows [slabs][stage_len][128] (row-major K and V) -> codes and exponents of cache positions [slot0, slot0 + T) of every slab
void launch_kv8_quant_rows(int dtype, const void* kstage, const void* vstage, int stage_len, void* kcodes, signed char* kexp, void* vcodes, signed char* vexp,
                           size_t slabs, int max_len, int T, int slot0, hipStream_t s);
// code slabs (is_k: the kperm8 order) -> the codes in logical order (codes_out, nullable) and the stored values in T (t_out, nullable), [slabs][max_len][128]
void launch_kv8_read(int dtype, const void* codes, const signed char* exps, int is_k, size_t slabs, int max_len, void* codes_out, void* t_out, hipStream_t s);
// Chained decode launches of the batch <= 2 step (chain.hip): units run as roles of one launch, chained by a fence-free counter
// hand-off (handoff.h) instead of a kernel boundary.
// Every launch is a graph node of ONE layer, so the layer's pointers travel by value (no device table, no dependent read in front of the weight
// stream). The launcher hands the kernel the fields its weight rings are addressed from (wdown / wqkv or their fp8 twins, hidden, inter, qkv_n, the
// down_proj workgroup count) as LEADING scalar arguments in front of the struct: the units of the batch-1/2 step are compiled with kernarg
// preloading (build.py UNIT_FLAGS), which has the command processor place leading non-aggregate arguments in SGPRs before the first wave starts.
struct ChainArgs {
    const void *wdown, *wqkv;        // down_proj of `layer`; QKV of `layer + 1` (unused by the last layer's launch)
    const void *wdown8, *wqkv8;      // fp8 weights (e4m3, 64-deep fragment order), null when the model dtype copy is streamed
    const float *sdown, *sqkv;       // their per-row scales
    const void* attn_norm;           // RMSNorm weight in front of QKV(layer + 1)
    int layer;                       // down_proj of this layer, QKV of the next (selects the hand-off counters)
    int hidden, inter, qkv_n, qkv_ld, B;
    int w8;                          // stream the fp8 weights (every projection quantised)
    // coded bf16 weights (bf16, K % 128 == 0 for both roles): the planes of down_proj(layer) / QKV(layer + 1) and their header words; wdown / wqkv stay
    // the raw packed copies, which the tiles flagged in the headers stream. wc = 0: decode_chain_k on the raw copies.
    // wc = 2: cdown / cqkv are the int4 streams (rdx_common.h W4Chunk) and wdown / wqkv the packed copies of the dequantised weights: decode_chain_w4_k.
    const void *cdown, *cqkv; const unsigned *hdown, *hqkv; int wc;
    float eps;
    void *dx, *dqkv, *dgu;           // [B][hidden] residual stream, [B][qkv_ld], [B][inter]
    int* ctr;                        // chain_ctr_ints(layers) ints, zero at the start of every step
    int* err;
    int naps;                        // poll back-off (x s_sleep(8) between polls)
    long long* trace;                // debug: [workgroup][8] timestamps (100 MHz ticks) of one launch, slots in chain.hip; null in every product launch
};
bool chain_supported(const LlamaDims& d, int inter, int B);
size_t chain_ctr_ints(int layers);
// down_proj(l) (+ residual) -> RMSNorm + QKV(l + 1) in ONE launch, one workgroup per CU; with_next_qkv = false for the last layer
void launch_decode_chain(int dtype, ChainArgs ca, bool with_next_qkv, hipStream_t s);
// decode attention + o_proj (+ residual) in ONE launch of 16-wave workgroups: fast attention body, two o_proj tiles per workgroup with
// their whole K slice in registers, data-tagged hand-off (handoff.h): a.out = g.X = the granule buffer ([2][hidden] x 4 bytes, one for the whole
// model, never zeroed after creation), `hint` = HO_HINT_INTS words behind it; `err` is set to 1 if a wait ever times out (never hangs).
constexpr int HO_HINT_INTS = 128;
bool attn_oproj16_supported(const LlamaDims& d, int N, int K, int B);
void launch_attn_oproj16(int dtype, const DecAttnArgs& a, const GemmArgs& g, int B, int* hint, int* err, hipStream_t s);

// LlamaRMSNorm of `rows` rows into any ActLayout (elem.hip). w null: re-layout only. slab: the fp32 partials [groups][slab rows][H] a K-split projection
// left pending -- x[row] += T(sum over the groups, in order) first, written back to x; slab rows = the rows the layout holds (32 for ACT_ROWS, <= 32 rows).
struct NormArgs {
    void* x; const void* w;          // [rows][H]; weight [H] or null
    void* out; float* xscale;        // the layout's buffer; the e4m3 layouts' scales [rows the layout holds]
    int rows, H; float eps;
    ActLayout layout; int mtiles;    // row tiles of 16 (ACT_TILES32; ACT_BLK64_E4M3: ceil(mtiles / 2) blocks, 0 = one). The one-block orders hold 32 rows
    const float* slab; int groups;
};
bool rmsnorm_supported(const NormArgs& n);
bool launch_rmsnorm(int dtype, const NormArgs& n, hipStream_t s);      // false: no kernel for this combination (rmsnorm_supported), nothing launched
// fp8 path (BASELINE configs[4]): e4m3 activations with absmax / 448 scales -- see gemm8.hip for the scheme
void launch_quant_rows(int dtype, const void* x, long ldx, void* out8, float* xscale, int rows, int K, int groups, hipStream_t s);
// fp8 x fp8 MFMA GEMM over row-major e4m3 activations (any M; N % 16 == 0, K % 64 == 0): epilogues NONE / RESID / SILU_MUL
bool gemm8_supported(const GemmArgs& a, int epi);
void launch_gemm8(int dtype, const GemmArgs& a, int epi, hipStream_t s);
void launch_layernorm(int dtype, const void* x, const float* gamma, const float* beta, void* out, float* out_f32,
                      int rows, int H, float eps, hipStream_t s);
void launch_layernorm_ex(int dtype, const void* x, long ldx, const float* gamma, const float* beta, const void* emb, int emb_rows,
                         void* out, long ldo, int rows, int H, float eps, hipStream_t s);
void launch_pool_gather(int dtype, const void* src, void* dst, int B, int L, int C, hipStream_t s);
void launch_pool_concat(int dtype, const void* patch, const void* tokens, void* dst, int B, int L, int C, hipStream_t s);
void launch_scramble_layernorm(int dtype, const void* pp_nhwc, const float* gamma, const float* beta, void* out,
                               float* out_f32, int B, int P, int C, float eps, hipStream_t s);
void launch_img_prep(int dtype, const float* img, void* out, int B, int S, int pad, int Hp, int Wp, hipStream_t s);
void launch_maxpool(int dtype, const void* in, void* out, int B, int H, int W, int C, hipStream_t s);
void launch_broadcast_rows(int dtype, const void* src, void* dst, int rows, int H, int B, hipStream_t s);
void launch_avgpool_flatten(int dtype, const void* in, void* out, int B, int G, int C, int pool, hipStream_t s);
void launch_to_f32(int dtype, const void* src, float* dst, size_t n, hipStream_t s);
void launch_from_f32(int dtype, const float* src, void* dst, size_t n, hipStream_t s);

void launch_prep_prompt(const int* ids, const int* mask_in, int B, int T, int img_id, int pad_id, int* img_pos,
                        int* pos_ids, uint8_t* key_mask, long km_bs, int* pos_next, int* slot_b, int* step_b,
                        int* unfinished, hipStream_t s);
void launch_prep_append(int B, int T_, int keep_len, int* img_pos, int* pos_ids, int* pos_next, int* slot_b, int* step_b,
                        int* unfinished, hipStream_t s);
void launch_embed_splice(int dtype, const int* ids, const int* img_pos, const void* embed, int vocab, const void* img_emb,
                         int n_img, void* out, int B, int T, int H, int use_img, hipStream_t s);
void launch_gather_last(int dtype, const void* x, void* out, int B, int T, int H, hipStream_t s);
// What follows the selection of a row's token, for both greedy kernels (elem.hip: step_tail). pos / slot_b null: not advanced (the prefill call).
// pos_ro / cos_t / sin_t / cur_rope: after the update, copy the cos | sin table row of each row's position into cur_rope [B][2][128] (pos_ro = the
// position array even when `pos` is null). ctr_zero / n_zero: hand-off counter words to clear for the next decode step (nullable).
// epoch (nullable): the step counter the tagged hand-off derives its tags from (handoff.h), incremented by thread 0 of block 0.
// hist / hist_len / hist_ld: the token history [B][hist_ld] and its lengths, read and appended to by select_step_k only (greedy_step_k: null).
struct StepTail {
    int eos_id, pad_id, max_new, vocab, H, n_zero, hist_ld;
    int *out_tokens, *unfinished, *pos, *slot_b, *step_b, *ctr_zero, *hist, *hist_len, *epoch;
    const int* pos_ro;
    const void *embed, *cos_t, *sin_t;
    void *x_next, *cur_rope;
};
void launch_greedy_step(int dtype, const float* part_val, const int* part_idx, int n_tiles, int B, const StepTail& t, hipStream_t s);
// Greedy step under logits rules (select_step_k): repetition penalty, n-gram ban and min-new-tokens on row b of `logits` (model dtype, row-major
// [B][vocab] at logits + n_gen[b] * step_stride elements), in place, then the argmax and the tail of launch_greedy_step.
struct SelectArgs {
    void* logits; long step_stride;
    const int* n_gen;                      // [B] tokens generated so far (the step's d_step; also the score row of a captured step)
    float penalty; int ngram, min_new;
    int* sel_out;                          // kernel-test hook: [B] selected tokens; the tail (state advance, history append) does not run
};
inline size_t select_step_lds(int vocab) { return (size_t)2 * ((vocab + 31) / 32) * sizeof(unsigned); }     // two bitmaps over the vocabulary
bool select_step_supported(int vocab);
void launch_select_step(int dtype, const SelectArgs& a, const StepTail& t, int B, hipStream_t s);       // t.hist* = the rows' history
// Sampled step (sample_step_k): the rules of SelectArgs (neutral = none; t.hist may then be null), then temperature, top-k, top-p and the draw of
// include/rdx.h (rdx_sampling) on the same row, in place, then the tail. `seed` is a device word: a new seed needs no new graph.
struct SampleArgs {
    float temperature; int top_k; float top_p;
    const unsigned long long* seed;
};
// dynamic LDS of sample_step_k: two bitmaps | masses u64[256] | scan u64[2][256] | counts int[256] | 16 words | the row (+ 8 elements of alignment slack)
inline size_t sample_step_lds(int vocab) {
    return (((size_t)2 * ((vocab + 31) / 32) * sizeof(unsigned) + 15) & ~(size_t)15) + 256 * 8 + 512 * 8 + 256 * 4 + 64 + ((((size_t)vocab + 8) * 2 + 15) & ~(size_t)15);
}
bool sample_step_supported(int vocab);
void launch_sample_step(int dtype, const SelectArgs& a, const SampleArgs& sp, const StepTail& t, int B, hipStream_t s);
void launch_hist_init(const int* ids, int B, int T, int* hist, int* hist_len, int ld, hipStream_t s);
void launch_hist_set_last(const int* ids, int* hist, const int* hist_len, int ld, int B, hipStream_t s);

// Prompt-lookup decoding (lookup.hip; the rules: include/rdx.h rdx_generate_lookup). lookup_accept_k: ONE workgroup, one sequence, behind the lm_head of a
// forward over d + 1 rows [last emitted token, draft_1 .. draft_d] (d == 0: the plain step, or the prompt's token-0 call with t.pos / t.slot_b null). It reduces
// the rows' argmax partials, accepts the longest draft prefix the model agrees with, emits a + 1 tokens through the EOS / pad rule (out_tokens, the history,
// `scores` rows from the pass's `logits`), advances the decode state of row 0 as a + 1 plain steps would have (step_tail's fields of t; t.hist is required),
// finds the next draft and leaves the next forward's inputs: tail ids, their position ids, and the status words the host reads.
constexpr int LOOKUP_MAX_DRAFT = 15, LOOKUP_MAX_NGRAM = 8;
// par (device, int[5]): the call's constants
enum { LKP_NCORPUS = 0, LKP_DRAFT_LEN = 1, LKP_NGRAM_MAX = 2, LKP_NGRAM_MIN = 3, LKP_SLOT_END = 4, LKP_INTS = 5 };
// status (device, int[4]): what the host copies after every forward ([0], [1]: 8 bytes) and what the kernel keeps for itself
enum { LKS_NEXT = 0 /* next d | finished << 8 */, LKS_SLOT = 1 /* cache slot of the next forward's first row */, LKS_FWD = 2 /* forwards so far */, LKS_INTS = 4 };
struct LookupArgs {
    const float* part_val; const int* part_idx; int n_tiles;     // [d + 1][n_tiles]
    int d;                                  // drafts this forward verified; they are tail[1 .. d]
    const void* logits; void* scores;       // the pass's rows [d + 1][vocab] -> scores[step + j][vocab] (both nullable; d == 0: the lm_head wrote the row in place)
    int* tail;                              // [LOOKUP_MAX_DRAFT + 1]: this forward's input ids in, the next forward's out
    const int* slot;                        // row 0's cache slot (t.slot_b where the forward advances it; the token-0 call only reads it)
    int* pos_ids; int* img_pos;             // the next pass's position ids [d' + 1] and its (unused) image position
    int* status; int* trace; int trace_cap; // trace [trace_cap][2] = (drafted, accepted) of forward status[LKS_FWD] (nullable; the token-0 call records nothing)
    const int* par; const int* corpus;      // corpus [par[LKP_NCORPUS]]
};
void launch_lookup_accept(int dtype, const LookupArgs& a, const StepTail& t, hipStream_t s);

// Scoring given tokens (score.hip). score_rows_k: one workgroup per row of logits [M][ld] (model dtype; ld % 8 == 0, base 16-byte aligned), over columns
// 0 .. vocab - 1 only: logprob[r] = (x_target - max) - log(sum exp(x - max)) in fp32, top1[r] = argmax (lowest index on ties); target -100: (0.0f, -1).
inline size_t score_rows_lds(int vocab) { return (size_t)((vocab + 7) / 8) * 16; }      // dynamic LDS: the row
bool score_rows_supported(int vocab, long ld);
void launch_score_rows(int dtype, const void* logits, long ld, const int* target, int vocab, float* logprob, int* top1, int M, hipStream_t s);
void launch_gather_rows(int dtype, const void* x, const int* rows, void* out, int n, int H, hipStream_t s);       // out[i] = x[rows[i]], rows of H elements (H % 8 == 0)
void launch_score_scatter(const float* lp, const int* t1, const int* dst, float* logprob, int* top1, int n, hipStream_t s);   // logprob[dst[i]] = lp[i] (top1 likewise, nullable); dst < 0: skipped
void launch_logits_out(int dtype, const void* ws, long ld, const int* dst, void* out, int vocab, int n, hipStream_t s);       // out[dst[i]][0 .. vocab) = ws[i][0 .. vocab)

// Generation log-probs (logprob.hip). logprob_step_k: one workgroup per batch row behind the step's selection launch. Row b describes step = d_step[b] - 1 (the
// tail has advanced it): the scores row at logits + step * step_stride + b * row_stride elements (model dtype, columns 0 .. vocab - 1) and the token
// tokens[b * max_new + step]. chosen [B][out_ld] float, top_ids / top_lp [B][out_ld][8]: entry [b][step] gets the token's log-prob and the top_n (0 .. 8)
// largest columns (descending, lowest index on ties) with theirs; a step outside [0, max_new) writes nothing (out_ld >= max_new).
struct LogprobArgs {
    const void* logits; long row_stride, step_stride;
    const int* d_step; const int* tokens;
    int B, max_new, vocab, top_n;
    float* chosen; int* top_ids; float* top_lp; long out_ld;
};
inline size_t logprob_step_lds(int vocab) { return (size_t)((vocab + 7) / 8) * 16; }      // dynamic LDS: the row in whole 8-element groups
bool logprob_step_supported(int vocab);
void launch_logprob_step(int dtype, const LogprobArgs& a, hipStream_t s);

// beam search (beam.hip)
#define RDX_MAX_BEAMS 8
void launch_beam_topk(int dtype, const void* logits, const float* beam_scores, int groups, int beams, int vocab, float* cand_score,
                      int* cand_idx, void* logp_out, hipStream_t s);
void launch_kv_beam_reorder(void* kcache, void* vcache, void* scratch, const int* src, const int* start, int rows, int heads, int layers, int max_len,
                            size_t layer_bytes, int p0, int p1, hipStream_t s);
void launch_embed_rows(int dtype, const int* tokens, const void* embed, int vocab, void* x, int rows, int H, hipStream_t s);

// ---- row sessions (rows.hip): staged rows into live rows, parked rows ----
constexpr int ROWLIST_MAX = 128;        // = RDX_MAX_ROWS: a list rides in the kernel arguments, no device copy of host indices
struct RowList { int n; short src[ROWLIST_MAX], dst[ROWLIST_MAX]; };      // absolute row indices; src unused when parking
// the per-row decode state row_state_move_k moves: [rows] ints, the key mask [rows][max_len], dx [rows][H] and cur_rope [rows][256] (2-byte elements),
// out_tokens [live rows][cap]; stage_tokens [staging rows][cap] holds token 0 of staged row r at row r - row0
struct RowState {
    int *pos, *slot, *step, *unf;
    uint8_t* key_mask; void* dx; void* cur_rope;
    int32_t* out_tokens; const int32_t* stage_tokens;
    int max_len, H, cap, pad_id, row0;
};
// positions [0, npos) (a multiple of 16, or max_len) of every layer's K and V: row src[i] -> row dst[i]; the two sets of rows are disjoint
void launch_kv_rows_move(void* kcache, void* vcache, const RowList& rl, int heads, int layers, int max_len, size_t layer_bytes, int npos, hipStream_t s);
// park == 0: state of row src[i] -> row dst[i], out_tokens row cleared, token 0 in column 0. park != 0: rows dst[i] parked (bit 1: out_tokens row cleared too)
void launch_row_state_move(const RowState& st, const RowList& rl, int park, hipStream_t s);

}  // namespace rdx
