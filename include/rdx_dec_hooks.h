/* rdx_dec_hooks.h -- the decoder's 3-16-row (xs16.hip) and row-block (xstat32.hip, BLK) GEMM kernels, its RMSNorm, decode attention and the prompt's RoPE / KV
 * write one launch at a time on caller data (tests/test_gpu_decoder_gemms.py, test_gpu_rmsnorm.py, test_gpu_decode_attn.py). Like the hooks of rdx_hooks.h they live in radialog_amd/librdx_hooks.so (radialog_amd/csrc/api_dec_hooks.hip,
 * linked against librdx.so), never in the product library, and radialog_amd/_lib.py binds them (DEC_HOOK_SYMBOLS) only under RDX_DEBUG_HOOKS=1.
 * Each hook packs the fp32 weight W [N][K] with the production packer, allocates its own temporaries, asks the production *_supported predicate
 * (an unsupported shape is an error and launches nothing) and calls the production launch_* functions unchanged. All tensors are device pointers
 * in the model dtype unless said otherwise; argmax_host is host memory. Epilogues: 0 none, 3 residual, 4 SwiGLU (W's 16-row tiles hold 8 gate rows
 * then the 8 matching up rows; N / 2 output columns), 5 logits. Fragment-packed blocks are returned RAW:
 *   [k / 32][row tiles][lane = 16 ((k % 32) / 8) + row % 16][8]. */
#ifndef RDX_DEC_HOOKS_H
#define RDX_DEC_HOOKS_H
#include "rdx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* launch_xstat16: X [M][4096] row-major, norm_w [4096] (the RMSNorm is the kernel's prologue), 3 <= M <= 16, N >= 8192. epi 0 / 5: out [M][ldo];
 * epi 4, out_packed 0: out [M][ldo] (N / 2 columns); out_packed 1: out = the packed block [N / 64][2 row tiles][64][8] of which the kernel writes
 * row tile 0 (N % 64 == 0, ldo unused). epi 5: logits for n < n_valid and argmax_host[M] = the per-tile partials reduced on the host, lowest index on ties. */
int rdx_xstat16_test(rdx_ctx* ctx, const void* X, const void* norm_w, float eps, const float* W, int M, int N, int epi, int n_valid, void* out,
                     int ldo, int out_packed, int32_t* argmax_host);

/* launch_xrow16: out [M][ldo] = resid [M][N] + T(X W^T), K % 32 == 0, K >= 512, N % 16 == 0. x_packed 0: X [M][K] row-major, re-laid into the packed
 * 32-row block by launch_rmsnorm without a norm weight; x_packed 1: X already is that block [K / 32][2][64][8] (rdx_xstat16_test's
 * out_packed 1 output: the production gate/up -> down_proj seam). */
int rdx_xrow16_test(rdx_ctx* ctx, const void* X, int x_packed, const float* W, const void* resid, int M, int N, int K, void* out, int ldo);

/* launch_rmsnorm into the row tiles (norm_w nullable: re-layout only) + launch_xstat_blk: X [M][4096], M <= 192, N >= 2048. epi 0 / 3 / 5: out [M][ldo]
 * (3: resid [M][N]); epi 4, out_packed 0: out [M][ldo]; out_packed 3: out = the packed block [N / 64][mtiles][64][8] (N % 64 == 0), mtiles =
 * ceil(M / 16). xp_out (nullable): the norm's packed output [128][mtiles][64][8]. */
int rdx_xstat_blk_test(rdx_ctx* ctx, const void* X, const void* norm_w, float eps, const float* W, const void* resid, int M, int N, int epi,
                       int n_valid, void* out, int ldo, int out_packed, void* xp_out, int32_t* argmax_host);

/* launch_rmsnorm (re-layout of X [M][11008]) + launch_xsplit_blk [+ launch_rmsnorm with the slabs]. slab_out (nullable) fp32 [4][16 mtiles][N]:
 * the K groups' partial sums. With x_resid: N == 4096, x_resid [M][4096] += T(sum of the slabs) in place, and xn_out = the packed RMSNorm
 * (norm_w [4096]) of the updated rows, [128][mtiles][64][8]. x_resid, norm_w and xn_out go together. */
int rdx_xsplit_blk_test(rdx_ctx* ctx, const void* X, const float* W, void* x_resid, const void* norm_w, float eps, int M, int N, float* slab_out,
                        void* xn_out);

/* fp8: launch_rmsnorm into e4m3 blocks (norm_w [4096] required) + launch_xstat_blk8 on e4m3 weights packed here: X [M][4096], 33 <= M <= 128. epi 0 / 5: out
 * [M][ldo]; epi 4: out [M][ldo], or out_packed 2: NB = ceil(M / 32) packed 32-row blocks in the 64-deep order, 32 (N / 2) elements each (N % 128 == 0).
 * x8_out (nullable) NB x 32 x 4096 e4m3 bytes and xscale_out (nullable) fp32 [32 NB]: what the norm wrote. */
int rdx_xstat_blk8_test(rdx_ctx* ctx, const void* X, const void* norm_w, float eps, const float* W, int M, int N, int epi, int n_valid, void* out,
                        int ldo, int out_packed, void* x8_out, float* xscale_out, int32_t* argmax_host);

/* fp8: launch_rmsnorm (64-deep order, no weight: re-layout of every 32-row block of X [M][K]) + launch_xsplit_blk8 [+ launch_rmsnorm into e4m3 blocks
 * with the slabs], K 4096 (2 groups) or 11008 (4). slab_out (nullable) fp32 [groups][32 NB][N]. With x_resid (N == 4096): updated in place, and x8_out /
 * xscale_out = the e4m3 blocks and scales of its RMSNorm. x_resid, norm_w, x8_out and xscale_out go together. */
int rdx_xsplit_blk8_test(rdx_ctx* ctx, const void* X, const float* W, void* x_resid, const void* norm_w, float eps, int M, int N, int K,
                         float* slab_out, void* x8_out, float* xscale_out);

/* launch_rmsnorm alone (elem.hip): x [rows][H], norm_w [H] or null (re-layout only), layout 0-5 = the activation orders of ActLayout (csrc/rdx_kernels.h: 0
 * row-major, 1 the 32-row block, 2 its 64-deep order, 3 mtiles row tiles, 4 e4m3 blocks in the 64-deep order + xscale, 5 e4m3 row-major + xscale). slab
 * (nullable) fp32 [groups][rows the layout holds][H]: x += T(sum of the slabs) in place first. out (out_bytes) and xscale (nullable, xscale_n floats) are
 * filled with 0xff bytes, then written by the norm. A combination without a kernel is an error and launches nothing. */
int rdx_rmsnorm_test(rdx_ctx* ctx, void* x, const void* norm_w, float eps, int rows, int H, int layout, int mtiles, const float* slab, int groups, void* out,
                     long long out_bytes, float* xscale, int xscale_n);

/* select_step_k alone (elem.hip: the greedy step under logits rules): its penalty, ban and argmax part on caller data, without the decode-state tail.
 * logits_inout [B][vocab] row-major model dtype (vocab may be odd: the rows then start at odd elements), processed in place; hist int32 [B][ld],
 * hist_len [B] (0 .. ld), n_generated [B] (what min_new_tokens compares with), all device; tokens_out int32 [B] device: the argmax of each processed
 * row, lowest index on ties. Works on any context (no weights involved). */
int rdx_select_test(rdx_ctx* ctx, void* logits_inout, int B, int vocab, const int32_t* hist, const int32_t* hist_len, const int32_t* n_generated, int ld,
                    const rdx_logits_rules* rules, int eos_id, int32_t* tokens_out);

/* lookup_accept_k alone (lookup.hip: what follows the lm_head of a forward of rdx_generate_lookup, see include/rdx.h) on caller data, all device pointers
 * unless said otherwise. part_val / part_idx [d + 1][n_tiles]: the rows' argmax partials; tail int32[16]: [last token, draft_1 .. draft_d] in, the next
 * forward's ids out; corpus int32[n_corpus] (nullable); draft_len (0: never draft) / ngram_max / ngram_min / slot_end: the call's constants; hist int32[hist_ld]:
 * the history, appended to; state int32[5] = {step, slot, position, unfinished, history length}, advanced in place (advance == 0: the token-0 form, which
 * leaves slot and position alone and records no forward); out_tokens int32[max_new]; logits [d + 1][vocab] / scores [max_new][vocab] model dtype, nullable;
 * status int32[4] (word 2, the forward count, is read: zero it first); trace int32[trace_cap][2] nullable; pos_ids int32[16]. vocab, the embedding and the
 * RoPE tables are those of the (finalized) context, and the kernel writes the context's own next-input row and cos | sin row: run a new prefill before
 * decoding on that context again. Refused before the launch: sizes out of range, a state that would leave the caller's arrays or the RoPE tables. */
int rdx_lookup_accept_test(rdx_ctx* ctx, const float* part_val, const int32_t* part_idx, int n_tiles, int d, int32_t* tail, const int32_t* corpus, int n_corpus,
                           int draft_len, int ngram_max, int ngram_min, int slot_end, int32_t* hist, int hist_ld, int32_t* state, int advance, int eos_id,
                           int pad_id, int max_new, int32_t* out_tokens, const void* logits, void* scores, int32_t* status, int32_t* trace, int trace_cap,
                           int32_t* pos_ids);

/* score_rows_k alone (score.hip: the kernel of the scoring pass, see include/rdx.h): logits [M][ld] model dtype (device, 16-byte aligned; ld a multiple of 8,
 * >= vocab: columns vocab .. ld - 1 are pad columns that must not be looked at), target int32 [M] (device; -100 = row not scored), logprob_out float [M],
 * top1_out int32 [M] (device). Works on any context (no weights involved). */
int rdx_score_rows_test(rdx_ctx* ctx, const void* logits, int M, int vocab, int ld, const int32_t* target, float* logprob_out, int32_t* top1_out);

/* logprob_step_k alone (logprob.hip: the generation log-probs of include/rdx.h) on caller data, all device pointers. Row b (b < B) describes step =
 * d_step[b] - 1: its scores row lies at logits + step * step_stride + b * row_stride ELEMENTS (model dtype; any 2-byte alignment: rows may start at odd
 * elements; columns >= vocab are not looked at), its token is tokens[b * max_new + step]. chosen_out float [B][out_ld], top_ids_out int32 and top_lp_out
 * float [B][out_ld][8] (out_ld >= max_new): entry [b][step] is written (of the top arrays the first top_n slots), nothing else is; a row whose step is outside
 * [0, max_new) writes nothing. Works on any context (no weights involved). */
int rdx_logprob_step_test(rdx_ctx* ctx, const void* logits, long long row_stride, long long step_stride, const int32_t* d_step, const int32_t* tokens, int B,
                          int vocab, int max_new, int top_n, float* chosen_out, int32_t* top_ids_out, float* top_lp_out, int out_ld);

/* launch_decode_attention alone (attn.hip, attn_body.h: one new token per row -- LoRA-B add, rotate-half RoPE, in-place KV append, attention over the cache), on
 * caller data: hidden = 128 heads, qkv_ld = 3 hidden + 2 lora_r rounded up to 16. qkv [B][qkv_ld] (q | k | v | LoRA-A of q [8] | of v [8]), lbq / lbv [hidden][8]
 * (lora_r 8; else ignored), EITHER cur_rope [B][2][128] (cos | sin row of each row's position) OR cos_t / sin_t [max_pos][128] with pos [B]; slot [B] (the
 * cache slot the new token is written to = the number of cached positions), key_mask [B][max_len] bytes, kcache / vcache [B][heads][max_len][128] (K in the
 * order k_perm names, rdx_common.h kperm), updated in place. out (out_bytes) is filled with 0xff bytes, then written in the order out_packed names (ActLayout 0-3;
 * out_mt: the row tiles of ACT_TILES32). The variant (16, 8 or 4 waves) is the launcher's choice: heads x B, or RDX_ATT_TP. Refused before anything is
 * written: max_len not a multiple of 32 in (0, 1536], lora_r not 0 or 8, a slot outside [1, max_len - 1], a zero mask byte at a row's own slot, a position
 * outside the tables, an out_packed whose layout does not hold B rows (or out_bytes below its extent). */
int rdx_decode_attn_test(rdx_ctx* ctx, int heads, int B, int max_len, int k_perm, int lora_r, float lora_scale, const void* qkv, const void* lbq, const void* lbv,
                         const void* cur_rope, const void* cos_t, const void* sin_t, int max_pos, const int32_t* pos, const int32_t* slot,
                         const uint8_t* key_mask, void* kcache, void* vcache, void* out, long long out_bytes, int out_packed, int out_mt);

/* launch_decode_attention_kv8 alone (the same three builds on the fp8 KV cache; the format: radialog_amd/kv8.py): rdx_decode_attn_test's arguments, with the
 * caches as kcodes / vcodes [B][heads][max_len][128] e4m3 bytes (K in the kernels' storage order, kv8.k_store; V row-major) and kexp / vexp [B][heads][max_len]
 * int8 row exponents, all updated in place: the new token's code rows and exponents at each row's slot. The output bits are those of rdx_decode_attn_test
 * on model-dtype caches holding the stored values. Same refusals. */
int rdx_decode_attn_kv8_test(rdx_ctx* ctx, int heads, int B, int max_len, int lora_r, float lora_scale, const void* qkv, const void* lbq, const void* lbv,
                             const void* cur_rope, const void* cos_t, const void* sin_t, int max_pos, const int32_t* pos, const int32_t* slot,
                             const uint8_t* key_mask, void* kcodes, void* kexp, void* vcodes, void* vexp, void* out, long long out_bytes, int out_packed,
                             int out_mt);
/* launch_kv8_quant_rows alone (attn.hip kv8_quant_rows_k: the prompt's staged rows into the fp8 cache): krows / vrows [B][heads][stage_len][128] model dtype,
 * row-major; rows t < T of every (row, head) go to positions slot0 + t of kcodes / kexp / vcodes / vexp (shapes as above, K in the storage order); every other
 * byte is left alone. Refused: stage_len < T, max_len not a multiple of 16, slots outside the cache. */
int rdx_kv8_quant_test(rdx_ctx* ctx, int heads, int B, int T, int stage_len, int max_len, int slot0, const void* krows, const void* vrows, void* kcodes, void* kexp,
                       void* vcodes, void* vexp);
/* Overwrites one layer's K (which 0) or V (1) cache of a finalized PLAIN context with src [max_batch][heads][max_len][128], model dtype, logical order (K is
 * stored in the order the context keeps it). How a test gives a plain engine the values an fp8-cache engine holds. Refused on a kv_fp8 context. */
int rdx_kv_write_test(rdx_ctx* ctx, int layer, int which, const void* src);

/* launch_rope_kv_prefill alone (attn.hip: the prompt's LoRA-B add, RoPE and KV-cache write), same dims: qkv [B][T][qkv_ld], pos_ids [B][T] (device), cos_t /
 * sin_t [max_pos][128]; token t of row b lands in cache slot slot0 + t; qout [B T][hidden] is filled with 0xff bytes, then written. Refused before anything is
 * written: slot0 < 0, slot0 + T > max_len, a position id outside the tables. */
int rdx_rope_kv_test(rdx_ctx* ctx, int heads, int B, int T, int max_len, int k_perm, int lora_r, float lora_scale, const void* qkv, const void* lbq,
                     const void* lbv, const void* cos_t, const void* sin_t, int max_pos, const int32_t* pos_ids, int slot0, void* kcache, void* vcache,
                     void* qout);

/* sample_step_k alone (elem.hip: the sampled step): rules, warpers and the draw on caller data, without the decode-state tail. Arguments as
 * rdx_select_test; rules NULL or neutral: none (hist / hist_len may then be NULL). n_generated [B] is the draw index of each row as well as what
 * min_new_tokens compares with; the row index of the Philox counter is the row's position in the launch. logits_inout receives the processed rows
 * (kept: scaled value, dropped: -inf), tokens_out the drawn tokens. Works on any context (no weights involved). */
int rdx_sample_test(rdx_ctx* ctx, void* logits_inout, int B, int vocab, const int32_t* hist, const int32_t* hist_len, const int32_t* n_generated, int ld,
                    const rdx_logits_rules* rules, int eos_id, const rdx_sampling* sampling, int32_t* tokens_out);
/* The 24 random bits of (seed, row, draw index) on the host: the same function the kernel calls (csrc/philox.h). No context, no device. */
int rdx_sample_u24_host(uint64_t seed, uint32_t row, uint32_t draw, uint32_t* out);

/* The device encoder of the coded bf16 weights alone (csrc/gemm.hip encode_wc_k; the format: radialog_amd/wcode.py): W fp32 [N][K] (device) is packed
 * as rdx_set_weight packs it (rows padded to whole tiles of 16), then encoded. packed_out: the packed bf16 buffer [Npad / 16][K / 32][64][8]; planes_out:
 * (Npad / 16) (K / 128) 3328 bytes; hdr_out: Npad / 16 words (base | raw << 8). All device pointers. bf16 contexts, K % 128 == 0. */
int rdx_wcode_test(rdx_ctx* ctx, const float* W, int N, int K, void* packed_out, void* planes_out, uint32_t* hdr_out);
/* The coded copies a finalized decoder holds (every gate/up, down_proj and QKV, the lm_head; none in f16 / fp8-weight contexts): out[0] = their 16-row
 * tiles, out[1] = of those, the tiles flagged raw in their header (the kernels read the packed bf16 bytes of these), out[2] = bytes of planes and headers,
 * out[3] / out[4] = launches of skinny_gemm_wc_k / decode_chain_wc_k this context has issued so far (a captured step graph counts once, at capture):
 * how a test sees that the coded kernels, and not their raw twins, ran. out holds 5 values. */
int rdx_wcode_stats(rdx_ctx* ctx, long long* out);
/* The dense words of the device encoder alone: W as for rdx_wcode_test (packed and encoded into temporaries of the hook); dense_host (HOST memory) gets
 * Npad / 16 words, 1 for a tile that is not flagged raw and holds no weight with h = 0 (radialog_amd/wcode.py dense()), 0 otherwise. */
int rdx_wcode_dense_test(rdx_ctx* ctx, const float* W, int N, int K, uint32_t* dense_host);
/* The header and dense words of one coded copy of a finalized decoder: unit 0 = QKV, 2 = gate/up, 3 = down_proj (of `layer`), 4 = lm_head; `tiles` must
 * be the weight's Npad / 16; words_host (HOST memory, may be null) gets 2 tiles words, headers then dense words -- which of the three K loops a tile
 * of that unit runs. dense_total (may be null): the dense tiles over all coded copies of the context. */
int rdx_wcode_dense_words(rdx_ctx* ctx, int unit, int layer, uint32_t* words_host, int tiles, long long* dense_total);

/* The device quantiser of the int4 group-quantised weights alone (csrc/gemm.hip quant_w4_k; the format: radialog_amd/w4.py): W fp32 [N][K] (device) is
 * quantised as rdx_set_weight(RDX_W_GEMM_W4) does it, every tile int4 (rows padded to whole tiles of 16). wprime_out: the packed bf16 buffer of the
 * dequantised weight [Npad / 16][K / 32][64][8]; stream_out: (Npad / 16) (K / 128) 1056 bytes; scales_out: the bf16 scale bits as they stand in the
 * stream, [Npad / 16][K / 128][16 rows]. All device pointers. Returns -8 outside a bf16 context or for K % 128 != 0, -1 for an Inf / NaN weight. */
int rdx_w4_test(rdx_ctx* ctx, const float* W, int N, int K, void* wprime_out, void* stream_out, void* scales_out);
/* The int4 streams a finalized decoder holds (RDX_W_GEMM_W4: every gate/up, down_proj and QKV): out[0] = their int4 16-row tiles, out[1] = their raw
 * tiles (the LoRA-A rows of the fused QKV weights: the kernels stream the packed bf16 bytes of these), out[2] = bytes of streams and headers,
 * out[3] / out[4] = launches of skinny_gemm_w4_k / decode_chain_w4_k this context has issued so far (a captured step graph counts once, at capture).
 * out holds 5 values. */
int rdx_w4_stats(rdx_ctx* ctx, long long* out);
/* ... and the int4 launches of the 3-16-row step (xs16.hip): out[0] = launches of xstat16_w4_k (QKV, gate/up), out[1] = of xrow16_w4_k (down_proj), counted
 * like the two above. out holds 2 values. */
int rdx_w4_rows_stats(rdx_ctx* ctx, long long out[2]);

/* launch_xstat16_w4 (bf16 context): rdx_xstat16_test's arguments for epi 0 / 4, but W fp32 [N][4096] is quantised by the production quantiser as
 * rdx_set_weight(RDX_W_GEMM_W4) does it, and the kernel streams the int4 chunks. The 16-row tiles of rows >= raw_lo (a multiple of 16; >= N: none) stay
 * raw bf16 and stream their packed bytes; raw_lo < 0: only the ONE tile of rows [-raw_lo, -raw_lo + 16) does, a raw tile between int4 tiles. N need not be a
 * multiple of 16: the last tile is padded with zero rows, columns >= N are not written (epi 4 writes the 8 columns of every tile that holds a gate row:
 * ldo >= round_up(N, 16) / 2). The output bits are those of rdx_xstat16_test on the dequantised weight. */
int rdx_xstat16_w4_test(rdx_ctx* ctx, const void* X, const void* norm_w, float eps, const float* W, int M, int N, int epi, void* out, int ldo,
                        int out_packed, int raw_lo);
/* launch_xrow16_w4 (bf16 context): rdx_xrow16_test's arguments with K % 128 == 0, W quantised likewise (every tile int4). */
int rdx_xrow16_w4_test(rdx_ctx* ctx, const void* X, int x_packed, const float* W, const void* resid, int M, int N, int K, void* out, int ldo);

#ifdef __cplusplus
}
#endif
#endif /* RDX_DEC_HOOKS_H */
