/* rdx_enc_hooks.h -- the image encoder's kernel-test hooks: the stem, the LayerNorm / pooling kernels and the attention kernels one launch at a
 * time on caller data (tests/test_gpu_encoder_kernels.py). Like the hooks of rdx_hooks.h they live in radialog_amd/librdx_hooks.so (built from
 * radialog_amd/csrc/api_debug.hip, linked against librdx.so), never in the product library, and radialog_amd/_lib.py binds them (ENC_HOOK_SYMBOLS)
 * only under RDX_DEBUG_HOOKS=1. Each hook launches the production launch_* functions and nothing else; what it cannot run is an error. */
#ifndef RDX_ENC_HOOKS_H
#define RDX_ENC_HOOKS_H
#include "rdx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the image encoder's stem on caller data: img_prep_k, then path 0 = stem_pool_k (fused 7x7/2 conv + bias + ReLU + 3x3/2 max pool) writing row-major,
 * 1 = stem_pool_k writing the fragment-packed layout with the encoder's pad-row zeroing (unpacked for the caller; a nonzero pad row is an error),
 * 2 = the two-kernel path conv_gemm + maxpool_k. image fp32 [B][3][S][S] (S % 4 == 0); W fp32 [stem][7 * 8 * 4] in the (kh, kw, c) order
 * rdx_set_weight("v.conv1.w") takes (kw = 7 and c = 3 zero); bias fp32 [stem]; out [B][S / 4][S / 4][stem] model dtype. Test hook. */
int rdx_stem_test(rdx_ctx* ctx, const float* image, const float* W, const float* bias, void* out, int B, int S, int stem, int path);

/* the encoder's LayerNorm / pooling kernels on caller data (X, emb, out model dtype; gamma, beta, out_f32 fp32, out_f32 nullable):
 * op 0 layernorm_k [rows][H]; op 1 layernorm_ex_k with row strides ldx / ldo and emb[row % aux] added (emb nullable); op 2 layernorm_packed_k
 * (packed in, unpacked out, out_f32 from the kernel); op 3 scramble_layernorm_k over NHWC [rows = B][aux = P][H = C]; op 4 avgpool_flatten_k
 * [rows = B][aux = G][G][H = C] -> [B][C][G / pool][G / pool]. Test hook. */
int rdx_norm_test(rdx_ctx* ctx, int op, const void* X, const float* gamma, const float* beta, const void* emb, void* out, float* out_f32,
                  int rows, int H, long long ldx, long long ldo, int aux, int pool, float eps);

/* softmax(Q K^T / sqrt(D)) V through AttnArgs: strides[12] = element strides (batch, token, head) of Q, K, V, O; D 32 / 64 / 128; causal;
 * key_mask nullable uint8 [B][km_bs] (km_bs >= Tk, km_bs % 4 == 0); o_packed: O written fragment-packed and unpacked into out [B Tq][H D].
 * kernel 0 = production dispatch, 1 = attention_k, 2 = flash_prefill_k (an error where flash_prefill_supported does not hold). Test hook. */
int rdx_attn_test(rdx_ctx* ctx, const void* Q, const void* K, const void* V, void* out, const long long* strides, int B, int H, int Tq, int Tk,
                  int D, int causal, const uint8_t* key_mask, long long km_bs, int o_packed, int kernel);

#ifdef __cplusplus
}
#endif
#endif /* RDX_ENC_HOOKS_H */
