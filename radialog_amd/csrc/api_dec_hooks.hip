// librdx_hooks.so, second unit: the decoder's 3-16-row and row-block GEMM kernels, its RMSNorm, decode attention and the prompt's RoPE / KV write on caller data
// (include/rdx_dec_hooks.h; tests/test_gpu_decoder_gemms.py, tests/test_gpu_rmsnorm.py, tests/test_gpu_decode_attn.py). Every hook packs the caller's fp32 weight with the production packer, allocates its own temporaries (the test
// engines have no decoder: c->kslab / c->dxs / c->dxn do not exist), asks the production *_supported predicate BEFORE anything is launched on the
// caller's outputs, and calls the production launch_* functions unchanged. Temporaries the kernels only partly write are filled with 0xff bytes
// (NaN in both model dtypes and in fp32) first. The temporaries are a DevBufs, the weight forms and the common ending (finish) come from hook_util.h.
#include "hook_util.h"
#include "philox.h"
#include "../../include/rdx_dec_hooks.h"

namespace {

bool epi_args_ok(int epi, int N, int n_valid, int ldo, int out_packed, const void* resid, const int32_t* argmax_host) {
    if (epi == EPI_LOGITS && (!argmax_host || n_valid <= 0 || n_valid > N)) return false;
    if (epi == EPI_RESID && !resid) return false;
    if (epi == EPI_SILU_MUL && out_packed != ACT_ROWS) return true;
    return ldo >= (epi == EPI_SILU_MUL ? N / 2 : N);
}

// the hooks' RMSNorm / re-layout launches: no slabs unless given
NormArgs nargs(const void* x, const void* w, void* out, float* xscale, int rows, int H, float eps, ActLayout layout, int mtiles) {
    return NormArgs{const_cast<void*>(x), w, out, xscale, rows, H, eps, layout, mtiles, nullptr, 0};
}

}  // namespace

extern "C" int rdx_xstat16_test(rdx_ctx* c, const void* X, const void* norm_w, float eps, const float* W, int M, int N, int epi, int n_valid, void* out,
                                int ldo, int out_packed, int32_t* argmax_host) {
    if (!c || !X || !norm_w || !W || !out || M <= 0 || N <= 0 || N % 16) return fail(c, -1, "rdx_xstat16_test: bad arguments (N %% 16 == 0)");
    if (!epi_args_ok(epi, N, n_valid, ldo, out_packed, nullptr, argmax_host) || (out_packed != ACT_ROWS && (out_packed != ACT_BLK32 || epi != EPI_SILU_MUL || N % 64)))
        return fail(c, -1, "rdx_xstat16_test: epilogue arguments (ldo, n_valid, argmax_host; out_packed 1 with SwiGLU and N %% 64 == 0 only)");
    HIPCHK(c, hipSetDevice(c->device));
    const int K = 4096, nt = N / 16;
    DevBufs b;
    GemmW w; w.N = N; w.K = K; w.Npad = N;
    w.w = b.get((size_t)N * K * 2);
    float* pv = (float*)b.get((size_t)M * nt * 4);
    int* pi = (int*)b.get((size_t)M * nt * 4);
    if (!w.w || !pv || !pi) return fail(c, -2, "rdx_xstat16_test: out of device memory");
    GemmArgs a = gargs(X, K, w, nullptr, out, ldo, M);
    a.norm_w = norm_w; a.eps = eps; a.out_packed = (ActLayout)out_packed;
    if (epi == EPI_LOGITS) { a.n_valid = n_valid; a.part_val = pv; a.part_idx = pi; }
    if (!xstat16_supported(a, epi)) return fail(c, -1, "rdx_xstat16_test: %d x %d (epilogue %d) is not a shape of xstat16_k", M, N, epi);
    pack_w(c, W, w);
    launch_xstat16(c->cfg.dtype, a, epi, c->stream);
    if (int rc = finish(c)) return rc;
    return epi == EPI_LOGITS ? reduce_partials(c, a, argmax_host) : 0;
}

extern "C" int rdx_xrow16_test(rdx_ctx* c, const void* X, int x_packed, const float* W, const void* resid, int M, int N, int K, void* out, int ldo) {
    if (!c || !X || !W || !resid || !out || M <= 0 || N <= 0 || K <= 0 || N % 16 || K % 32 || ldo < N) return fail(c, -1, "rdx_xrow16_test: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    DevBufs b;
    GemmW w; w.N = N; w.K = K; w.Npad = N;
    w.w = b.get((size_t)N * K * 2);
    void* xp = x_packed ? nullptr : b.get((size_t)32 * K * 2);
    if (!w.w || (!x_packed && !xp)) return fail(c, -2, "rdx_xrow16_test: out of device memory");
    GemmArgs a = gargs(x_packed ? X : xp, K, w, nullptr, out, ldo, M);
    a.resid = resid; a.ldr = N; a.xpacked = ACT_BLK32;
    if (!xrow16_supported(a)) return fail(c, -1, "rdx_xrow16_test: %d x %d x %d is not a shape of xrow16_k", M, N, K);
    pack_w(c, W, w);
    if (!x_packed) run_rmsnorm(c, nargs(X, nullptr, xp, nullptr, M, K, 0.f, ACT_BLK32, 0));      // w = null: re-layout only
    launch_xrow16(c->cfg.dtype, a, c->stream);
    return finish(c);
}

extern "C" int rdx_xstat16_w4_test(rdx_ctx* c, const void* X, const void* norm_w, float eps, const float* W, int M, int N, int epi, void* out, int ldo,
                                   int out_packed, int raw_lo) {
    if (!c || !X || !norm_w || !W || !out || M <= 0 || N <= 0) return fail(c, -1, "rdx_xstat16_w4_test: bad arguments");
    // N need not fill its last tile: the rows up to npad are zeros in the stream and in the packed copy (launch_quant_w4), the kernel stores columns < N
    // (SwiGLU: the whole 8 columns of a tile that holds a gate row, hence ldo against npad)
    const int npad = (N + 15) / 16 * 16;
    if ((epi != EPI_NONE && epi != EPI_SILU_MUL) || !epi_args_ok(epi, epi == EPI_SILU_MUL ? npad : N, N, ldo, out_packed, nullptr, nullptr) ||
        (out_packed != ACT_ROWS && (out_packed != ACT_BLK32 || epi != EPI_SILU_MUL || N % 64)))
        return fail(c, -1, "rdx_xstat16_w4_test: epilogue arguments (epi 0 or 4; ldo; out_packed 1 with SwiGLU and N %% 64 == 0 only)");
    // raw_lo >= 0: the tiles from row raw_lo on are raw, as in rdx_set_weight; raw_lo < 0: the ONE tile of rows [-raw_lo, -raw_lo + 16) is (a raw tile between int4 tiles)
    const int lo = raw_lo < 0 ? -raw_lo : raw_lo >= N ? npad : raw_lo, hi = raw_lo < 0 ? lo + 16 : npad;
    if (lo % 16 || hi > npad) return fail(c, -1, "rdx_xstat16_w4_test: raw_lo = %d is no tile boundary inside N = %d", raw_lo, N);
    HIPCHK(c, hipSetDevice(c->device));
    const int K = 4096;
    DevBufs b;
    GemmW w; w.N = N; w.K = K; w.Npad = npad;
    if (c->cfg.dtype != DT_BF16) return fail(c, -8, "rdx_xstat16_w4_test: int4 weights need a bf16 context");
    if (int rc = quant_w4_for_test(c, b, W, w, lo, hi)) return fail(c, rc, "rdx_xstat16_w4_test: %s", rc == -2 ? "out of device memory" : "the weight holds an Inf or a NaN");
    GemmArgs a = gargs(X, K, w, nullptr, out, ldo, M);
    a.norm_w = norm_w; a.eps = eps; a.out_packed = (ActLayout)out_packed;
    a.W4 = w.w4; a.w4hdr = w.w4h;
    if (!xstat16_w4_supported(c->cfg.dtype, a, epi)) return fail(c, -1, "rdx_xstat16_w4_test: %d x %d (epilogue %d) is not a shape of xstat16_w4_k", M, N, epi);
    launch_xstat16_w4(a, epi, c->stream);
    return finish(c);
}

extern "C" int rdx_xrow16_w4_test(rdx_ctx* c, const void* X, int x_packed, const float* W, const void* resid, int M, int N, int K, void* out, int ldo) {
    if (!c || !X || !W || !resid || !out || M <= 0 || N <= 0 || K <= 0 || N % 16 || K % W4_CHUNK_K || ldo < N) return fail(c, -1, "rdx_xrow16_w4_test: bad arguments (K %% 128 == 0)");
    if (c->cfg.dtype != DT_BF16) return fail(c, -8, "rdx_xrow16_w4_test: int4 weights need a bf16 context");
    HIPCHK(c, hipSetDevice(c->device));
    DevBufs b;
    GemmW w; w.N = N; w.K = K; w.Npad = N;
    void* xp = x_packed ? nullptr : b.get((size_t)32 * K * 2);
    if (!x_packed && !xp) return fail(c, -2, "rdx_xrow16_w4_test: out of device memory");
    if (int rc = quant_w4_for_test(c, b, W, w, N, N)) return fail(c, rc, "rdx_xrow16_w4_test: %s", rc == -2 ? "out of device memory" : "the weight holds an Inf or a NaN");
    GemmArgs a = gargs(x_packed ? X : xp, K, w, nullptr, out, ldo, M);
    a.resid = resid; a.ldr = N; a.xpacked = ACT_BLK32;
    a.W4 = w.w4; a.w4hdr = w.w4h;
    if (!xrow16_w4_supported(c->cfg.dtype, a)) return fail(c, -1, "rdx_xrow16_w4_test: %d x %d x %d is not a shape of xrow16_w4_k", M, N, K);
    if (!x_packed) run_rmsnorm(c, nargs(X, nullptr, xp, nullptr, M, K, 0.f, ACT_BLK32, 0));      // w = null: re-layout only
    launch_xrow16_w4(a, c->stream);
    return finish(c);
}

extern "C" int rdx_xstat_blk_test(rdx_ctx* c, const void* X, const void* norm_w, float eps, const float* W, const void* resid, int M, int N, int epi,
                                  int n_valid, void* out, int ldo, int out_packed, void* xp_out, int32_t* argmax_host) {
    if (!c || !X || !W || !out || M <= 0 || M > 192 || N <= 0 || N % 16) return fail(c, -1, "rdx_xstat_blk_test: bad arguments (M <= 192, N %% 16 == 0)");
    if (!epi_args_ok(epi, N, n_valid, ldo, out_packed, resid, argmax_host) || (out_packed != ACT_ROWS && (out_packed != ACT_TILES32 || epi != EPI_SILU_MUL || N % 64)))
        return fail(c, -1, "rdx_xstat_blk_test: epilogue arguments (ldo, resid, n_valid, argmax_host; out_packed 3 with SwiGLU and N %% 64 == 0 only)");
    HIPCHK(c, hipSetDevice(c->device));
    const int K = 4096, nt = N / 16, mtl = (M + 15) / 16;
    const size_t xpb = (size_t)mtl * 16 * K * 2;
    DevBufs b;
    GemmW w; w.N = N; w.K = K; w.Npad = N;
    w.w = b.get((size_t)N * K * 2);
    void* xp = b.get(xpb);
    float* pv = (float*)b.get((size_t)M * nt * 4);
    int* pi = (int*)b.get((size_t)M * nt * 4);
    if (!w.w || !xp || !pv || !pi) return fail(c, -2, "rdx_xstat_blk_test: out of device memory");
    GemmArgs a = with_switches(c, gargs(xp, K, w, nullptr, out, ldo, M));
    a.xpacked = ACT_TILES32; a.mtiles = mtl; a.out_packed = (ActLayout)out_packed;
    if (epi == EPI_RESID) { a.resid = resid; a.ldr = N; }
    if (epi == EPI_LOGITS) { a.n_valid = n_valid; a.part_val = pv; a.part_idx = pi; }
    if (!xstat_blk_supported(a, epi)) return fail(c, -1, "rdx_xstat_blk_test: %d x %d (epilogue %d) is not a shape of the row-block xstat32_k", M, N, epi);
    pack_w(c, W, w);
    HIPCHK(c, hipMemsetAsync(xp, 0xff, xpb, c->stream));
    run_rmsnorm(c, nargs(X, norm_w, xp, nullptr, M, K, eps, ACT_TILES32, mtl));
    launch_xstat_blk(c->cfg.dtype, a, epi, c->stream);
    if (xp_out) HIPCHK(c, hipMemcpyAsync(xp_out, xp, xpb, hipMemcpyDeviceToDevice, c->stream));
    if (int rc = finish(c)) return rc;
    return epi == EPI_LOGITS ? reduce_partials(c, a, argmax_host) : 0;
}

extern "C" int rdx_xsplit_blk_test(rdx_ctx* c, const void* X, const float* W, void* x_resid, const void* norm_w, float eps, int M, int N, float* slab_out,
                                   void* xn_out) {
    if (!c || !X || !W || M <= 0 || M > 192 || N <= 0 || N % 16 || (!slab_out && !x_resid)) return fail(c, -1, "rdx_xsplit_blk_test: bad arguments");
    if ((x_resid != nullptr) != (xn_out != nullptr) || (x_resid && (!norm_w || N != 4096)))
        return fail(c, -1, "rdx_xsplit_blk_test: the slab combine (x_resid, norm_w, xn_out together) is the 4096-wide RMSNorm: N = 4096 only");
    HIPCHK(c, hipSetDevice(c->device));
    const int K = 11008, mtl = (M + 15) / 16, groups = 4;
    const size_t xpb = (size_t)mtl * 16 * K * 2, sb = (size_t)groups * 16 * mtl * N * 4;
    DevBufs b;
    GemmW w; w.N = N; w.K = K; w.Npad = N;
    w.w = b.get((size_t)N * K * 2);
    void* xp = b.get(xpb);
    float* slab = (float*)b.get(sb);
    if (!w.w || !xp || !slab) return fail(c, -2, "rdx_xsplit_blk_test: out of device memory");
    GemmArgs a = with_switches(c, gargs(xp, K, w, nullptr, nullptr, N, M));
    a.xpacked = ACT_TILES32; a.mtiles = mtl;
    if (!xsplit_blk_supported(a)) return fail(c, -1, "rdx_xsplit_blk_test: %d x %d is not a shape of the row-block xsplit32_k", M, N);
    pack_w(c, W, w);
    HIPCHK(c, hipMemsetAsync(xp, 0xff, xpb, c->stream));
    HIPCHK(c, hipMemsetAsync(slab, 0xff, sb, c->stream));
    run_rmsnorm(c, nargs(X, nullptr, xp, nullptr, M, K, eps, ACT_TILES32, mtl));       // w = null: re-layout only
    launch_xsplit_blk(c->cfg.dtype, a, slab, c->stream);
    if (slab_out) HIPCHK(c, hipMemcpyAsync(slab_out, slab, sb, hipMemcpyDeviceToDevice, c->stream));
    if (x_resid) run_rmsnorm(c, NormArgs{x_resid, norm_w, xn_out, nullptr, M, N, eps, ACT_TILES32, mtl, slab, groups});
    return finish(c);
}

extern "C" int rdx_xstat_blk8_test(rdx_ctx* c, const void* X, const void* norm_w, float eps, const float* W, int M, int N, int epi, int n_valid, void* out,
                                   int ldo, int out_packed, void* x8_out, float* xscale_out, int32_t* argmax_host) {
    if (!c || !X || !norm_w || !W || !out || M <= 0 || M > 128 || N <= 0 || N % 16) return fail(c, -1, "rdx_xstat_blk8_test: bad arguments (norm_w, M <= 128, N %% 16 == 0)");
    if (!epi_args_ok(epi, N, n_valid, ldo, out_packed, nullptr, argmax_host) || (out_packed != ACT_ROWS && (out_packed != ACT_BLK64 || epi != EPI_SILU_MUL || N % 128)))
        return fail(c, -1, "rdx_xstat_blk8_test: epilogue arguments (ldo, n_valid, argmax_host; out_packed 2 with SwiGLU and N %% 128 == 0 only)");
    HIPCHK(c, hipSetDevice(c->device));
    const int K = 4096, nt = N / 16, mtl = (M + 15) / 16, NB = (mtl + 1) / 2;
    const size_t x8b = (size_t)NB * 32 * K;
    DevBufs b;
    GemmW w; w.N = N; w.K = K; w.Npad = N;
    w.w8 = b.get((size_t)N * K);
    w.scale = (float*)b.get((size_t)N * 4);
    void* x8 = b.get(x8b);
    float* xs = (float*)b.get((size_t)NB * 32 * 4);
    float* pv = (float*)b.get((size_t)M * nt * 4);
    int* pi = (int*)b.get((size_t)M * nt * 4);
    if (!w.w8 || !w.scale || !x8 || !xs || !pv || !pi) return fail(c, -2, "rdx_xstat_blk8_test: out of device memory");
    GemmArgs a = with_switches(c, gargs(x8, K, w, nullptr, out, ldo, M));
    a.xpacked = ACT_BLK64_E4M3; a.xscale = xs; a.xgroups = 1; a.mtiles = mtl; a.out_packed = (ActLayout)out_packed;
    if (epi == EPI_LOGITS) { a.n_valid = n_valid; a.part_val = pv; a.part_idx = pi; }
    if (!xstat_blk8_supported(a, epi)) return fail(c, -1, "rdx_xstat_blk8_test: %d x %d (epilogue %d) is not a shape of the fp8 row-block xstat32_k", M, N, epi);
    pack_w8(c, W, w);
    run_rmsnorm(c, nargs(X, norm_w, x8, xs, M, K, eps, ACT_BLK64_E4M3, mtl));
    launch_xstat_blk8(c->cfg.dtype, a, epi, c->stream);
    if (x8_out) HIPCHK(c, hipMemcpyAsync(x8_out, x8, x8b, hipMemcpyDeviceToDevice, c->stream));
    if (xscale_out) HIPCHK(c, hipMemcpyAsync(xscale_out, xs, (size_t)NB * 32 * 4, hipMemcpyDeviceToDevice, c->stream));
    if (int rc = finish(c)) return rc;
    return epi == EPI_LOGITS ? reduce_partials(c, a, argmax_host) : 0;
}

extern "C" int rdx_xsplit_blk8_test(rdx_ctx* c, const void* X, const float* W, void* x_resid, const void* norm_w, float eps, int M, int N, int K,
                                    float* slab_out, void* x8_out, float* xscale_out) {
    if (!c || !X || !W || M <= 0 || M > 128 || N <= 0 || N % 16 || !(K == 4096 || K == 11008) || (!slab_out && !x_resid))
        return fail(c, -1, "rdx_xsplit_blk8_test: bad arguments (M <= 128, N %% 16 == 0, K 4096 or 11008)");
    if ((x_resid != nullptr) != (x8_out != nullptr) || (x_resid != nullptr) != (xscale_out != nullptr) || (x_resid && (!norm_w || N != 4096)))
        return fail(c, -1, "rdx_xsplit_blk8_test: the slab combine (x_resid, norm_w, x8_out, xscale_out together) is the 4096-wide RMSNorm: N = 4096 only");
    HIPCHK(c, hipSetDevice(c->device));
    const int mtl = (M + 15) / 16, NB = (mtl + 1) / 2;
    const size_t xpb = (size_t)NB * 32 * K * 2;
    DevBufs b;
    GemmW w; w.N = N; w.K = K; w.Npad = N;
    w.w8 = b.get((size_t)N * K);
    w.scale = (float*)b.get((size_t)N * 4);
    char* xp = (char*)b.get(xpb);
    if (!w.w8 || !w.scale || !xp) return fail(c, -2, "rdx_xsplit_blk8_test: out of device memory");
    GemmArgs a = with_switches(c, gargs(xp, K, w, nullptr, nullptr, N, M));
    a.xpacked = ACT_BLK64; a.mtiles = mtl;
    const int groups = xsplit_blk8_groups(a);
    if (!groups) return fail(c, -1, "rdx_xsplit_blk8_test: %d x %d x %d is not a shape of the fp8 row-block xsplit32_k", M, N, K);
    const size_t sb = (size_t)groups * 32 * NB * N * 4;
    float* slab = (float*)b.get(sb);
    if (!slab) return fail(c, -2, "rdx_xsplit_blk8_test: out of device memory");
    pack_w8(c, W, w);
    HIPCHK(c, hipMemsetAsync(slab, 0xff, sb, c->stream));
    for (int blk = 0; blk < NB; ++blk)      // every 32-row block in the 64-deep order of the fp8 kernels, rows past M zero: the re-layout launch of rdx_gemm_test's fp8 K-split mode
        run_rmsnorm(c, nargs((const char*)X + (size_t)blk * 32 * K * 2, nullptr, xp + (size_t)blk * 32 * K * 2, nullptr, std::min(32, M - 32 * blk), K, eps, ACT_BLK64, 0));
    launch_xsplit_blk8(c->cfg.dtype, a, slab, c->stream);
    if (slab_out) HIPCHK(c, hipMemcpyAsync(slab_out, slab, sb, hipMemcpyDeviceToDevice, c->stream));
    if (x_resid) run_rmsnorm(c, NormArgs{x_resid, norm_w, x8_out, xscale_out, M, N, eps, ACT_BLK64_E4M3, mtl, slab, groups});
    return finish(c);
}

extern "C" int rdx_rmsnorm_test(rdx_ctx* c, void* x, const void* w, float eps, int rows, int H, int layout, int mtiles, const float* slab, int groups, void* out,
                                long long out_bytes, float* xscale, int xscale_n) {
    if (!c || !x || !out || out_bytes <= 0 || (xscale && xscale_n <= 0)) return fail(c, -1, "rdx_rmsnorm_test: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(out, 0xff, (size_t)out_bytes, c->stream));
    if (xscale) HIPCHK(c, hipMemsetAsync(xscale, 0xff, (size_t)xscale_n * 4, c->stream));
    run_rmsnorm(c, NormArgs{x, w, out, xscale, rows, H, eps, (ActLayout)layout, mtiles, slab, groups});
    return finish(c);
}

extern "C" int rdx_select_test(rdx_ctx* c, void* logits_inout, int B, int vocab, const int32_t* hist, const int32_t* hist_len, const int32_t* n_generated, int ld,
                               const rdx_logits_rules* rules, int eos_id, int32_t* tokens_out) {
    if (!c || !logits_inout || !hist || !hist_len || !n_generated || !rules || !tokens_out || B <= 0 || ld <= 0)
        return fail(c, -1, "rdx_select_test: bad arguments");
    if (!(rules->repetition_penalty > 0.f) || rules->no_repeat_ngram_size < 0 || rules->min_new_tokens < 0) return fail(c, -1, "rdx_select_test: bad rules");
    if (!select_step_supported(vocab)) return fail(c, -1, "rdx_select_test: vocab %d exceeds the LDS bitmaps of select_step_k", vocab);
    HIPCHK(c, hipSetDevice(c->device));
    SelectArgs a;
    a.logits = logits_inout; a.step_stride = 0; a.n_gen = n_generated;
    a.penalty = rules->repetition_penalty; a.ngram = rules->no_repeat_ngram_size; a.min_new = rules->min_new_tokens; a.sel_out = tokens_out;
    StepTail t = {};
    t.vocab = vocab; t.eos_id = eos_id;
    t.hist = const_cast<int32_t*>(hist); t.hist_len = const_cast<int32_t*>(hist_len); t.hist_ld = ld;       // read only: with sel_out set the tail does not run
    launch_select_step(c->cfg.dtype, a, t, B, c->stream);
    return finish(c);
}

extern "C" int rdx_score_rows_test(rdx_ctx* c, const void* logits, int M, int vocab, int ld, const int32_t* target, float* logprob_out, int32_t* top1_out) {
    if (!c || !logits || !target || !logprob_out || !top1_out || M <= 0) return fail(c, -1, "rdx_score_rows_test: bad arguments");
    if (((uintptr_t)logits & 15) || !score_rows_supported(vocab, ld))
        return fail(c, -1, "rdx_score_rows_test: rows of vocab %d at stride %d (a multiple of 8 >= vocab, 16-byte aligned base, the row within the LDS of score_rows_k)", vocab, ld);
    HIPCHK(c, hipSetDevice(c->device));
    launch_score_rows(c->cfg.dtype, logits, ld, target, vocab, logprob_out, top1_out, M, c->stream);
    return finish(c);
}

extern "C" int rdx_logprob_step_test(rdx_ctx* c, const void* logits, long long row_stride, long long step_stride, const int32_t* d_step, const int32_t* tokens,
                                     int B, int vocab, int max_new, int top_n, float* chosen_out, int32_t* top_ids_out, float* top_lp_out, int out_ld) {
    if (!c || !logits || !d_step || !tokens || !chosen_out || !top_ids_out || !top_lp_out || B <= 0 || max_new <= 0 || out_ld < max_new || row_stride < 0 || step_stride < 0)
        return fail(c, -1, "rdx_logprob_step_test: bad arguments");
    if (top_n < 0 || top_n > RDX_MAX_TOP_LOGPROBS) return fail(c, -1, "rdx_logprob_step_test: top_n %d outside [0, %d]", top_n, RDX_MAX_TOP_LOGPROBS);
    if (((uintptr_t)logits & 1) || !logprob_step_supported(vocab)) return fail(c, -1, "rdx_logprob_step_test: a row of vocab %d does not fit the LDS of logprob_step_k", vocab);
    HIPCHK(c, hipSetDevice(c->device));
    LogprobArgs a;
    a.logits = logits; a.row_stride = (long)row_stride; a.step_stride = (long)step_stride; a.d_step = d_step; a.tokens = tokens;
    a.B = B; a.max_new = max_new; a.vocab = vocab; a.top_n = top_n;
    a.chosen = chosen_out; a.top_ids = top_ids_out; a.top_lp = top_lp_out; a.out_ld = out_ld;
    launch_logprob_step(c->cfg.dtype, a, c->stream);
    return finish(c);
}

extern "C" int rdx_lookup_accept_test(rdx_ctx* c, const float* part_val, const int32_t* part_idx, int n_tiles, int d, int32_t* tail, const int32_t* corpus,
                                      int n_corpus, int draft_len, int ngram_max, int ngram_min, int slot_end, int32_t* hist, int hist_ld, int32_t* state,
                                      int advance, int eos_id, int pad_id, int max_new, int32_t* out_tokens, const void* logits, void* scores, int32_t* status,
                                      int32_t* trace, int trace_cap, int32_t* pos_ids) {
    if (!c || !part_val || !part_idx || !tail || !hist || !state || !out_tokens || !status || !pos_ids || n_tiles <= 0 || hist_ld <= 0 || max_new <= 0 ||
        n_corpus < 0 || (n_corpus && !corpus) || trace_cap < 0)
        return fail(c, -1, "rdx_lookup_accept_test: bad arguments");
    if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_lookup_accept_test: needs a finalized llama context (the embedding and RoPE tables are its own)");
    if (d < 0 || d > LOOKUP_MAX_DRAFT || draft_len < 0 || draft_len > LOOKUP_MAX_DRAFT || ngram_max < 1 || ngram_max > LOOKUP_MAX_NGRAM || ngram_min < 1 || ngram_min > ngram_max)
        return fail(c, -1, "rdx_lookup_accept_test: d / draft_len outside [0, %d] or n-gram sizes outside 1 <= min <= max <= %d", LOOKUP_MAX_DRAFT, LOOKUP_MAX_NGRAM);
    HIPCHK(c, hipSetDevice(c->device));
    // refused before anything is written: a state that would carry a store or a table read out of the caller's arrays
    int st[5], fwd = 0;
    HIPCHK(c, hipMemcpy(st, state, sizeof(st), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(&fwd, status + LKS_FWD, sizeof(int), hipMemcpyDeviceToHost));
    if (st[0] < 0 || st[2] < 0 || st[2] + LOOKUP_MAX_DRAFT + 1 >= c->cfg.max_pos || st[4] < 0 || st[4] > hist_ld || fwd < 0)
        return fail(c, -1, "rdx_lookup_accept_test: state (step %d, position %d, history %d of %d) outside the caller's arrays / the RoPE tables", st[0], st[2], st[4], hist_ld);
    DevBufs bufs;
    int* par = (int*)bufs.get(LKP_INTS * sizeof(int));
    int* img = (int*)bufs.get(sizeof(int));
    int* one = (int*)bufs.get(sizeof(int));      // stands in for a null corpus
    if (!par || !img || !one) return fail(c, -2, "rdx_lookup_accept_test: out of device memory");
    const int ph[LKP_INTS] = {n_corpus, draft_len, ngram_max, ngram_min, slot_end};
    HIPCHK(c, hipMemcpy(par, ph, sizeof(ph), hipMemcpyHostToDevice));
    const rdx_config& f = c->cfg;
    StepTail t = {};
    t.eos_id = eos_id; t.pad_id = pad_id; t.max_new = max_new; t.out_tokens = out_tokens;
    t.step_b = state; t.unfinished = state + 3; t.hist_len = state + 4; t.hist = hist; t.hist_ld = hist_ld;
    t.pos_ro = state + 2; t.pos = advance ? state + 2 : nullptr; t.slot_b = advance ? state + 1 : nullptr;
    t.embed = c->embed; t.vocab = f.vocab; t.x_next = c->dx; t.H = f.hidden; t.cos_t = c->rope_cos; t.sin_t = c->rope_sin; t.cur_rope = c->d_cur_rope;
    LookupArgs a;
    a.part_val = part_val; a.part_idx = part_idx; a.n_tiles = n_tiles; a.d = d; a.logits = logits; a.scores = scores;
    a.tail = tail; a.slot = state + 1; a.pos_ids = pos_ids; a.img_pos = img; a.status = status; a.trace = trace; a.trace_cap = trace_cap;
    a.par = par; a.corpus = corpus ? corpus : one;
    launch_lookup_accept(f.dtype, a, t, c->stream);
    return finish(c);
}

namespace {

// the dims both attention hooks build: hidden = 128 heads, the QKV row as the engine lays it out (api.hip: wqkv.Npad)
bool attn_dims(LlamaDims& d, int heads, int max_len, int k_perm, int lora_r, float lora_scale, int max_pos) {
    if (heads <= 0 || heads > 64 || max_len <= 0 || max_len > 1536 || max_len % 32 || !(lora_r == 0 || lora_r == 8)) return false;
    d.hidden = 128 * heads; d.heads = heads; d.head_dim = 128; d.qkv_ld = (3 * d.hidden + 2 * lora_r + 15) / 16 * 16;
    d.lora_r = lora_r; d.lora_scale = lora_scale; d.max_len = max_len; d.max_pos = max_pos; d.k_perm = k_perm ? 1 : 0;
    return true;
}

}  // namespace

namespace {

// both decode-attention hooks: the checks, then the launch on the model-dtype caches or (kexp / vexp given) on the fp8 codes and exponents
int decode_attn_hook(rdx_ctx* c, const char* who, int heads, int B, int max_len, int k_perm, int lora_r, float lora_scale, const void* qkv, const void* lbq,
                     const void* lbv, const void* cur_rope, const void* cos_t, const void* sin_t, int max_pos, const int32_t* pos, const int32_t* slot,
                     const uint8_t* key_mask, void* kcache, void* vcache, signed char* kexp, signed char* vexp, void* out, long long out_bytes, int out_packed,
                     int out_mt) {
    if (!c || !qkv || !slot || !key_mask || !kcache || !vcache || !out || B <= 0 || B > 4096) return fail(c, -1, "%s: bad arguments", who);
    DecAttnArgs a;
    if (!attn_dims(a.d, heads, max_len, k_perm, lora_r, lora_scale, max_pos))
        return fail(c, -1, "%s: heads %d, max_len %d (a multiple of 32 in (0, 1536]), lora_r %d (0 or 8)", who, heads, max_len, lora_r);
    if (lora_r && (!lbq || !lbv)) return fail(c, -1, "%s: lora_r 8 needs lbq and lbv", who);
    const bool tables = cos_t && sin_t && pos && max_pos > 0;
    if ((cur_rope != nullptr) == tables || (!cur_rope && (cos_t || sin_t || pos) && !tables))
        return fail(c, -1, "%s: either cur_rope, or cos_t / sin_t / pos with max_pos > 0", who);
    const size_t H = a.d.hidden;
    size_t extent = 0;      // bytes the layout holds; 0: it does not hold B rows
    switch (out_packed) {
    case ACT_ROWS: extent = (size_t)B * H * 2; break;
    case ACT_BLK32: out_mt = 2; extent = B <= 32 ? 32 * H * 2 : 0; break;
    case ACT_BLK64: extent = (size_t)((B + 31) / 32) * 32 * H * 2; break;
    case ACT_TILES32: extent = (out_mt > 0 && B <= 16 * out_mt) ? (size_t)16 * out_mt * H * 2 : 0; break;
    default: break;
    }
    if (!extent || out_bytes < (long long)extent)
        return fail(c, -1, "%s: out_packed %d (out_mt %d, %lld bytes) does not hold %d rows", who, out_packed, out_mt, out_bytes, B);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> hs(B), hp(B);
    std::vector<uint8_t> hm((size_t)B * max_len);
    HIPCHK(c, hipMemcpy(hs.data(), slot, (size_t)B * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(hm.data(), key_mask, hm.size(), hipMemcpyDeviceToHost));
    if (tables) HIPCHK(c, hipMemcpy(hp.data(), pos, (size_t)B * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < B; ++b) {
        if (hs[b] < 1 || hs[b] > max_len - 1) return fail(c, -1, "%s: row %d: slot %d outside [1, %d]", who, b, hs[b], max_len - 1);
        if (!hm[(size_t)b * max_len + hs[b]]) return fail(c, -1, "%s: row %d: the mask byte of its own slot %d is zero", who, b, hs[b]);
        if (tables && (hp[b] < 0 || hp[b] >= max_pos)) return fail(c, -1, "%s: row %d: position %d outside the tables [0, %d)", who, b, hp[b], max_pos);
    }
    a.qkv = qkv; a.lbq = lbq; a.lbv = lbv; a.cos_t = cos_t; a.sin_t = sin_t; a.cur_rope = cur_rope; a.pos = pos; a.slot_b = slot; a.key_mask = key_mask;
    a.kcache = kcache; a.vcache = vcache; a.out = out; a.out_packed = (ActLayout)out_packed; a.out_mt = out_mt;
    HIPCHK(c, hipMemsetAsync(out, 0xff, (size_t)out_bytes, c->stream));
    if (kexp) { a.d.kv_fp8 = 1; launch_decode_attention_kv8(c->cfg.dtype, a, kexp, vexp, B, attn_sw(c), c->stream); }
    else launch_decode_attention(c->cfg.dtype, a, B, attn_sw(c), c->stream);
    return finish(c);
}

}  // namespace

extern "C" int rdx_decode_attn_test(rdx_ctx* c, int heads, int B, int max_len, int k_perm, int lora_r, float lora_scale, const void* qkv, const void* lbq,
                                    const void* lbv, const void* cur_rope, const void* cos_t, const void* sin_t, int max_pos, const int32_t* pos,
                                    const int32_t* slot, const uint8_t* key_mask, void* kcache, void* vcache, void* out, long long out_bytes, int out_packed,
                                    int out_mt) {
    return decode_attn_hook(c, "rdx_decode_attn_test", heads, B, max_len, k_perm, lora_r, lora_scale, qkv, lbq, lbv, cur_rope, cos_t, sin_t, max_pos, pos, slot, key_mask,
                            kcache, vcache, nullptr, nullptr, out, out_bytes, out_packed, out_mt);
}

extern "C" int rdx_decode_attn_kv8_test(rdx_ctx* c, int heads, int B, int max_len, int lora_r, float lora_scale, const void* qkv, const void* lbq, const void* lbv,
                                        const void* cur_rope, const void* cos_t, const void* sin_t, int max_pos, const int32_t* pos, const int32_t* slot,
                                        const uint8_t* key_mask, void* kcodes, void* kexp, void* vcodes, void* vexp, void* out, long long out_bytes, int out_packed,
                                        int out_mt) {
    if (!kexp || !vexp) return fail(c, -1, "rdx_decode_attn_kv8_test: bad arguments");
    return decode_attn_hook(c, "rdx_decode_attn_kv8_test", heads, B, max_len, 0, lora_r, lora_scale, qkv, lbq, lbv, cur_rope, cos_t, sin_t, max_pos, pos, slot, key_mask,
                            kcodes, vcodes, (signed char*)kexp, (signed char*)vexp, out, out_bytes, out_packed, out_mt);
}

extern "C" int rdx_kv8_quant_test(rdx_ctx* c, int heads, int B, int T, int stage_len, int max_len, int slot0, const void* krows, const void* vrows, void* kcodes,
                                  void* kexp, void* vcodes, void* vexp) {
    if (!c || !krows || !vrows || !kcodes || !kexp || !vcodes || !vexp || heads <= 0 || B <= 0 || T <= 0) return fail(c, -1, "rdx_kv8_quant_test: bad arguments");
    if (stage_len < T || max_len % 16 || slot0 < 0 || T > max_len || slot0 > max_len - T)
        return fail(c, -1, "rdx_kv8_quant_test: %d staged rows of stride %d into slots [%d, %d + %d) of max_len %d (a multiple of 16)", T, stage_len, slot0, slot0, T, max_len);
    HIPCHK(c, hipSetDevice(c->device));
    launch_kv8_quant_rows(c->cfg.dtype, krows, vrows, stage_len, kcodes, (signed char*)kexp, vcodes, (signed char*)vexp, (size_t)B * heads, max_len, T, slot0, c->stream);
    return finish(c);
}

// logical model-dtype rows [B][heads][max_len][128] into a PLAIN context's cache of one layer (K in the order the context keeps it)
extern "C" int rdx_kv_write_test(rdx_ctx* c, int layer, int which, const void* src) {
    if (!c || !c->finalized || !c->cfg.enable_llama || !src || layer < 0 || layer >= c->cfg.layers) return fail(c, -1, "rdx_kv_write_test: bad arguments");
    if (c->sw.kv_fp8) return fail(c, -1, "rdx_kv_write_test: a plain (model-dtype) KV cache is needed, this context's is fp8 (kv_fp8)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = c->kv_layer_elems * 2;
    if (which || !c->ld.k_perm) {
        HIPCHK(c, hipMemcpyAsync(kv_ptr(c, which ? c->vcache : c->kcache, layer), src, bytes, hipMemcpyDeviceToDevice, c->stream));
    } else {
        // the fragment order on the host: element offsets from kperm() itself
        const int L = c->cfg.max_len;
        const size_t slabs = c->kv_layer_elems / ((size_t)L * 128);
        std::vector<unsigned short> in(c->kv_layer_elems), outv(c->kv_layer_elems);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(in.data(), src, bytes, hipMemcpyDeviceToHost));
        for (size_t sl = 0; sl < slabs; ++sl)
            for (int p = 0; p < L; ++p)
                for (int d8 = 0; d8 < 128; d8 += 8)
                    memcpy(&outv[sl * L * 128 + kperm(p, d8, 1)], &in[sl * L * 128 + (size_t)p * 128 + d8], 16);
        HIPCHK(c, hipMemcpy(kv_ptr(c, c->kcache, layer), outv.data(), bytes, hipMemcpyHostToDevice));
    }
    return finish(c);
}

extern "C" int rdx_rope_kv_test(rdx_ctx* c, int heads, int B, int T, int max_len, int k_perm, int lora_r, float lora_scale, const void* qkv, const void* lbq,
                                const void* lbv, const void* cos_t, const void* sin_t, int max_pos, const int32_t* pos_ids, int slot0, void* kcache,
                                void* vcache, void* qout) {
    if (!c || !qkv || !cos_t || !sin_t || !pos_ids || !kcache || !vcache || !qout || B <= 0 || B > 4096 || T <= 0 || max_pos <= 0)
        return fail(c, -1, "rdx_rope_kv_test: bad arguments");
    LlamaDims d;
    if (!attn_dims(d, heads, max_len, k_perm, lora_r, lora_scale, max_pos))
        return fail(c, -1, "rdx_rope_kv_test: heads %d, max_len %d (a multiple of 32 in (0, 1536]), lora_r %d (0 or 8)", heads, max_len, lora_r);
    if (lora_r && (!lbq || !lbv)) return fail(c, -1, "rdx_rope_kv_test: lora_r 8 needs lbq and lbv");
    if (slot0 < 0 || T > max_len || slot0 > max_len - T) return fail(c, -1, "rdx_rope_kv_test: slots [%d, %d + %d) do not fit max_len %d", slot0, slot0, T, max_len);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> hp((size_t)B * T);
    HIPCHK(c, hipMemcpy(hp.data(), pos_ids, hp.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < hp.size(); ++i)
        if (hp[i] < 0 || hp[i] >= max_pos) return fail(c, -1, "rdx_rope_kv_test: position id %d (row %d, token %d) outside the tables [0, %d)", hp[i], (int)(i / T), (int)(i % T), max_pos);
    HIPCHK(c, hipMemsetAsync(qout, 0xff, (size_t)B * T * d.hidden * 2, c->stream));
    launch_rope_kv_prefill(c->cfg.dtype, d, qkv, lbq, lbv, cos_t, sin_t, pos_ids, qout, kcache, vcache, B, T, slot0, c->stream);
    return finish(c);
}

extern "C" int rdx_sample_test(rdx_ctx* c, void* logits_inout, int B, int vocab, const int32_t* hist, const int32_t* hist_len, const int32_t* n_generated, int ld,
                               const rdx_logits_rules* rules, int eos_id, const rdx_sampling* sm, int32_t* tokens_out) {
    if (!c || !logits_inout || !n_generated || !sm || !tokens_out || B <= 0) return fail(c, -1, "rdx_sample_test: bad arguments");
    const rdx_logits_rules r = rules ? *rules : rdx_logits_rules{1.0f, 0, 0};
    const bool ruled = r.repetition_penalty != 1.0f || r.no_repeat_ngram_size != 0 || r.min_new_tokens != 0;
    if (!(r.repetition_penalty > 0.f) || r.no_repeat_ngram_size < 0 || r.min_new_tokens < 0) return fail(c, -1, "rdx_sample_test: bad rules");
    if (ruled && (!hist || !hist_len || ld <= 0)) return fail(c, -1, "rdx_sample_test: rules need a history");
    if (!(sm->temperature > 0.f) || !std::isfinite(sm->temperature) || sm->top_k < 0 || !(sm->top_p > 0.f) || !(sm->top_p <= 1.0f))
        return fail(c, -1, "rdx_sample_test: bad sampling parameters");
    if (!sample_step_supported(vocab) || (ruled && !select_step_supported(vocab))) return fail(c, -1, "rdx_sample_test: a row of vocab %d does not fit the LDS of sample_step_k", vocab);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_seed) ALLOC(c, c->d_seed, sizeof(unsigned long long));
    const unsigned long long seed = sm->seed;
    HIPCHK(c, hipMemcpyAsync(c->d_seed, &seed, sizeof(seed), hipMemcpyHostToDevice, c->stream));
    SelectArgs a;
    a.logits = logits_inout; a.step_stride = 0; a.n_gen = n_generated;
    a.penalty = r.repetition_penalty; a.ngram = r.no_repeat_ngram_size; a.min_new = r.min_new_tokens; a.sel_out = tokens_out;
    StepTail t = {};
    t.vocab = vocab; t.eos_id = eos_id;
    if (ruled) { t.hist = const_cast<int32_t*>(hist); t.hist_len = const_cast<int32_t*>(hist_len); t.hist_ld = ld; }     // read only: with sel_out set the tail does not run
    const SampleArgs sp = {sm->temperature, sm->top_k, sm->top_p, c->d_seed};
    launch_sample_step(c->cfg.dtype, a, sp, t, B, c->stream);
    return finish(c);
}

extern "C" int rdx_sample_u24_host(uint64_t seed, uint32_t row, uint32_t draw, uint32_t* out) {
    if (!out) return -1;
    *out = sample_u24(seed, row, draw);
    return 0;
}

extern "C" int rdx_wcode_test(rdx_ctx* c, const float* W, int N, int K, void* packed_out, void* planes_out, uint32_t* hdr_out) {
    if (!c || !W || !packed_out || !planes_out || !hdr_out || N <= 0 || K <= 0) return fail(c, -1, "rdx_wcode_test: bad arguments");
    if (c->cfg.dtype != DT_BF16 || K % WC_CHUNK_K) return fail(c, -1, "rdx_wcode_test: coded weights need a bf16 context and K %% 128 == 0");
    HIPCHK(c, hipSetDevice(c->device));
    const int npad = (N + 15) / 16 * 16;
    launch_pack_weight(c->cfg.dtype, W, packed_out, N, K, npad, nullptr, c->stream);
    // the encoder writes the dense words behind the header words: a buffer of both, of which hdr_out gets the first half
    DevBufs tmp;
    unsigned* words = (unsigned*)tmp.get(wc_hdr_words(npad) * sizeof(unsigned));
    if (!words) return fail(c, -2, "rdx_wcode_test: out of device memory");
    launch_encode_wc(packed_out, planes_out, words, npad, K, c->stream);
    HIPCHK(c, hipMemcpyAsync(hdr_out, words, (size_t)(npad / 16) * sizeof(unsigned), hipMemcpyDeviceToDevice, c->stream));
    return finish(c);
}

extern "C" int rdx_wcode_dense_test(rdx_ctx* c, const float* W, int N, int K, uint32_t* dense_host) {
    if (!c || !W || !dense_host || N <= 0 || K <= 0) return fail(c, -1, "rdx_wcode_dense_test: bad arguments");
    if (c->cfg.dtype != DT_BF16 || K % WC_CHUNK_K) return fail(c, -1, "rdx_wcode_dense_test: coded weights need a bf16 context and K %% 128 == 0");
    HIPCHK(c, hipSetDevice(c->device));
    const int npad = (N + 15) / 16 * 16, nt = npad / 16;
    DevBufs tmp;
    void* packed = tmp.get((size_t)npad * K * 2);
    void* planes = tmp.get(wc_bytes(npad, K));
    unsigned* words = (unsigned*)tmp.get(wc_hdr_words(npad) * sizeof(unsigned));
    if (!packed || !planes || !words) return fail(c, -2, "rdx_wcode_dense_test: out of device memory");
    launch_pack_weight(c->cfg.dtype, W, packed, N, K, npad, nullptr, c->stream);
    launch_encode_wc(packed, planes, words, npad, K, c->stream);
    if (int rc = finish(c)) return rc;
    HIPCHK(c, hipMemcpy(dense_host, words + nt, (size_t)nt * sizeof(unsigned), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int rdx_wcode_dense_words(rdx_ctx* c, int unit, int layer, uint32_t* words_host, int tiles, long long* dense_total) {
    if (!c || !c->finalized) return fail(c, -1, "rdx_wcode_dense_words: a finalized context is needed");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (dense_total) {
        *dense_total = 0;
        for (const StreamW& sw : stream_weights(c)) {
            const GemmW* W = sw.W;
            if (!W->wc || !W->wch) continue;
            const int nt = W->Npad / 16;
            std::vector<unsigned> d(nt);
            HIPCHK(c, hipMemcpy(d.data(), W->wch + nt, (size_t)nt * sizeof(unsigned), hipMemcpyDeviceToHost));
            for (unsigned v : d) *dense_total += v & 1u;
        }
    }
    if (!words_host) return 0;
    const GemmW* W = nullptr;
    if (unit == UNIT_LM_HEAD) W = &c->lm_head;
    else if (layer >= 0 && layer < (int)c->ll.size())
        W = unit == UNIT_QKV ? &c->ll[layer].wqkv : unit == UNIT_GATE_UP ? &c->ll[layer].wgu : unit == UNIT_DOWN ? &c->ll[layer].wdown : nullptr;
    if (!W || !W->wc || !W->wch) return fail(c, -1, "rdx_wcode_dense_words: unit %d of layer %d has no coded copy", unit, layer);
    if (tiles != W->Npad / 16) return fail(c, -1, "rdx_wcode_dense_words: the weight has %d tiles, not %d", W->Npad / 16, tiles);
    HIPCHK(c, hipMemcpy(words_host, W->wch, wc_hdr_words(W->Npad) * sizeof(unsigned), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int rdx_wcode_stats(rdx_ctx* c, long long* out) {
    if (!c || !out || !c->finalized) return fail(c, -1, "rdx_wcode_stats: a finalized context and an output are needed");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = 0;
    out[3] = c->n_stream[rdx_ctx::WK_GEMV][WS_CODED]; out[4] = c->n_stream[rdx_ctx::WK_CHAIN][WS_CODED];
    for (const StreamW& sw : stream_weights(c)) {
        const GemmW* W = sw.W;
        if (!W->wc || !W->wch) continue;
        const int nt = W->Npad / 16;
        std::vector<unsigned> h(nt);
        HIPCHK(c, hipMemcpy(h.data(), W->wch, (size_t)nt * sizeof(unsigned), hipMemcpyDeviceToHost));
        out[0] += nt;
        for (unsigned v : h) out[1] += (v >> 8) & 1u;
        out[2] += (long long)wc_bytes(W->Npad, W->K) + (long long)wc_hdr_words(W->Npad) * 4;
    }
    return 0;
}

extern "C" int rdx_w4_test(rdx_ctx* c, const float* W, int N, int K, void* wprime_out, void* stream_out, void* scales_out) {
    if (!c || !W || !wprime_out || !stream_out || !scales_out || N <= 0 || K <= 0) return fail(c, -1, "rdx_w4_test: bad arguments");
    if (c->cfg.dtype != DT_BF16 || K % W4_CHUNK_K) return fail(c, -8, "rdx_w4_test: int4 weights need a bf16 context and K %% 128 == 0");
    HIPCHK(c, hipSetDevice(c->device));
    const int npad = (N + 15) / 16 * 16;
    DevBufs b;
    char* tmp = (char*)b.get((size_t)(npad / 16) * sizeof(unsigned) + sizeof(int));        // header words + the quantiser's non-finite flag
    if (!tmp) return fail(c, -2, "rdx_w4_test: out of device memory");
    int* badf = (int*)(tmp + (size_t)(npad / 16) * sizeof(unsigned));
    hipMemsetAsync(badf, 0, sizeof(int), c->stream);
    launch_quant_w4(W, wprime_out, stream_out, (unsigned*)tmp, badf, N, K, npad, npad, npad, c->stream);
    // the scales as they stand in the stream: the 32 bytes behind every chunk's nibbles
    hipMemcpy2DAsync(scales_out, 32, (const char*)stream_out + 1024, W4_CHUNK_BYTES, 32, (size_t)(npad / 16) * (K / W4_CHUNK_K), hipMemcpyDeviceToDevice, c->stream);
    int bad = 0;
    hipMemcpyAsync(&bad, badf, sizeof(int), hipMemcpyDeviceToHost, c->stream);
    if (int rc = finish(c)) return rc;
    if (bad) return fail(c, -1, "rdx_w4_test: the weight holds an Inf or a NaN");
    return 0;
}

extern "C" int rdx_w4_rows_stats(rdx_ctx* c, long long out[2]) {
    if (!c || !out || !c->finalized) return fail(c, -1, "rdx_w4_rows_stats: a finalized context and an output are needed");
    out[0] = c->n_stream[rdx_ctx::WK_XSTAT16][WS_W4]; out[1] = c->n_stream[rdx_ctx::WK_XROW16][WS_W4];
    return 0;
}

extern "C" int rdx_w4_stats(rdx_ctx* c, long long* out) {
    if (!c || !out || !c->finalized) return fail(c, -1, "rdx_w4_stats: a finalized context and an output are needed");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = 0;
    out[3] = c->n_stream[rdx_ctx::WK_GEMV][WS_W4]; out[4] = c->n_stream[rdx_ctx::WK_CHAIN][WS_W4];
    for (const StreamW& sw : stream_weights(c)) {
        const GemmW* W = sw.W;
        if (!W->w4 || !W->w4h) continue;
        const int nt = W->Npad / 16;
        std::vector<unsigned> h(nt);
        HIPCHK(c, hipMemcpy(h.data(), W->w4h, (size_t)nt * sizeof(unsigned), hipMemcpyDeviceToHost));
        long long raw = 0;
        for (unsigned v : h) raw += (v >> 8) & 1u;
        out[0] += nt - raw; out[1] += raw;
        out[2] += (long long)w4_bytes(W->Npad, W->K) + (long long)nt * 4;
    }
    return 0;
}
