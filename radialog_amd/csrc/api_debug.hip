// librdx_hooks.so, first unit: kernel-test, trace and microbenchmark hooks (include/rdx_hooks.h, and the encoder's: include/rdx_enc_hooks.h) -- NOT part of the product
// library. Linked against librdx.so, whose context and launchers it drives; radialog_amd/_lib.py loads it only under RDX_DEBUG_HOOKS=1 (the tests' conftest and the
// tools/ scripts set it). The product entry points, rdx_time included, are in librdx.so (include/rdx.h). Device temporaries, event pairs and borrowed context fields
// are scoped (hook_util.h: no hook frees or restores by hand), and every hook that launches ends in finish().
#include "hook_util.h"
#include "../../include/rdx_hooks.h"
#include "../../include/rdx_enc_hooks.h"

// Debug: the stand-alone decode-attention kernel of layer `layer` at the current state, 8 timestamps of workgroup (0,0):
// host[0..6] = after slot load, inputs ready, new token done, barrier 1, scores + barrier, softmax, PV + barrier; [7] = entry.
extern "C" int rdx_attn_trace(rdx_ctx* c, int layer, long long* host) {
    if (!c || !c->finalized || c->cur_B <= 0 || !host) return fail(c, -1, "rdx_attn_trace: run a prefill first");
    HIPCHK(c, hipSetDevice(c->device));
    DevBufs b;
    long long* dtr = (long long*)b.get(8 * sizeof(long long));
    if (!dtr) return fail(c, -2, "rdx_attn_trace: out of device memory");
    HIPCHK(c, hipMemsetAsync(dtr, 0, 8 * sizeof(long long), c->stream));
    DecAttnArgs at = dec_attn_args(c, layer);
    at.trace = dtr;
    run_decode_attention(c, at, layer, c->cur_B);
    if (int rc = finish(c)) return rc;
    HIPCHK(c, hipMemcpy(host, dtr, 8 * sizeof(long long), hipMemcpyDeviceToHost));
    return 0;
}

// Test hook: the fp8 path's activation quantisers on caller data. mode 0 = quant_rows_k (rows of X [M][K] -> e4m3 bytes [M][K] + scales [M][groups]),
// mode 1 = RMSNorm -> e4m3 (ACT_ROWS_E4M3: bytes [M][K] + one scale per row; norm_w [K] in the model dtype, groups ignored).
extern "C" int rdx_quant_test(rdx_ctx* c, const void* X, int M, int K, int groups, int mode, const void* norm_w, float eps, void* out8, float* scales) {
    if (!c || !X || !out8 || !scales || M <= 0 || K <= 0 || K % 128) return fail(c, -1, "rdx_quant_test: bad arguments (K %% 128 == 0)");
    if (mode == 0 && (groups < 1 || groups > 4)) return fail(c, -1, "rdx_quant_test: 1..4 K groups");
    if (mode == 1 && !norm_w) return fail(c, -1, "rdx_quant_test: mode 1 needs the norm weight");
    HIPCHK(c, hipSetDevice(c->device));
    if (mode == 0) launch_quant_rows(c->cfg.dtype, X, K, out8, scales, M, K, groups, c->stream);
    else run_rmsnorm(c, NormArgs{const_cast<void*>(X), norm_w, out8, scales, M, K, eps, ACT_ROWS_E4M3, 0, nullptr, 0});
    return finish(c);
}

// Debug: one stand-alone decode GEMV (what = 1 gate/up, 2 qkv, 4 down, as in rdx_time) of `layer` with per-workgroup
// timestamps: host[tile*8 + {0 entry, 1 weights issued, 2 activations staged, 3 K loop done, 4 all waves done, 5 end}].
// what = 7: the chained down(layer) -> QKV(layer + 1) launch IN SITU (its hand-off counters are only valid inside a real step): ONE eager
// decode step runs and advances the state; host[workgroup*8 + slot] with the slots of chain.hip (chain_tile; down_proj workgroups first, then the QKV workgroups).
// what = 8: the fused attention + o_proj launch of `layer` IN SITU, the same way: the heads * B attention workgroups first ([0] entry, [1] qkv row loaded,
// [2] scores done, [3] softmax done, [4] P.V reduced, [5] output stored (stores issued), [6] arrival), then the o_proj workgroups (chain_tile's slots:
// [0] entry, [5] first weight KiB back, [3] inputs ready, [6] first MFMA, [1] K loop done, [7] end).
extern "C" int rdx_gemv_trace(rdx_ctx* c, int what, int layer, long long* host, int max_tiles) {
    if (!c || !c->finalized || c->cur_B <= 0 || !host) return fail(c, -1, "rdx_gemv_trace: run a prefill first");
    HIPCHK(c, hipSetDevice(c->device));
    const rdx_config& f = c->cfg;
    const int H = f.hidden, B = c->cur_B;
    const bool in_situ = what == 7 || what == 8;
    if (in_situ) {
        if (layer < 0 || layer >= f.layers) return fail(c, -1, "rdx_gemv_trace(%d): layer %d of %d", what, layer, f.layers);
        if (c->cur_T + c->cur_steps + 1 > f.max_len || c->cur_T + c->cur_steps + 1 > f.max_pos)       // as rdx_time(7): bounded by the KV cache, not by max_new
            return fail(c, -1, "rdx_gemv_trace(%d): no room for one more decode step in the KV cache", what);
        const bool fused = c->sw.fuse_ao && attn_oproj16_supported(c->ld, c->ll[layer].wo.N, c->ll[layer].wo.K, B);
        if (what == 8 && !fused)
            return fail(c, -1, "rdx_gemv_trace(8): the fused attention + o_proj launch is not active in this configuration (batch > 2, RDX_FUSE_AO=0)");
        const int wgs = what == 7 ? H / 16 + ((c->ll[0].wqkv.Npad + 15) / 16 + 3) / 4      // down_proj tiles + QKV workgroups of 4 tiles
                                  : f.heads * B + ((c->ll[layer].wo.N + 15) / 16 + 1) / 2;  // attention workgroups + o_proj workgroups of 2 tiles
        if (wgs > max_tiles) return fail(c, -1, "rdx_gemv_trace(%d): need room for %d workgroups", what, wgs);
    }
    DevBufs b;
    const size_t bytes = (size_t)max_tiles * 8 * sizeof(long long);
    long long* dtr = (long long*)b.get(bytes);
    if (!dtr) return fail(c, -2, "rdx_gemv_trace: out of device memory");
    HIPCHK(c, hipMemsetAsync(dtr, 0, bytes, c->stream));
    bool chained = true;
    if (in_situ) {
        if (what == 7) { c->chain_trace = dtr; c->chain_trace_layer = layer; }
        else { c->ao_trace = dtr; c->ao_trace_layer = layer; }
        chained = decode_step_launch(c, nullptr, nullptr, 0);
        c->chain_trace = nullptr; c->chain_trace_layer = -1;
        c->ao_trace = nullptr; c->ao_trace_layer = -1;
        c->cur_steps = std::max(c->cur_steps + 1, c->cur_max_new);      // the state has moved: a new prefill comes first
    } else {
        const LlamaLayer& L = c->ll[layer];
        const DecUnit u = what == 1 ? UNIT_GATE_UP : what == 2 ? UNIT_QKV : UNIT_DOWN;
        GemmArgs a = decode_family(c, B) == DEC_CHAINED ? chained_unit(c, &L, u, B) : unit_args(c, &L, u, B);      // the step's builder: with the copy the chained family streams
        if (what != 1 && what != 2) { a.out = c->dqkv; a.resid = nullptr; a.ldr = 0; }      // down_proj alone: into a scratch buffer, no residual (dx stays as it is)
        if ((a.N + 15) / 16 > max_tiles) return fail(c, -1, "rdx_gemv_trace: need room for %d tiles", (a.N + 15) / 16);
        a.trace = dtr;
        skinny(c, a, what == 1 ? EPI_SILU_MUL : EPI_NONE);
    }
    if (int rc = finish(c)) return rc;
    HIPCHK(c, hipMemcpy(host, dtr, bytes, hipMemcpyDeviceToHost));
    if (what == 7 && !chained) return fail(c, -1, "rdx_gemv_trace(7): the chained down -> QKV launch is not active in this configuration (batch > 2, RDX_CHAIN=0)");
    return 0;
}

// Kernel benchmark hook: `iters` launches of one GEMM (ksize = 0: out[M][N] = epi(X[M][K] W^T), M = rows) or one NHWC convolution
// (ksize = 1 / 3: batch `rows` images of H x H x K channels -> N channels, `stride`, pad = ksize / 2) through the SAME dispatch
// the encoder / prefill use (run_gemm / conv_gemm), timed with HIP events on the context's stream. Contents are zeros; epi 3 / 6
// read a residual. Returns ms per launch.
extern "C" int rdx_kernel_bench(rdx_ctx* c, int rows, int N, int K, int H, int ksize, int stride, int epi, int iters, float* ms_host,
                                long long* trace_host, int trace_wgs) {
    if (!c || !ms_host || iters <= 0 || rows <= 0) return fail(c, -1, "rdx_kernel_bench: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const int Kg = ksize ? ksize * ksize * K : K;
    if (Kg % 32 || N % 16) return fail(c, -1, "rdx_kernel_bench: need K %% 32 == 0 and N %% 16 == 0");
    const int Ho = ksize ? (H + 2 * (ksize / 2) - ksize) / stride + 1 : 0;
    const size_t M = ksize ? (size_t)rows * Ho * Ho : (size_t)rows, Min = ksize ? (size_t)rows * H * H : (size_t)rows;
    const bool kb_wstat = getenv("RDX_KB_WSTAT") && atoi(getenv("RDX_KB_WSTAT")) && !ksize;
    const size_t xb = ((Min + 15) & ~(size_t)15) * K * 2 + 64, wb = (size_t)N * Kg * 2, ob = M * N * 2 + 64, bb = (size_t)N * 4;
    DevBufs b;
    char* buf = (char*)b.get(xb + wb + 2 * ob + bb);
    long long* dtr = trace_host && trace_wgs > 0 ? (long long*)b.get((size_t)trace_wgs * 64) : nullptr;
    if (!buf || (trace_host && trace_wgs > 0 && !dtr)) return fail(c, -2, "rdx_kernel_bench: out of device memory");
    HIPCHK(c, hipMemsetAsync(buf, 0, xb + wb + 2 * ob + bb, c->stream));
    if (dtr) HIPCHK(c, hipMemset(dtr, 0, (size_t)trace_wgs * 64));
    GemmW w; w.N = N; w.K = Kg; w.Npad = N; w.w = buf + xb;
    void *out = buf + xb + wb, *res = buf + xb + wb + ob;
    const float* bias = (const float*)(buf + xb + wb + 2 * ob);
    const bool need_res = epi == EPI_RESID || epi == EPI_RESID_RELU;
    EventPair ev;
    Scoped<bool> ws(c->ws_ok, true);
    auto once = [&]() {
        if (ksize) conv_gemm(c, buf, w, bias, need_res ? res : nullptr, out, rows, H, H, K, ksize, ksize, stride, ksize / 2, Ho, Ho, epi);
        else {
            GemmArgs a = gargs(buf, K, w, bias, out, N, (int)M); a.resid = need_res ? res : nullptr; a.ldr = N; a.trace = dtr;
            if (kb_wstat) {       // RDX_KB_WSTAT=1: the single prompt's weight-stationary kernel on (zero) fragment-packed activations
                a.xpacked = ACT_TILES32; a.mtiles = (int)((M + 15) / 16); a.bias = nullptr;
                if (wstat_supported(a, epi)) { launch_wstat(c->cfg.dtype, a, epi, c->stream); return; }
            }
            run_gemm(c, a, epi);
        }
    };
    once();
    HIPCHK(c, ev.start(c->stream));
    for (int i = 0; i < iters; ++i) once();
    float ms = 0.f;
    HIPCHK(c, ev.stop(c->stream, &ms));
    if (int rc = finish(c)) return rc;
    if (dtr) HIPCHK(c, hipMemcpy(trace_host, dtr, (size_t)trace_wgs * 64, hipMemcpyDeviceToHost));
    *ms_host = ms / (float)iters;
    return 0;
}

// One NHWC convolution on caller data through (path 0) the production dispatch of the row-major encoder path (conv_gemm) or (path 1) the
// fragment-packed kernel family pconv_k (pack_rows -> pconv -> unpack_rows; path 2: pconv writing row-major itself). X [B][H][H][Cin] and resid /
// out [B][Ho][Ho][Cout] model dtype, W [Cout][ksize * ksize * Cin] fp32 in the (kh, kw, c) K order, bias fp32. ms_host (nullable) = ms per launch
// of the convolution kernel alone over `iters` launches (layout conversions excluded).
extern "C" int rdx_conv_test(rdx_ctx* c, const void* X, const float* W, const float* bias, const void* resid, void* out, int B, int H, int Cin,
                             int Cout, int ksize, int stride, int epi, int path, int iters, float* ms_host) {
    if (!c || !X || !W || !out || B <= 0) return fail(c, -1, "rdx_conv_test: bad arguments");
    if (!(ksize == 1 || ksize == 3)) return fail(c, -1, "rdx_conv_test: ksize 1 or 3");
    HIPCHK(c, hipSetDevice(c->device));
    const int K = ksize * ksize * Cin, Ho = (H + 2 * (ksize / 2) - ksize) / stride + 1;
    const int M = B * Ho * Ho, Min = B * H * H, dt = c->cfg.dtype;
    if (K % 32 || Cout % 16) return fail(c, -1, "rdx_conv_test: need K %% 32 == 0 and Cout %% 16 == 0");
    const bool need_res = epi == EPI_RESID || epi == EPI_RESID_RELU;
    if (need_res && !resid) return fail(c, -1, "rdx_conv_test: epilogue needs a residual");
    const int mt_in = (Min + 15) / 16, mt_out = (M + 15) / 16;
    const size_t wb = (size_t)Cout * K * 2, xpb = (size_t)mt_in * 16 * Cin * 2, opb = (size_t)mt_out * 16 * Cout * 2;
    DevBufs b;
    char* buf = (char*)b.get(wb + xpb + 2 * opb + 256);
    if (!buf) return fail(c, -2, "rdx_conv_test: out of device memory");
    GemmW w; w.N = Cout; w.K = K; w.Npad = Cout; w.w = buf;
    pack_w(c, W, w);
    char *xp = buf + wb, *rp = xp + xpb, *op = rp + opb;
    Scoped<bool> ws(c->ws_ok, true);
    PConvArgs pa;
    memset(&pa, 0, sizeof(pa));
    if (path) {
        launch_pack_rows(dt, X, Cin, xp, Min, Cin, c->stream);
        if (need_res) launch_pack_rows(dt, resid, Cout, rp, M, Cout, c->stream);
        pa.X = xp; pa.W = buf; pa.bias = bias; pa.resid = need_res ? rp : nullptr; pa.out = path == 2 ? out : (void*)op; pa.zero16 = c->zero16;
        pa.Hin = H; pa.Win = H; pa.Cin = Cin; pa.Hout = Ho; pa.Wout = Ho; pa.N = Cout; pa.M = M; pa.mt_in = mt_in; pa.mt_out = mt_out; pa.ldo = Cout;
        pa.no_ksplit = !c->sw.pconv_ksplit;
        if (const char* e = getenv("RDX_PCONV_TILE")) {            // "MxN" or "MxNkS": forced register tile (tools/pconv_check.py)
            if (e[0] >= '1' && e[0] <= '8' && e[1] == 'x' && (e[2] == '2' || e[2] == '4')) {
                pa.tile_m = e[0] - '0'; pa.tile_n = e[2] - '0';
                if (e[3] == 'k' && (e[4] == '4' || e[4] == '8')) pa.tile_k = e[4] - '0';
            }
        }
        if (!c->zero16 || !pconv_supported(pa, ksize * ksize, stride, epi)) return fail(c, -1, "rdx_conv_test: shape not supported by pconv");
    }
    bool refused = false;
    auto once = [&]() {
        if (path) { if (!launch_pconv(dt, pa, ksize * ksize, stride, epi, path == 2, c->stream)) refused = true; }
        else conv_gemm(c, X, w, bias, need_res ? resid : nullptr, out, B, H, H, Cin, ksize, ksize, stride, ksize / 2, Ho, Ho, epi);
    };
    once();
    if (refused) return fail(c, -1, "rdx_conv_test: pconv refused the tiling (1 x 1 stride-1 with different input / output row tilings)");
    if (ms_host && iters > 0) {
        EventPair ev;
        HIPCHK(c, ev.start(c->stream));
        for (int i = 0; i < iters; ++i) once();
        float ms = 0.f;
        HIPCHK(c, ev.stop(c->stream, &ms));
        *ms_host = ms / (float)iters;
    }
    if (path == 1) launch_unpack_rows(dt, op, out, Cout, M, Cout, c->stream);
    return finish(c);
}

// Microbenchmark: GB/s that `wgs` workgroups (256 threads) pull from a cache-resident buffer, `bytes_per_wg` each (shared = 1: all
// read the same region), read `reps` times; mode 0 = global_load_dwordx4, 1 = global_load_lds_dwordx4. Returns the aggregate GB/s.
extern "C" int rdx_l2_bench(rdx_ctx* c, int mode, long long bytes_per_wg, int shared, int reps, int wgs, float* gbps_host) {
    if (!c || !gbps_host || bytes_per_wg < 65536 || wgs <= 0 || reps <= 0) return fail(c, -1, "rdx_l2_bench: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t total = shared ? (size_t)bytes_per_wg : (size_t)bytes_per_wg * wgs;
    DevBufs b;
    char* buf = (char*)b.get(total + 64);
    if (!buf) return fail(c, -2, "rdx_l2_bench: out of device memory");
    HIPCHK(c, hipMemsetAsync(buf, 1, total + 64, c->stream));
    EventPair ev;
    launch_l2_bench(mode, buf, (size_t)bytes_per_wg, shared, 1, wgs, (unsigned*)(buf + total), c->stream);        // warm the caches
    HIPCHK(c, ev.start(c->stream));
    launch_l2_bench(mode, buf, (size_t)bytes_per_wg, shared, reps, wgs, (unsigned*)(buf + total), c->stream);
    float ms = 0.f;
    HIPCHK(c, ev.stop(c->stream, &ms));
    if (int rc = finish(c)) return rc;
    *gbps_host = (float)((double)bytes_per_wg * wgs * reps / (ms * 1e-3) / 1e9);
    return 0;
}

namespace {

// fp8 weights at batch >= 3 multiply fp8 x fp8 (xstat32_k<W8, A8>): [RMSNorm +] e4m3 quantisation of the rows into the 32-row fragment block,
// like skinny_prenorm does in the decode step; the block and its 32 scales are one temporary of the call
int fp8_block_for_test(rdx_ctx* c, DevBufs& b, GemmArgs& a, int epi) {
    if (!(a.W8 && a.wscale) || a.M < xs_min_rows()) return 0;
    GemmArgs t = a; t.norm_w = nullptr;
    if (!xstat32_supported(t, epi)) return 0;
    char* blk = (char*)b.get((size_t)32 * a.K + 32 * sizeof(float));
    if (!blk) return fail(c, -2, "fp8 activation block: out of device memory");
    float* xs = (float*)(blk + (size_t)32 * a.K);
    run_rmsnorm(c, NormArgs{const_cast<void*>(a.X), a.norm_w, blk, xs, a.M, a.K, a.eps, ACT_BLK64_E4M3, 0, nullptr, 0});
    a.X = blk; a.ldx = a.K; a.xpacked = ACT_BLK64_E4M3; a.xscale = xs; a.xgroups = 1; a.norm_w = nullptr;
    return 0;
}

struct GemmCall {       // one rdx_gemm_test call: its arguments, its device temporaries, and the weight in the form its kernel family streams
    rdx_ctx* c; const void* X; const float* W; const float* bias; const void* resid; void* out; int M, N, K, epi; const void* norm_w; float eps;
    GemmW w;            // N, K, Npad (whole 16-row tiles: zero rows, as the engine's loader pads them) from the entry point; the pointers from packed() / fp8() / quant_w4_for_test()
    DevBufs b;
    int bad_shape() const { return fail(c, -1, "rdx_gemm_test: need K %% 32 == 0 and N %% 16 == 0"); }
    int oom() const { return fail(c, -2, "rdx_gemm_test: out of device memory"); }
    // W in the model dtype, packed. false: out of device memory
    bool packed() {
        if ((w.w = b.get((size_t)w.Npad * K * 2))) pack_w(c, W, w);
        return w.w != nullptr;
    }
    // W as the fp8 engine holds it (N % 16 == 0): e4m3 bytes + scales only, in one block behind the room of the model-dtype copy it does not have
    bool fp8() {
        char* blk = (char*)b.get((size_t)N * K * 3 + (size_t)N * 4);
        if (!blk) return false;
        w.w8 = blk + (size_t)N * K * 2; w.scale = (float*)(blk + (size_t)N * K * 3);
        pack_w8(c, W, w);
        return true;
    }
    GemmArgs args() const {       // row-major X, the RMSNorm (norm_w) as the kernel's prologue
        GemmArgs a = with_switches(c, gargs(X, K, w, bias, out, epi == EPI_SILU_MUL ? N / 2 : N, M));
        a.resid = resid; a.ldr = N; a.norm_w = norm_w; a.eps = eps;
        return a;
    }
};

// ---- runners: a kernel family on the weight form its caller prepared ----

// skinny(), as the decode step calls it: the weight-streaming GEMV, from 3 rows the 32-row kernels
int run_skinny(GemmCall& g, GemmArgs a) {
    rdx_ctx* c = g.c;
    if (g.M > 32) return fail(c, -1, "rdx_gemm_test: skinny path needs M <= 32");
    if (int rc = fp8_block_for_test(c, g.b, a, g.epi)) return rc;
    // skinny() pre-normalises into c->dxn when the rows do not fit the LDS: a test engine has no decoder, so the buffer is the call's
    const bool prenorm = a.norm_w && !skinny_fits_lds(g.M, g.K);
    void* xn = prenorm ? g.b.get((size_t)32 * g.K * 2) : c->dxn;
    if (prenorm && !xn) return g.oom();
    Scoped<void*> dxn(c->dxn, xn);
    skinny(c, a, g.epi == EPI_RESID_RELU ? EPI_RESID : g.epi);
    return finish(c);
}

// the K-split slab path: pack X -> xsplit32_k -> slab combine (+ residual) at the launch boundary; out = resid + X W^T
int run_ksplit(GemmCall& g) {
    rdx_ctx* c = g.c;
    if (g.epi != EPI_RESID || !g.resid || g.M <= 16 || g.M > 32) return fail(c, -1, "rdx_gemm_test: force 5 needs epi 3 and 16 < M <= 32");
    const size_t xb = (size_t)32 * g.K * 2, sb = (size_t)4 * 32 * g.N * 4;
    char* tmp = (char*)g.b.get(2 * xb + sb);       // the packed rows, the combine's packed output (unused), the slabs
    if (!tmp) return g.oom();
    float* slab = (float*)(tmp + 2 * xb);
    GemmArgs a = g.args();
    a.X = tmp; a.xpacked = g.w.w8 ? ACT_BLK64 : ACT_BLK32; a.norm_w = nullptr;
    run_rmsnorm(c, NormArgs{const_cast<void*>(g.X), nullptr, tmp, nullptr, g.M, g.K, g.eps, a.xpacked, 0, nullptr, 0});   // w = null: re-layout only
    const int kg = xsplit32_groups(a);
    if (!kg) return fail(c, -1, "rdx_gemm_test: shape not supported by xsplit32_k");
    launch_xsplit32(c->cfg.dtype, a, slab, c->stream);
    HIPCHK(c, hipMemcpyAsync(g.out, g.resid, (size_t)g.M * g.N * 2, hipMemcpyDeviceToDevice, c->stream));
    run_rmsnorm(c, NormArgs{g.out, nullptr, tmp + xb, nullptr, g.M, g.N, g.eps, ACT_ROWS, 0, slab, kg});
    return finish(c);
}

// ---- one function per kernel family: its preconditions (any N > 0 unless it asks for whole tiles), the weight, the activations, the production predicate, the launch ----

int gemm_skinny(GemmCall& g, bool fp8) {
    if (fp8 && g.N % 16) return g.bad_shape();
    if (fp8 && g.K % 64) return fail(g.c, -1, "rdx_gemm_test: fp8 needs K %% 64 == 0");
    if (!(fp8 ? g.fp8() : g.packed())) return g.oom();
    return run_skinny(g, g.args());
}

int gemm_ksplit(GemmCall& g, bool fp8) {
    if (g.N % 16) return g.bad_shape();
    if (fp8 && g.K % 64) return fail(g.c, -1, "rdx_gemm_test: fp8 needs K %% 64 == 0");
    if (!(fp8 ? g.fp8() : g.packed())) return g.oom();
    return run_ksplit(g);
}

// the GEMV on the coded copy of the packed weight
int gemm_skinny_coded(GemmCall& g) {
    rdx_ctx* c = g.c;
    if (c->cfg.dtype != DT_BF16 || g.K % WC_CHUNK_K || g.M >= xs_min_rows() || !skinny_fits_lds(g.M, g.K))
        return fail(c, -1, "rdx_gemm_test: force 12 (coded bf16 weights) needs a bf16 context, K %% 128 == 0 and M <= 2 rows that fit the GEMV's LDS stage");
    void* planes = g.packed() ? g.b.get(wc_bytes(g.w.Npad, g.K)) : nullptr;
    unsigned* hdr = planes ? (unsigned*)g.b.get(wc_hdr_words(g.w.Npad) * sizeof(unsigned)) : nullptr;
    if (!hdr) return g.oom();
    GemmArgs a = g.args();
    code_w(c, g.w, planes, hdr, a);
    // the epilogue as given: what is not a coded epilogue (6, relu(+resid), among them) is refused, not mapped onto one that is
    if (g.epi == EPI_LOGITS || !skinny_wc_supported(c->cfg.dtype, a, g.epi)) return fail(c, -1, "rdx_gemm_test: force 12: no coded GEMV for epilogue %d", g.epi);
    return run_skinny(g, a);
}

// the GEMV on the int4 stream; raw_tile: the tile of rows 16..31 stays raw and streams its packed bf16 bytes
int gemm_skinny_w4(GemmCall& g, bool raw_tile) {
    rdx_ctx* c = g.c;
    if (c->cfg.dtype != DT_BF16 || g.K % W4_CHUNK_K || g.M >= xs_min_rows() || !skinny_fits_lds(g.M, g.K) || (raw_tile && g.N < 48))
        return fail(c, -1, "rdx_gemm_test: force 13 / 14 (int4 weights) needs a bf16 context, K %% 128 == 0 and M <= 2 rows that fit the GEMV's LDS stage (14: N >= 48)");
    if (int rc = quant_w4_for_test(c, g.b, g.W, g.w, raw_tile ? 16 : g.w.Npad, raw_tile ? 32 : g.w.Npad))
        return rc == -2 ? g.oom() : fail(c, -1, "rdx_gemm_test: the weight holds an Inf or a NaN");
    GemmArgs a = g.args();
    a.W4 = g.w.w4; a.w4hdr = g.w.w4h;
    if (!skinny_w4_supported(c->cfg.dtype, a, g.epi))
        return fail(c, -1, "rdx_gemm_test: force %d: no int4 GEMV for epilogue %d", raw_tile ? RDX_GEMM_SKINNY_W4_RAW : RDX_GEMM_SKINNY_W4, g.epi);
    return run_skinny(g, a);
}

// many rows: gemm_dma_k where it takes the shape (try_dma), else tiled_gemm_k (may_tile); the RMSNorm is a launch of its own in front
int gemm_rows(GemmCall& g, bool try_dma, bool may_tile) {
    rdx_ctx* c = g.c;
    if (g.N % 16) return g.bad_shape();
    void* xn = g.packed() && g.norm_w ? g.b.get((size_t)g.M * g.K * 2) : nullptr;
    if (!g.w.w || (g.norm_w && !xn)) return g.oom();
    GemmArgs a = g.args();
    if (g.norm_w) {
        run_rmsnorm(c, NormArgs{const_cast<void*>(g.X), g.norm_w, xn, nullptr, g.M, g.K, g.eps, ACT_ROWS, 0, nullptr, 0});
        a.X = xn; a.norm_w = nullptr;
    }
    if (try_dma && gemm_dma_supported(a)) launch_gemm_dma(c->cfg.dtype, a, g.epi, c->gemm_ws, c->gemm_ws_floats, c->stream);
    else if (!may_tile) return fail(c, -1, "rdx_gemm_test: shape not supported by gemm_dma_k");
    else launch_tiled_gemm(c->cfg.dtype, a, ConvGeom{}, g.epi, c->stream);
    return finish(c);
}

// the encoder's many-row kernel (wsgemm.hip), tile shape by the context's switch "ws_cfg"
int gemm_wsgemm(GemmCall& g) {
    rdx_ctx* c = g.c;
    if (g.N % 16) return g.bad_shape();
    if (!c->zero16 || g.K % 64) return fail(c, -1, "rdx_gemm_test: shape not supported by wsgemm_k");
    if (!g.packed()) return g.oom();
    GemmArgs a = g.args();
    a.norm_w = nullptr;
    launch_wsgemm(c->cfg.dtype, a, ConvGeom{}, g.epi, c->zero16, c->sw.ws_cfg, c->stream);
    return finish(c);
}

// the single prompt's weight-stationary kernel (wstat.hip): RMSNorm / re-layout into the fragment-packed order, then the GEMM
int gemm_wstat(GemmCall& g) {
    rdx_ctx* c = g.c;
    if (g.N % 16) return g.bad_shape();
    const int mtl = (g.M + 15) / 16;
    void* xt = g.packed() ? g.b.get((size_t)mtl * 16 * g.K * 2) : nullptr;
    if (!xt) return g.oom();
    run_rmsnorm(c, NormArgs{const_cast<void*>(g.X), g.norm_w, xt, nullptr, g.M, g.K, g.eps, ACT_TILES32, mtl, nullptr, 0});        // norm_w == null: re-layout only
    GemmArgs a = g.args();
    a.X = xt; a.xpacked = ACT_TILES32; a.mtiles = mtl; a.norm_w = nullptr;
    if (!wstat_supported(a, g.epi)) return fail(c, -1, "rdx_gemm_test: shape not supported by wstat_k");
    launch_wstat(c->cfg.dtype, a, g.epi, c->stream);
    return finish(c);
}

// the fp8 path's prefill GEMM (gemm8.hip): e4m3 weights x e4m3 activations with G K groups; RMSNorm -> fp8 (one group) or quant_rows_k
int gemm_gemm8(GemmCall& g, int G) {
    rdx_ctx* c = g.c;
    if (g.N % 16) return g.bad_shape();
    if (g.K % 64 || (g.norm_w && G != 1)) return fail(c, -1, "rdx_gemm_test: gemm8 needs K %% 64 == 0 (and one K group behind an RMSNorm)");
    char* x8 = g.fp8() ? (char*)g.b.get((size_t)g.M * g.K + (size_t)g.M * 4 * sizeof(float)) : nullptr;
    if (!x8) return g.oom();
    float* xs = (float*)(x8 + (size_t)g.M * g.K);
    if (g.norm_w) run_rmsnorm(c, NormArgs{const_cast<void*>(g.X), g.norm_w, x8, xs, g.M, g.K, g.eps, ACT_ROWS_E4M3, 0, nullptr, 0});
    else launch_quant_rows(c->cfg.dtype, g.X, g.K, x8, xs, g.M, g.K, G, c->stream);
    GemmArgs a = gargs(x8, g.K, g.w, nullptr, g.out, g.epi == EPI_SILU_MUL ? g.N / 2 : g.N, g.M);      // no bias, the norm already applied
    a.resid = g.resid; a.ldr = g.N; a.xscale = xs; a.xgroups = G;
    if (!gemm8_supported(a, g.epi)) return fail(c, -1, "rdx_gemm_test: shape / epilogue not supported by gemm8");
    launch_gemm8(c->cfg.dtype, a, g.epi, c->stream);
    return finish(c);
}

}  // namespace

// One bare GEMM through the production kernels (unit tests / kernel benchmarks): out = epilogue(X . W^T).
// X, resid, norm_w, out are model-dtype device tensors; W [N][K] and bias [N] are fp32 device tensors (W is prepared here, in the form the family `force` names streams).
extern "C" int rdx_gemm_test(rdx_ctx* c, const void* X, const float* W, const float* bias, const void* resid, void* out,
                             int M, int N, int K, int epi, const void* norm_w, float eps, int force) {
    if (!c || !X || !W || !out) return fail(c, -1, "rdx_gemm_test: null argument");
    GemmCall g{c, X, W, bias, resid, out, M, N, K, epi, norm_w, eps};
    if (K % 32 || N <= 0) return g.bad_shape();
    g.w.N = N; g.w.K = K; g.w.Npad = (N + 15) / 16 * 16;
    HIPCHK(c, hipSetDevice(c->device));
    switch (force) {
    case RDX_GEMM_DISPATCH: return N % 16 ? g.bad_shape() : M <= 32 ? gemm_skinny(g, false) : gemm_rows(g, true, true);
    case RDX_GEMM_SKINNY: return gemm_skinny(g, false);
    case RDX_GEMM_LDS_DMA: return gemm_rows(g, true, false);
    case RDX_GEMM_SKINNY_FP8: return gemm_skinny(g, true);
    case RDX_GEMM_KSPLIT: return gemm_ksplit(g, false);
    case RDX_GEMM_KSPLIT_FP8: return gemm_ksplit(g, true);
    case RDX_GEMM_WSGEMM: return gemm_wsgemm(g);
    case RDX_GEMM_WSTAT: return gemm_wstat(g);
    case RDX_GEMM_GEMM8_G1: return gemm_gemm8(g, 1);
    case RDX_GEMM_GEMM8_G2: return gemm_gemm8(g, 2);
    case RDX_GEMM_GEMM8_G4: return gemm_gemm8(g, 4);
    case RDX_GEMM_SKINNY_CODED: return gemm_skinny_coded(g);
    case RDX_GEMM_SKINNY_W4: return gemm_skinny_w4(g, false);
    case RDX_GEMM_SKINNY_W4_RAW: return gemm_skinny_w4(g, true);
    case RDX_GEMM_TILED: default: return gemm_rows(g, false, true);      // a code outside the enum has always run the tiled kernel
    }
}

// the lm_head epilogue (logits + per-tile argmax partials) of the weight-streaming kernels on a bare GEMM: what the decode
// step runs before greedy_step_k; the partials are reduced here on the host with the same tie rule (lowest index)
extern "C" int rdx_logits_test(rdx_ctx* c, const void* X, const float* W, int M, int N, int n_valid, int K, void* out_logits,
                               int32_t* argmax_host, int fp8) {
    if (!c || !X || !W || !out_logits || !argmax_host) return fail(c, -1, "rdx_logits_test: null argument");
    const bool coded = fp8 == 2;          // 2: the GEMV on the coded bf16 copy of W (as rdx_gemm_test force 12)
    if (coded) fp8 = 0;
    if (K % 32 || N % 16 || M > 32 || n_valid > N || (fp8 && K % 64)) return fail(c, -1, "rdx_logits_test: bad shape");
    if (coded && (c->cfg.dtype != DT_BF16 || K % WC_CHUNK_K || M >= xs_min_rows() || !skinny_fits_lds(M, K)))
        return fail(c, -1, "rdx_logits_test: coded bf16 weights need a bf16 context, K %% 128 == 0 and M <= 2 rows that fit the GEMV's LDS stage");
    HIPCHK(c, hipSetDevice(c->device));
    GemmW w;
    w.N = N; w.K = K; w.Npad = N;
    const int nt = N / 16;
    // one block: the packed weight; qb: the fp8 copy and its scales, or the coded copy's planes (16-byte aligned behind wb) and header words; the partials; slack
    const size_t cpb = coded ? wc_bytes(N, K) : 0;
    const size_t wb = (size_t)N * K * 2, qb = fp8 ? (size_t)N * K + (size_t)N * 4 : cpb + (coded ? wc_hdr_words(N) * 4 : 0), pb = (size_t)M * nt * 4;
    DevBufs b;
    char* wp = (char*)b.get(wb + qb + 2 * pb + (size_t)M * K * 2);
    if (!wp) return fail(c, -2, "rdx_logits_test: out of device memory");
    if (fp8) {
        w.w8 = wp + wb; w.scale = (float*)(wp + wb + (size_t)N * K);
        pack_w8(c, W, w);
    } else {
        w.w = wp;
        pack_w(c, W, w);
    }
    GemmArgs a = gargs(X, K, w, nullptr, out_logits, N, M);
    a.n_valid = n_valid;
    a.part_val = (float*)(wp + wb + qb); a.part_idx = (int*)(wp + wb + qb + pb);
    if (coded) code_w(c, w, wp + wb, (unsigned*)(wp + wb + cpb), a);
    if (int rc = fp8_block_for_test(c, b, a, EPI_LOGITS)) return rc;
    skinny(c, a, EPI_LOGITS);
    if (int rc = finish(c)) return rc;
    return reduce_partials(c, a, argmax_host);
}

// The image encoder's stem on caller data: img_prep_k, then (path 0) stem_pool_k row-major, (1) stem_pool_k fragment-packed with the encoder's
// pad-row zeroing (run_stem_pool), unpacked here, or (2) the two-kernel path conv_gemm + maxpool_k. image fp32 [B][3][S][S]; W fp32 [stem][224] in
// the (kh, kw 0..7, c 0..3) K order rdx_set_weight("v.conv1.w") takes, packed here as it packs it; out [B][S / 4][S / 4][stem] model dtype.
// Path 1 also checks that the pad rows of the last packed tile (what every packed consumer reads as MFMA columns) are zero.
extern "C" int rdx_stem_test(rdx_ctx* c, const float* image, const float* W, const float* bias, void* out, int B, int S, int stem, int path) {
    if (!c || !image || !W || !bias || !out || B <= 0 || S < 16 || S % 4) return fail(c, -1, "rdx_stem_test: bad arguments (S %% 4 == 0, S >= 16)");
    if (path < 0 || path > 2) return fail(c, -1, "rdx_stem_test: path 0 (fused, row-major), 1 (fused, packed) or 2 (conv_gemm + maxpool_k)");
    if (path < 2 && !stem_pool_supported(stem)) return fail(c, -1, "rdx_stem_test: stem_pool_k has no instantiation for %d channels", stem);
    if (path == 2 && stem % 16) return fail(c, -1, "rdx_stem_test: conv_gemm needs stem %% 16 == 0");
    if (path == 1 && !c->zero16) return fail(c, -1, "rdx_stem_test: no zero line for the packed layout");
    HIPCHK(c, hipSetDevice(c->device));
    const int dt = c->cfg.dtype, Hp = S + 6, Hc = S / 2, Ho = S / 4;
    const long M = (long)B * Ho * Ho;
    const int mt = (int)((M + 15) / 16);
    const size_t wb = (size_t)stem * 224 * 2, ib = (size_t)B * Hp * Hp * 4 * 2;
    const size_t tb = path == 1 ? (size_t)mt * 16 * stem * 2 : (path == 2 ? (size_t)B * Hc * Hc * stem * 2 : 0);
    DevBufs b;
    char* buf = (char*)b.get(wb + ib + tb + 64);
    if (!buf) return fail(c, -2, "rdx_stem_test: out of device memory");
    GemmW w; w.N = stem; w.K = 224; w.Npad = stem; w.w = buf;
    void* vin = buf + wb;
    char* tmp = buf + wb + ib;
    pack_w(c, W, w);
    launch_img_prep(dt, image, vin, B, S, 3, Hp, Hp, c->stream);
    Scoped<bool> ws(c->ws_ok, true);
    int rc = 0;
    if (path == 0) rc = run_stem_pool(c, vin, w, bias, out, B, S, false);
    else if (path == 1) {
        (void)hipMemsetAsync(tmp, 0xff, tb, c->stream);              // what the buffer held before: NaN patterns, so that a missed pad row shows
        rc = run_stem_pool(c, vin, w, bias, tmp, B, S, true);
        if (!rc) launch_unpack_rows(dt, tmp, out, stem, (int)M, stem, c->stream);
    } else {
        conv_gemm(c, vin, w, bias, nullptr, tmp, B, Hp, Hp, 4, 7, 8, 2, 0, Hc, Hc, EPI_RELU);
        launch_maxpool(dt, tmp, out, B, Hc, Hc, stem, c->stream);
    }
    if (rc) return rc;
    if (int frc = finish(c)) return frc;
    if (path == 1 && (M & 15)) {
        std::vector<unsigned short> last((size_t)stem / 32 * 512);
        for (int kc = 0; kc < stem / 32; ++kc)
            HIPCHK(c, hipMemcpy(last.data() + (size_t)kc * 512, tmp + ((size_t)kc * mt + (mt - 1)) * 1024, 1024, hipMemcpyDeviceToHost));
        for (int kc = 0; kc < stem / 32; ++kc)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j)
                    if ((lane & 15) >= (int)(M & 15) && last[(size_t)kc * 512 + lane * 8 + j])
                        return fail(c, -3, "rdx_stem_test: pad row %d of the last packed tile (channel chunk %d) is not zero", lane & 15, kc);
    }
    return 0;
}

// The encoder's normalisation / pooling kernels on caller data (X, emb, out model dtype; gamma, beta, out_f32 fp32; out_f32 nullable):
//   op 0 layernorm_k          X [rows][H] -> out [rows][H] (+ out_f32);
//   op 1 layernorm_ex_k       X rows `ldx` apart -> out rows `ldo` apart; emb (nullable) [aux][H] added as emb[row % aux];
//   op 2 layernorm_packed_k   X [rows][H] packed here (pack_rows_k), normalised packed, unpacked into out [rows][H]; out_f32 [rows][H] by the kernel;
//   op 3 scramble_layernorm_k X NHWC [rows = B][aux = P][H = C] -> out [B][P][C] (+ out_f32);
//   op 4 avgpool_flatten_k    X [rows = B][aux = G][G][H = C] -> out [B][C][G / pool][G / pool] (gamma, beta, eps unused).
extern "C" int rdx_norm_test(rdx_ctx* c, int op, const void* X, const float* gamma, const float* beta, const void* emb, void* out, float* out_f32,
                             int rows, int H, long long ldx, long long ldo, int aux, int pool, float eps) {
    if (!c || !X || !out || rows <= 0 || H <= 0) return fail(c, -1, "rdx_norm_test: bad arguments");
    if (op != 4 && (!gamma || !beta)) return fail(c, -1, "rdx_norm_test: LayerNorm needs gamma and beta");
    HIPCHK(c, hipSetDevice(c->device));
    const int dt = c->cfg.dtype;
    hipStream_t s = c->stream;
    DevBufs b;
    switch (op) {
    case 0: launch_layernorm(dt, X, gamma, beta, out, out_f32, rows, H, eps, s); break;
    case 1:
        if (ldx < H || ldo < H || (emb && aux <= 0)) return fail(c, -1, "rdx_norm_test: layernorm_ex needs ldx, ldo >= H and emb rows > 0");
        launch_layernorm_ex(dt, X, (long)ldx, gamma, beta, emb, emb ? aux : 1, out, (long)ldo, rows, H, eps, s);
        break;
    case 2: {
        if (!layernorm_packed_supported(H)) return fail(c, -1, "rdx_norm_test: layernorm_packed_k has no instantiation for H = %d", H);
        const size_t pb = (size_t)(rows + 15) / 16 * 16 * H * 2;
        char* tmp = (char*)b.get(2 * pb);
        if (!tmp) return fail(c, -2, "rdx_norm_test: out of device memory");
        launch_pack_rows(dt, X, H, tmp, rows, H, s);
        launch_layernorm_packed(dt, tmp, gamma, beta, tmp + pb, out_f32, rows, H, eps, s);
        launch_unpack_rows(dt, tmp + pb, out, H, rows, H, s);
        break;
    }
    case 3:
        if (aux <= 0) return fail(c, -1, "rdx_norm_test: scramble needs P > 0");
        launch_scramble_layernorm(dt, X, gamma, beta, out, out_f32, rows, aux, H, eps, s);
        break;
    case 4:
        if (aux <= 0 || pool <= 0 || aux / pool == 0) return fail(c, -1, "rdx_norm_test: avgpool needs G >= pool > 0");
        launch_avgpool_flatten(dt, X, out, rows, aux, H, pool, s);
        break;
    default: return fail(c, -1, "rdx_norm_test: op 0..4");
    }
    return finish(c);
}

// softmax(Q K^T / sqrt(D)) V through AttnArgs as the encoder / prefill callers fill it. strides[12] = element strides (batch, token, head) of Q, K, V, O;
// key_mask (nullable) uint8 [B][km_bs], km_bs % 4 == 0 and >= Tk (the kernels read the mask as 32-bit words); o_packed: O is written fragment-packed
// ([(h D + d) / 32][ceil(B Tq / 16)][64][8], row = b Tq + q) and unpacked here into out [B Tq][H D] (the O strides are then unused).
// kernel 0 = production dispatch (launch_attention with the context's flash_min), 1 = attention_k, 2 = flash_prefill_k (only where
// flash_prefill_supported holds: an error otherwise).
extern "C" int rdx_attn_test(rdx_ctx* c, const void* Q, const void* K, const void* V, void* out, const long long* strides, int B, int H, int Tq,
                             int Tk, int D, int causal, const uint8_t* key_mask, long long km_bs, int o_packed, int kernel) {
    if (!c || !Q || !K || !V || !out || !strides || B <= 0 || H <= 0 || Tq <= 0 || Tk <= 0) return fail(c, -1, "rdx_attn_test: bad arguments");
    if (!(D == 32 || D == 64 || D == 128)) return fail(c, -1, "rdx_attn_test: head dim 32, 64 or 128");
    if (key_mask && (km_bs < Tk || km_bs % 4)) return fail(c, -1, "rdx_attn_test: key mask rows need km_bs >= Tk and km_bs %% 4 == 0");
    if (kernel < 0 || kernel > 2) return fail(c, -1, "rdx_attn_test: kernel 0 (dispatch), 1 (attention_k) or 2 (flash_prefill_k)");
    if ((size_t)16 * ((Tk + 31) & ~31) * 6 > 160 * 1024 && kernel != 2) return fail(c, -1, "rdx_attn_test: Tk = %d does not fit attention_k's LDS", Tk);
    HIPCHK(c, hipSetDevice(c->device));
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.Q = Q; a.K = K; a.V = V;
    a.q_bs = strides[0]; a.q_ts = strides[1]; a.q_hs = strides[2];
    a.k_bs = strides[3]; a.k_ts = strides[4]; a.k_hs = strides[5];
    a.v_bs = strides[6]; a.v_ts = strides[7]; a.v_hs = strides[8];
    a.o_bs = strides[9]; a.o_ts = strides[10]; a.o_hs = strides[11];
    a.B = B; a.H = H; a.Tq = Tq; a.Tk = Tk; a.causal = causal;
    a.key_mask = key_mask; a.km_bs = key_mask ? (long)km_bs : 0;
    a.flash_min = kernel == 0 ? c->sw.flash_min : (kernel == 2 ? 1 : 0);
    if (kernel == 2 && !flash_prefill_supported(D, a))
        return fail(c, -1, "rdx_attn_test: flash_prefill_k does not take this call (D 128, causal, key mask, 8-element strides)");
    const long M = (long)B * Tq;
    const int mt = (int)((M + 15) / 16);
    DevBufs b;
    void* tmp = o_packed ? b.get((size_t)mt * 16 * H * D * 2) : nullptr;
    if (o_packed && !tmp) return fail(c, -2, "rdx_attn_test: out of device memory");
    a.O = o_packed ? tmp : out; a.o_packed_mt = o_packed ? mt : 0;
    launch_attention(c->cfg.dtype, D, a, c->stream);
    if (o_packed) launch_unpack_rows(c->cfg.dtype, tmp, out, H * D, (int)M, H * D, c->stream);
    return finish(c);
}
