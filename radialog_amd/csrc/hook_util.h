// hook_util.h -- private to librdx_hooks.so (api_debug.hip, api_dec_hooks.hip): what a hook owns for the length of one call, how every hook ends, and the
// weight forms the hooks prepare from the caller's fp32 W with the production packers. Everything here has internal linkage: the library exports its hooks only.
#pragma once
#include <cmath>

#include "rdx_ctx.h"

namespace {

struct DevBufs {       // device temporaries of one hook call, freed on every return path (hipFree waits for the device: a return between a launch and its synchronisation is safe)
    std::vector<void*> p;
    ~DevBufs() { for (void* q : p) hipFree(q); }
    void* get(size_t bytes) {
        void* q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 16) != hipSuccess) return nullptr;
        p.push_back(q);
        return q;
    }
};

struct EventPair {     // the start / stop events of a timed hook, destroyed on every return path
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~EventPair() { if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1); }
    hipError_t start(hipStream_t s) {                // creates both, records the start event
        hipError_t e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        return e != hipSuccess ? e : hipEventRecord(e0, s);
    }
    hipError_t stop(hipStream_t s, float* ms) {      // waits for the stop event; *ms = start .. stop
        hipError_t e = hipEventRecord(e1, s);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        return e != hipSuccess ? e : hipEventElapsedTime(ms, e0, e1);
    }
};

template <typename T>
struct Scoped {        // a context field set for the length of a hook call and put back on every return path (c->ws_ok, c->dxn)
    T& ref; T old;
    Scoped(T& r, T v) : ref(r), old(r) { r = v; }
    ~Scoped() { ref = old; }
    Scoped(const Scoped&) = delete;
};

// how every hook ends: the stream drained, then the context's "unsupported" note taken ALWAYS (a HIP error must not leave it behind for the next call on the
// context); the refusal if there is one (a launch without a kernel for its shape: run_rmsnorm, the dispatch), else the HIP error
int finish(rdx_ctx* c) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (int rc = take_unsupported(c)) return rc;
    HIPCHK(c, e);
    return 0;
}

// the per-tile argmax partials of EPI_LOGITS reduced with the kernels' tie rule (lowest index), as greedy_step_k reduces them in the decode step
int reduce_partials(rdx_ctx* c, const GemmArgs& a, int32_t* argmax_host) {
    const int nt = (a.N + 15) / 16;
    std::vector<float> pv((size_t)a.M * nt);
    std::vector<int> pi((size_t)a.M * nt);
    HIPCHK(c, hipMemcpy(pv.data(), a.part_val, pv.size() * 4, hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(pi.data(), a.part_idx, pi.size() * 4, hipMemcpyDeviceToHost));
    for (int m = 0; m < a.M; ++m) {
        float bv = -INFINITY; int bi = 0x7fffffff;
        for (int t = 0; t < nt; ++t) {
            const float v = pv[(size_t)m * nt + t]; const int ix = pi[(size_t)m * nt + t];
            if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
        }
        argmax_host[m] = bi;
    }
    return 0;
}

// ---- weight forms, from W fp32 [w.N][w.K] into memory the hook owns (w's pointers set by the caller: the hooks keep their own block layouts) ----
// the model dtype, packed as rdx_set_weight packs it (the rows up to w.Npad zero)
void pack_w(rdx_ctx* c, const float* W, const GemmW& w) { launch_pack_weight(c->cfg.dtype, W, w.w, w.N, w.K, w.Npad, nullptr, c->stream); }
// fp8 as the engine holds it: e4m3 bytes (w.w8) + one scale per row (w.scale)
void pack_w8(rdx_ctx* c, const float* W, const GemmW& w) { launch_pack_weight_fp8(c->cfg.dtype, W, w.w8, w.scale, nullptr, w.N, w.K, w.N, c->stream); }
// the coded bf16 copy of the packed w.w, as rdx_finalize_weights builds it for the batch <= 2 step, and the GEMV's arguments pointed at it
void code_w(rdx_ctx* c, const GemmW& w, void* planes, unsigned* hdr, GemmArgs& a) {
    launch_encode_wc(w.w, planes, hdr, w.Npad, w.K, c->stream);
    a.WC = planes; a.wchdr = hdr;
}

// W quantised as rdx_set_weight(RDX_W_GEMM_W4) does it (launch_quant_w4; the tiles of rows [raw_lo, raw_hi) raw): w.w = the packed copy of W',
// w.w4 / w.w4h = the stream and its header words. Returns 0, -2 (out of memory) or -1 (an Inf / NaN in W), after a synchronisation.
int quant_w4_for_test(rdx_ctx* c, DevBufs& b, const float* W, GemmW& w, int raw_lo, int raw_hi) {
    w.w = b.get((size_t)w.Npad * w.K * 2);
    w.w4 = b.get(w4_bytes(w.Npad, w.K));
    w.w4h = (unsigned*)b.get((size_t)(w.Npad / 16) * sizeof(unsigned));
    int* badf = (int*)b.get(sizeof(int));
    if (!w.w || !w.w4 || !w.w4h || !badf) return -2;
    hipMemsetAsync(badf, 0, sizeof(int), c->stream);
    launch_quant_w4(W, w.w, w.w4, w.w4h, badf, w.N, w.K, w.Npad, raw_lo, raw_hi, c->stream);
    int bad = 0;
    if (hipMemcpyAsync(&bad, badf, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    return bad ? -1 : 0;
}

}  // namespace
