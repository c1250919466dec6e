// librdx C ABI, part 5: introspection and in-situ timing of the hot-path units (rdx_kv_read / rdx_hidden_read: the parity tests' view of the
// decoder state; rdx_time: HIP-event timing on the context's stream -- bench.py's live `roofline` figures). Part of the product library.
// (The kernel-test / trace / microbenchmark hooks live in api_debug.hip -> librdx_hooks.so, loaded only under RDX_DEBUG_HOOKS=1.)
#include "rdx_ctx.h"

// ------------------------------------------------------------------------------------------------------------------
// introspection
// ------------------------------------------------------------------------------------------------------------------
extern "C" int rdx_kv_read(rdx_ctx* c, int layer, int which, void* dst) {
    if (!c || !c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_kv_read: no llama state");
    if (layer < 0 || layer >= c->cfg.layers || !dst) return fail(c, -1, "rdx_kv_read: bad arguments");
    if (c->sw.kv_fp8) {        // the stored values x' = code 2^e in the model dtype, logical order
        launch_kv8_read(c->cfg.dtype, kv_ptr(c, which ? c->vcache : c->kcache, layer), kvx_ptr(c, which ? c->vexp : c->kexp, layer), which ? 0 : 1,
                        c->kv_layer_elems / ((size_t)c->cfg.max_len * 128), c->cfg.max_len, nullptr, dst, c->stream);
        return 0;
    }
    if (which) HIPCHK(c, hipMemcpyAsync(dst, kv_ptr(c, c->vcache, layer), c->kv_layer_elems * 2, hipMemcpyDeviceToDevice, c->stream));
    else launch_k_unperm(kv_ptr(c, c->kcache, layer), dst, c->kv_layer_elems / ((size_t)c->cfg.max_len * 128), c->cfg.max_len, c->ld.k_perm, c->stream);   // K: back from the fragment order
    return 0;
}

extern "C" int rdx_kv_read_codes(rdx_ctx* c, int layer, int which, void* codes, void* exps) {
    if (!c || !c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_kv_read_codes: no llama state");
    if (!c->sw.kv_fp8) return fail(c, -1, "rdx_kv_read_codes: the context's KV cache is not fp8 (rdx_set_option kv_fp8)");
    if (layer < 0 || layer >= c->cfg.layers || !codes || !exps) return fail(c, -1, "rdx_kv_read_codes: bad arguments");
    launch_kv8_read(c->cfg.dtype, kv_ptr(c, which ? c->vcache : c->kcache, layer), nullptr, which ? 0 : 1, c->kv_layer_elems / ((size_t)c->cfg.max_len * 128),
                    c->cfg.max_len, codes, nullptr, c->stream);
    HIPCHK(c, hipMemcpyAsync(exps, kvx_ptr(c, which ? c->vexp : c->kexp, layer), c->kv_layer_elems / 128, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

extern "C" long long rdx_kv_bytes(rdx_ctx* c) {
    if (!c || !c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_kv_bytes: no llama state");
    return (long long)c->kv_alloc_bytes;
}

extern "C" int rdx_hidden_read(rdx_ctx* c, void* dst) {
    if (!c || !c->finalized || !c->cfg.enable_llama || c->cur_B <= 0) return fail(c, -1, "rdx_hidden_read: no llama state");
    HIPCHK(c, hipMemcpyAsync(dst, c->datt, (size_t)c->cur_B * c->cfg.hidden * 2, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

extern "C" int rdx_time(rdx_ctx* c, int what, int iters, float* ms_host) {
    if (!c || !c->finalized || !c->cfg.enable_llama || c->cur_B <= 0) return fail(c, -1, "rdx_time: run a prefill first");
    if (int src = rows_refuse(c, "rdx_time")) return src;       // its replays would advance rows behind the session's host mirror
    if (!ms_host || iters <= 0) return fail(c, -1, "rdx_time: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const rdx_config& f = c->cfg;
    const int dt = f.dtype, B = c->cur_B;
    const bool same_layer = what >= 10;   // what = 10 + k: unit k on layer 0 only (weights stay cache resident)
    if (same_layer) what -= 10;
    const DecFamily fam = decode_family(c, B);
    const bool proj = what >= 1 && what <= 5;         // the per-projection units: 1 gate/up, 2 QKV, 3 o_proj, 4 down_proj, 5 lm_head (6: decode attention)
    if (proj && (fam == DEC_BLK || fam == DEC_BLK8 || fam == DEC_UNSUPPORTED)) return fail(c, -1, "rdx_time: the per-projection units time the <= 32-row kernel families; at %d rows use unit 0 (step) or 6 (attention)", B);
    hipEvent_t e0, e1;
    HIPCHK(c, hipEventCreate(&e0));
    HIPCHK(c, hipEventCreate(&e1));
    int launches = 0;
    bool x16 = false;
    if (what == 7) {
        // the chained down(l) -> QKV(l+1) launch (decode_chain_k, batch <= 2), IN SITU: `iters` eager decode steps with an event pair
        // around each of its launches (the hand-off counters are only valid inside a real step, so it cannot be looped alone)
        std::vector<int> slot(B);
        HIPCHK(c, hipMemcpyAsync(slot.data(), c->d_slot, B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (slot[0] + iters >= f.max_len) return fail(c, -1, "rdx_time: %d steps would overflow the KV cache (slot %d, max_len %d)", iters, slot[0], f.max_len);
        std::vector<hipEvent_t> evs, nul;
        bool chained = true;
        for (int i = 0; i < iters && chained; ++i) {
            chained = decode_step_launch(c, nullptr, nullptr, 0, &evs);
            // calibration: an EMPTY bracket (two event records back to back) costs stream time of its own; it is measured in the same
            // stream, once per step, and subtracted from every bracket below
            hipEvent_t a0, a1; hipEventCreate(&a0); hipEventCreate(&a1);
            hipEventRecord(a0, c->stream); hipEventRecord(a1, c->stream);
            nul.push_back(a0); nul.push_back(a1);
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->cur_steps = std::max(c->cur_steps, c->cur_max_new);
        double tot = 0.0, empty = 0.0;
        for (size_t i = 0; i + 1 < evs.size(); i += 2) { float m = 0.f; hipEventElapsedTime(&m, evs[i], evs[i + 1]); tot += m; }
        for (size_t i = 0; i + 1 < nul.size(); i += 2) { float m = 0.f; hipEventElapsedTime(&m, nul[i], nul[i + 1]); empty += m; }
        const size_t n = evs.size() / 2;
        // (the empty bracket costs MORE than what an event adds around a kernel -- subtracting it put the result 6 % under rocprof's
        // kernel duration -- so it is measured but NOT subtracted: the bracket = launch gap + kernel, 7 % over rocprof, conservative)
        (void)empty;
        for (hipEvent_t e : evs) hipEventDestroy(e);
        for (hipEvent_t e : nul) hipEventDestroy(e);
        hipEventDestroy(e0); hipEventDestroy(e1);
        if (!chained || n == 0) return fail(c, -1, "rdx_time(7): the chained down -> QKV launch is not active in this configuration (batch > 2, RDX_CHAIN=0)");
        *ms_host = (float)(tot / (double)n);
        return 0;
    }
    if (what == 0) {
        int rc = build_graph(c, nullptr);
        if (rc) return rc;
        // state advances with every replay: keep the KV slot inside the cache
        std::vector<int> slot(B);
        HIPCHK(c, hipMemcpyAsync(slot.data(), c->d_slot, B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (slot[0] + iters >= f.max_len) return fail(c, -1, "rdx_time: %d replays would overflow the KV cache (slot %d, max_len %d)", iters, slot[0], f.max_len);
        HIPCHK(c, hipEventRecord(e0, c->stream));
        for (int i = 0; i < iters; ++i) HIPCHK(c, hipGraphLaunch(c->graph, c->stream));
        HIPCHK(c, hipEventRecord(e1, c->stream));
        launches = iters;
        c->cur_steps = std::max(c->cur_steps, c->cur_max_new);
    } else {
        if (!proj && what != 6) { hipEventDestroy(e0); hipEventDestroy(e1); return fail(c, -1, "rdx_time: unknown unit %d", what); }
        // Every unit's arguments come from the builders the step launches from (api_dispatch.hip). What the timers change on purpose:
        //  - o_proj / down_proj write to dqkv, so that repeated launches do not grow dx, and (outside xs16, whose xrow16_k needs one) add no residual;
        //  - a projection whose RMSNorm is a launch of its own (skinny_prenorm: rows beyond the GEMV's LDS stage, or the 32-row kernels from 3 rows) is
        //    normalised once, outside the timed region, and the GEMM launches are timed alone.
        const DecUnit u = what == 1 ? UNIT_GATE_UP : what == 2 ? UNIT_QKV : what == 3 ? UNIT_O : what == 4 ? UNIT_DOWN : UNIT_LM_HEAD;
        const int epi = what == 1 ? EPI_SILU_MUL : what == 5 ? EPI_LOGITS : EPI_NONE;
        const bool resid_unit = u == UNIT_O || u == UNIT_DOWN;
        // batch 3-16 decodes on xs16.hip (norm-prologue xstat16_k, un-split xrow16_k): time THOSE kernels, not the 32-row family the step never launches there
        x16 = proj && fam == DEC_XS16;
        GemmArgs pn; bool hoisted = false;
        if (proj && !x16 && !resid_unit) { pn = skinny_prenorm(c, unit_args(c, &c->ll[0], u, B), epi); hoisted = !pn.norm_w; }
        HIPCHK(c, hipEventRecord(e0, c->stream));
        for (int i = 0; i < iters; ++i) {
            for (int l = 0; l < (what == 5 ? 1 : f.layers); ++l, ++launches) {
                const int li = same_layer ? 0 : l;
                const LlamaLayer* L = &c->ll[li];
                if (what == 6) { run_decode_attention(c, dec_attn_args(c, li), li, B); continue; }       // at the current slot (re-appends the same KV row: idempotent)
                // the builder of the step's family (with the copy of the weight that family streams) into the step's choose-and-count launchers
                GemmArgs a = fam == DEC_CHAINED ? chained_unit(c, L, u, B) : x16 ? xs16_unit(c, L, u, B) : unit_args(c, L, u, B);
                if (resid_unit) a.out = c->dqkv;
                if (x16) launch_xs16(c, a, resid_unit ? EPI_RESID : epi);
                else if (resid_unit) {
                    a.resid = nullptr; a.ldr = 0;
                    const bool split = u == UNIT_O ? B >= xs_min_rows() && c->kslab && xsplit32_groups(ksplit_args(a)) : down_split_ok(c, *L, B);
                    if (split) launch_xsplit32(dt, ksplit_args(a), c->kslab, c->stream);
                    else skinny(c, a, EPI_NONE);
                } else {        // (a hoisted RMSNorm leaves skinny() nothing to put in front)
                    if (hoisted) { a = prenormed(c, a); a.xpacked = pn.xpacked; a.xscale = pn.xscale; a.xgroups = pn.xgroups; }
                    skinny(c, a, epi);
                }
            }
        }
        HIPCHK(c, hipEventRecord(e1, c->stream));
    }
    HIPCHK(c, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    hipEventDestroy(e0); hipEventDestroy(e1);
    *ms_host = ms / (float)launches;
    return take_unsupported(c);
}
