// librdx C ABI, part 8: row sessions (include/rdx.h) -- continuous batching. The decode step runs on `rows` live rows; a finished row is refilled from the
// caller's queue while its neighbours go on decoding. A refill runs the prompt path (api_llama.hip: prefill_rows_at, the launches of rdx_prefill(B = R, T)) into
// STAGING rows above the live ones, then moves each staged row -- its KV of all layers and its decode state -- into its target row (rows.hip). Everything is
// enqueued on the context's stream between steps; the steps are decode_step_launch / the graph of build_graph, unchanged.
#include "rdx_ctx.h"

static RowState row_state(rdx_ctx* c) {
    RowState st;
    st.pos = c->d_pos; st.slot = c->d_slot; st.step = c->d_step; st.unf = c->d_unf;
    st.key_mask = c->key_mask; st.dx = c->dx; st.cur_rope = c->d_cur_rope;
    st.out_tokens = c->cur_tokens; st.stage_tokens = c->rs_stage_tok;
    st.max_len = c->cfg.max_len; st.H = c->cfg.hidden; st.cap = c->rs_cap; st.pad_id = c->cur_pad; st.row0 = c->rs_rows;
    return st;
}

// every row that is not live is (re-)parked: slot and position back to 0, so that no number of steps carries it out of its cache row
static void park_idle_rows(rdx_ctx* c, int clear_tokens) {
    RowList rl;
    rl.n = 0;
    for (int r = 0; r < c->rs_rows; ++r)
        if (c->rs_state[r] != RS_LIVE) { rl.src[rl.n] = 0; rl.dst[rl.n++] = (short)r; }
    launch_row_state_move(row_state(c), rl, clear_tokens ? 3 : 1, c->stream);
}

static int rows_need_session(rdx_ctx* c, const char* who) {
    if (!c->rs_on) return fail(c, -1, "%s: no row session is open on this context; rdx_rows_begin first", who);
    return 0;
}

extern "C" int rdx_rows_begin(rdx_ctx* c, int rows, int stage, int cap, int eos_id, int pad_id, int32_t* out_tokens) {
    if (!c) return -1;
    if (c->rs_on) return fail(c, -1, "rdx_rows_begin: a row session is already open on this context; rdx_rows_end first");
    if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_rows_begin: llama weights not finalized");
    if (int krc = kv8_refuse(c, "rdx_rows_begin", "the row moves copy model-dtype cache rows")) return krc;
    const rdx_config& f = c->cfg;
    if (c->rules_on) return fail(c, -1, "rdx_rows_begin: not available under logits rules (a moved row's token history would have to move too); rdx_set_logits_rules(ctx, NULL) first");
    if (c->sampling.do_sample) return fail(c, -1, "rdx_rows_begin: not available while sampling is on (a moved row's draw index would have to move too); rdx_set_sampling(ctx, NULL) first");
    if (c->logprobs >= 0) return fail(c, -1, "rdx_rows_begin: not available while the logprobs option is on (a moved row's entries would have to move too); rdx_set_logprobs(ctx, -1) first");
    if (rows < 1 || stage < 1 || rows + stage > f.max_batch || rows + stage > ROWLIST_MAX)
        return fail(c, -1, "rdx_rows_begin: rows (%d) + stage (%d) must be >= 1 each and fit max_batch %d", rows, stage, f.max_batch);
    if (cap < 1 || cap >= f.max_len || cap >= f.max_pos) return fail(c, -1, "rdx_rows_begin: cap %d outside [1, max_len %d / max_position_embeddings %d)", cap, f.max_len, f.max_pos);
    if (!out_tokens) return fail(c, -1, "rdx_rows_begin: null out_tokens");
    if (rows + stage > 32 && !blk64_ok(c, rows + stage))
        return fail(c, -1, "rdx_rows_begin: more than 32 rows (%d + %d staging) per context need the Vicuna-7B widths (hidden 4096, inter 11008: the row-block decode family)", rows, stage);
    if (decode_family(c, rows) == DEC_UNSUPPORTED) return fail(c, -1, "rdx_rows_begin: no decode kernel family for %d rows on this model", rows);
    HIPCHK(c, hipSetDevice(c->device));
    const size_t need = (size_t)stage * cap;
    if (need > c->rs_stage_tok_ints) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->rs_stage_tok_ints = 0;
        dfree(c, c->rs_stage_tok);
        ALLOC(c, c->rs_stage_tok, need * sizeof(int32_t));
        c->rs_stage_tok_ints = need;
    }
    c->rs_on = true; c->rs_rows = rows; c->rs_stage = stage; c->rs_cap = cap;
    c->rs_slot.assign(rows, 0); c->rs_step.assign(rows, 0); c->rs_state.assign(rows, RS_PARKED);
    // the step runs on the live rows only (decode_family(rows)); max_new of the step's tail is the session's cap. No conversation for the single-step calls.
    c->cur_B = rows; c->cur_T = 0; c->cur_max_new = cap; c->cur_eos = eos_id; c->cur_pad = pad_id; c->cur_tokens = out_tokens;
    c->cur_steps = cap;
    c->hist_ready = false;
    park_idle_rows(c, /*clear_tokens=*/1);
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int rdx_rows_refill(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int R, int T, const float* qformer_embs, const int32_t* rows_host,
                               void* logits) {
    if (!c) return -1;
    if (int rc = rows_need_session(c, "rdx_rows_refill")) return rc;
    const rdx_config& f = c->cfg;
    if (!ids || !rows_host) return fail(c, -1, "rdx_rows_refill: null ids / rows");
    if (R < 1 || R > c->rs_stage) return fail(c, -1, "rdx_rows_refill: %d prompts outside [1, stage %d]", R, c->rs_stage);
    if (T <= 0 || T + c->rs_cap > f.max_len) return fail(c, -1, "rdx_rows_refill: T (%d) + cap (%d) exceeds max_len %d", T, c->rs_cap, f.max_len);
    if (T + c->rs_cap > f.max_pos) return fail(c, -1, "rdx_rows_refill: sequence exceeds max_position_embeddings %d", f.max_pos);
    if (qformer_embs && T < 32) return fail(c, -1, "rdx_rows_refill: image splice needs T >= 32");
    if (R > 32 && !blk64_ok(c, R)) return fail(c, -1, "rdx_rows_refill: more than 32 prompts per refill need the Vicuna-7B widths (hidden 4096, inter 11008)");
    RowList rl;
    rl.n = R;
    for (int i = 0; i < R; ++i) {
        const int r = rows_host[i];
        if (r < 0 || r >= c->rs_rows) return fail(c, -1, "rdx_rows_refill: target row %d outside [0, %d)", r, c->rs_rows);
        for (int j = 0; j < i; ++j)
            if (rows_host[j] == r) return fail(c, -1, "rdx_rows_refill: target row %d is listed twice", r);
        rl.src[i] = (short)(c->rs_rows + i); rl.dst[i] = (short)r;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = prefill_rows_at(c, ids, mask, R, T, qformer_embs, /*row0=*/c->rs_rows, c->rs_stage_tok, logits)) return rc;
    const int npos = std::min((T + 15) & ~15, f.max_len);
    launch_kv_rows_move(c->kcache, c->vcache, rl, f.heads, f.layers, f.max_len, c->kv_layer_elems * 2, npos, c->stream);
    launch_row_state_move(row_state(c), rl, /*park=*/0, c->stream);
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < R; ++i) { const int r = rows_host[i]; c->rs_slot[r] = T; c->rs_step[r] = 1; c->rs_state[r] = RS_LIVE; }
    return 0;
}

extern "C" int rdx_rows_step(rdx_ctx* c, int n, int use_graph, void* logits) {
    if (!c) return -1;
    if (int rc = rows_need_session(c, "rdx_rows_step")) return rc;
    const rdx_config& f = c->cfg;
    const int lim = std::min(f.max_len, f.max_pos);
    if (n < 1 || n >= lim) return fail(c, -1, "rdx_rows_step: %d steps outside [1, max_len %d)", n, lim);
    if (logits && n != 1) return fail(c, -1, "rdx_rows_step: logits are returned for a single step only (n == 1, got %d)", n);
    for (int r = 0; r < c->rs_rows; ++r)
        if (c->rs_state[r] == RS_LIVE && c->rs_slot[r] + n > lim)
            return fail(c, -1, "rdx_rows_step: KV cache row %d full (slot %d + %d steps of %d); refill or park it", r, c->rs_slot[r], n, lim);
    HIPCHK(c, hipSetDevice(c->device));
    park_idle_rows(c, 0);
    if (use_graph) {
        if (int rc = build_graph(c, logits, /*fixed=*/true)) return rc;
        for (int i = 0; i < n; ++i) HIPCHK(c, hipGraphLaunch(c->graph, c->stream));
    } else {
        for (int i = 0; i < n; ++i) decode_step_launch(c, logits, nullptr, 0);
    }
    for (int r = 0; r < c->rs_rows; ++r)
        if (c->rs_state[r] == RS_LIVE) { c->rs_slot[r] += n; c->rs_step[r] += n; }
    HIPCHK(c, hipGetLastError());
    return take_unsupported(c);
}

extern "C" int rdx_rows_poll(rdx_ctx* c, int32_t* unfinished_host, int32_t* steps_host) {
    if (!c) return -1;
    if (int rc = rows_need_session(c, "rdx_rows_poll")) return rc;
    if (!unfinished_host) return fail(c, -1, "rdx_rows_poll: null unfinished");
    HIPCHK(c, hipSetDevice(c->device));
    int herr = 0;
    HIPCHK(c, hipMemcpyAsync(unfinished_host, c->d_unf, c->rs_rows * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&herr, c->d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int r = 0; r < c->rs_rows; ++r) {
        if (c->rs_state[r] == RS_LIVE && !unfinished_host[r]) c->rs_state[r] = RS_DONE;       // re-parked from the next step on; its tokens stay
        if (steps_host) steps_host[r] = c->rs_step[r];
    }
    if (herr) {
        hipMemset(c->d_err, 0, sizeof(int));
        return fail(c, -5, "rdx_rows_poll: a workgroup hand-off timed out inside a fused/chained launch (results invalid)");
    }
    return 0;
}

extern "C" int rdx_rows_park(rdx_ctx* c, const int32_t* rows_host, int n) {
    if (!c) return -1;
    if (int rc = rows_need_session(c, "rdx_rows_park")) return rc;
    if (!rows_host || n < 1 || n > c->rs_rows) return fail(c, -1, "rdx_rows_park: %d rows outside [1, %d]", n, c->rs_rows);
    RowList rl;
    rl.n = n;
    for (int i = 0; i < n; ++i) {
        const int r = rows_host[i];
        if (r < 0 || r >= c->rs_rows) return fail(c, -1, "rdx_rows_park: row %d outside [0, %d)", r, c->rs_rows);
        rl.src[i] = 0; rl.dst[i] = (short)r;
    }
    HIPCHK(c, hipSetDevice(c->device));
    launch_row_state_move(row_state(c), rl, /*park=*/1, c->stream);
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < n; ++i) { const int r = rows_host[i]; c->rs_slot[r] = 0; c->rs_step[r] = 0; c->rs_state[r] = RS_PARKED; }
    return 0;
}

extern "C" int rdx_rows_end(rdx_ctx* c) {
    if (!c) return -1;
    if (int rc = rows_need_session(c, "rdx_rows_end")) return rc;
    // the caller's out_tokens may go away behind this call: drain what still writes to it
    hipSetDevice(c->device);
    const hipError_t e = hipStreamSynchronize(c->stream);
    c->rs_on = false; c->rs_rows = c->rs_stage = c->rs_cap = 0;
    // no conversation behind a session, as after rdx_score: the decode-step and append calls refuse until the next prefill
    c->cur_B = 0; c->cur_T = 0; c->cur_max_new = 0; c->cur_steps = 0; c->cur_tokens = nullptr;
    c->hist_ready = false;
    if (e != hipSuccess) return fail(c, -2, "rdx_rows_end: hipStreamSynchronize failed: %s", hipGetErrorString(e));
    return 0;
}
