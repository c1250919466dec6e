// librdx C ABI, part 3: the Llama decoder -- prompt prefill, the hipGraph-captured greedy decode step, multi-turn append, beam search.
#include <cmath>

#include "rdx_ctx.h"

// ------------------------------------------------------------------------------------------------------------------
// Llama prefill / decode
// ------------------------------------------------------------------------------------------------------------------
static int ensure_prefill_ws(rdx_ctx* c, size_t rows) {
    rows = (rows + 15) & ~(size_t)15;            // the fragment-packed layouts hold whole row tiles of 16
    if (rows <= c->prefill_rows) return 0;
    const rdx_config& f = c->cfg;
    // grows with the largest batch x prompt length seen (test.py-style evaluation: variable prompt lengths): drain the stream,
    // release the old buffers, then allocate; a failure leaves prefill_rows = 0 so the next call starts over
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->prefill_rows = 0;
    dfree(c, c->px); dfree(c, c->pxn); dfree(c, c->pqkv); dfree(c, c->pq); dfree(c, c->patt); dfree(c, c->pgu); dfree(c, c->pxq); dfree(c, c->pxs); dfree(c, c->pslab);
    if (fp8_weights(c->ll[0].wqkv)) {       // e4m3 activations of the fp8 x fp8 prefill GEMMs (gemm8.hip) and their per-(row, K group) scales
        ALLOC(c, c->pxq, rows * (size_t)std::max(f.hidden, f.inter));
        ALLOC(c, c->pxs, rows * 4 * sizeof(float));
    }
    ALLOC(c, c->px, rows * f.hidden * 2); ALLOC(c, c->pxn, rows * f.hidden * 2);
    ALLOC(c, c->pslab, (size_t)4 * std::min<size_t>(rows, 192) * f.hidden * sizeof(float));
    ALLOC(c, c->pqkv, rows * c->ld.qkv_ld * 2); ALLOC(c, c->pq, rows * f.hidden * 2);
    ALLOC(c, c->patt, rows * f.hidden * 2); ALLOC(c, c->pgu, rows * f.inter * 2);
    c->prefill_rows = rows;
    return 0;
}

static const char* const k_need_blk = "more than 32 decoder rows need hidden 4096 / inter 11008 (the row-block family)";

// the tail of a selection on the conversation's rows from base 0 (rdx_kernels.h StepTail); advance == 0: the prompt's token-0 call
StepTail step_tail_args(rdx_ctx* c, int advance) {
    const rdx_config& f = c->cfg;
    StepTail t = {};
    t.eos_id = c->cur_eos; t.pad_id = c->cur_pad; t.max_new = c->cur_max_new; t.out_tokens = c->cur_tokens; t.unfinished = c->d_unf;
    t.pos = advance ? c->d_pos : nullptr; t.slot_b = advance ? c->d_slot : nullptr; t.step_b = c->d_step;
    t.embed = c->embed; t.vocab = f.vocab; t.x_next = c->dx; t.H = f.hidden; t.pos_ro = c->d_pos; t.cos_t = c->rope_cos; t.sin_t = c->rope_sin;
    t.cur_rope = c->d_cur_rope;
    t.ctr_zero = c->sw.chain ? c->d_ctr : nullptr;
    t.n_zero = (int)chain_ctr_ints(f.layers);
    t.epoch = c->d_epoch;
    return t;
}

// row0 / tokens (a row session's refill, never under rules or sampling): the selected rows are rows row0 .. row0 + B - 1 of the per-row decode state, and
// token 0 of row r goes to tokens[r * max_new] instead of the conversation's out_tokens. x, the logits and the argmax partials stay B-row scratch at base 0.
static void lm_head_and_greedy(rdx_ctx* c, const void* x, int B, void* logits, const int* out_step, long step_stride,
                               int advance, int row0 = 0, int32_t* tokens = nullptr) {
    const rdx_config& f = c->cfg;
    // logits rules: the row select_step_k processes must exist, so without a caller buffer the lm_head writes into the context's own
    // (generation log-probs likewise: logprob_step_k reads the row)
    if ((c->rules_on || c->sampling.do_sample || c->logprobs >= 0) && !logits) { logits = c->rule_logits; out_step = nullptr; }
    auto lm = [&](GemmArgs a) { a.X = x; a.out = logits; a.out_step = out_step; a.out_step_stride = step_stride; return a; };
    switch (const DecFamily fam = decode_family(c, B); fam) {
    case DEC_UNSUPPORTED: c->unsupported = k_need_blk; return;
    // 33-128 rows: final RMSNorm into the fragment-packed row tiles (after the last layer it also folds in the K-split down_proj's slabs), lm_head in row blocks
    case DEC_BLK: launch_xstat_blk(f.dtype, norm_in_front(c, lm(blk_unit(c, nullptr, UNIT_LM_HEAD, B))), EPI_LOGITS, c->stream); break;
    case DEC_BLK8: launch_xstat_blk8(f.dtype, norm_in_front(c, lm(blk8_unit(c, nullptr, UNIT_LM_HEAD, B))), EPI_LOGITS, c->stream); break;
    case DEC_XS16:       // batch 3-16 decode: the final RMSNorm is the kernel's prologue (the prompt's last rows, in datt, go the generic way)
        if (x == c->dx) { launch_xs16(c, lm(xs16_unit(c, nullptr, UNIT_LM_HEAD, B)), EPI_LOGITS); break; }
        [[fallthrough]];
    default:       // the prompt's last rows are no decode step: the unit's base form, whichever family the batch decodes on
        skinny(c, lm(advance && fam == DEC_CHAINED ? chained_unit(c, nullptr, UNIT_LM_HEAD, B) : unit_args(c, nullptr, UNIT_LM_HEAD, B)), EPI_LOGITS);
    }
    StepTail t = step_tail_args(c, advance);
    // prompt-lookup decoding (api_lookup.hip): inside rdx_generate_lookup the selection behind every lm_head is lookup_accept_k, here on the one row of a plain forward
    if (c->lk_run) { lookup_accept(c, t, 0, c->part_val, c->part_idx, nullptr); return; }
    if (row0) {       // (advance == 0: pos / slot_b are null)
        t.unfinished += row0; t.step_b += row0; t.pos_ro += row0;
        t.x_next = (char*)c->dx + (size_t)row0 * f.hidden * 2; t.cur_rope = (char*)c->d_cur_rope + (size_t)row0 * 512;
    }
    if (tokens) t.out_tokens = tokens;
    // generation log-probs: behind whichever selection ran, on the row it left and the token its tail wrote (d_step is already advanced: the kernel takes d_step - 1)
    auto logprobs = [&] {
        if (c->logprobs < 0) return;
        LogprobArgs la;
        la.logits = logits; la.row_stride = f.vocab; la.step_stride = out_step ? step_stride : 0;
        la.d_step = c->d_step; la.tokens = c->cur_tokens; la.B = B; la.max_new = c->cur_max_new; la.vocab = f.vocab; la.top_n = c->logprobs;
        la.chosen = c->lp_chosen; la.top_ids = c->lp_top_ids; la.top_lp = c->lp_top_lp; la.out_ld = f.max_len;
        launch_logprob_step(f.dtype, la, c->stream);
    };
    if (!c->rules_on && !c->sampling.do_sample) { launch_greedy_step(f.dtype, c->part_val, c->part_idx, c->n_vtiles, B, t, c->stream); logprobs(); return; }
    // the row at the address the lm_head just wrote (a captured step with scores: both offset it by the step count, read from d_step before the tail advances it)
    if (c->rules_on) { t.hist = c->d_hist; t.hist_len = c->d_hist_len; t.hist_ld = f.max_len; }
    SelectArgs sa;
    sa.logits = logits; sa.step_stride = out_step ? step_stride : 0; sa.n_gen = c->d_step;
    sa.penalty = c->rules.repetition_penalty; sa.ngram = c->rules.no_repeat_ngram_size; sa.min_new = c->rules.min_new_tokens; sa.sel_out = nullptr;
    if (!c->sampling.do_sample) { launch_select_step(f.dtype, sa, t, B, c->stream); logprobs(); return; }
    // sampled: the draw index of row b is d_step[b] too (0 for the token the prefill selects)
    const SampleArgs sp = {c->sampling.temperature, c->sampling.top_k, c->sampling.top_p, c->d_seed};
    launch_sample_step(f.dtype, sa, sp, t, B, c->stream);
    logprobs();
}

// an unwritten entry reads (0.0f, -1, 0.0f): rows [0, B) of the three buffers, in stream order in front of the prompt
static int logprobs_reset(rdx_ctx* c, int B) {
    if (c->logprobs < 0) return 0;
    const size_t n = (size_t)B * c->cfg.max_len;
    HIPCHK(c, hipMemsetAsync(c->lp_chosen, 0, n * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->lp_top_ids, 0xff, n * RDX_MAX_TOP_LOGPROBS * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(c->lp_top_lp, 0, n * RDX_MAX_TOP_LOGPROBS * sizeof(float), c->stream));
    return 0;
}

extern "C" int rdx_set_logprobs(rdx_ctx* c, int top_n) {
    if (!c) return -1;
    if (top_n == -1) { c->logprobs = -1; return 0; }
    if (top_n < 0 || top_n > RDX_MAX_TOP_LOGPROBS) return fail(c, -1, "rdx_set_logprobs: top_n %d of the logprobs outside [0, %d] (-1 = off)", top_n, RDX_MAX_TOP_LOGPROBS);
    if (int src = rows_refuse(c, "rdx_set_logprobs")) return src;
    if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_set_logprobs: llama weights not finalized");
    const rdx_config& f = c->cfg;
    if (!logprob_step_supported(f.vocab)) return fail(c, -1, "rdx_set_logprobs: a row of vocab %d does not fit the LDS of logprob_step_k", f.vocab);
    HIPCHK(c, hipSetDevice(c->device));
    // each buffer on its own: a call that failed half way leaves the option as it was, and the next one allocates what is still missing
    const size_t n = (size_t)f.max_batch * f.max_len;
    const bool fresh = !c->lp_chosen || !c->lp_top_ids || !c->lp_top_lp;
    if (!c->rule_logits) ALLOC(c, c->rule_logits, (size_t)f.max_batch * f.vocab * 2);
    if (!c->lp_chosen) ALLOC(c, c->lp_chosen, n * sizeof(float));
    if (!c->lp_top_ids) ALLOC(c, c->lp_top_ids, n * RDX_MAX_TOP_LOGPROBS * sizeof(int));
    if (!c->lp_top_lp) ALLOC(c, c->lp_top_lp, n * RDX_MAX_TOP_LOGPROBS * sizeof(float));
    const int was = c->logprobs;
    c->logprobs = top_n;
    if (fresh) {        // steps that have not run read (0.0f, -1, 0.0f) from the first call on
        if (int rc = logprobs_reset(c, f.max_batch)) { c->logprobs = was; return rc; }
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return 0;
}

extern "C" int rdx_get_logprobs(rdx_ctx* c, int batch, int n_steps, float* chosen_host, int32_t* top_ids_host, float* top_lp_host) {
    if (!c) return -1;
    if (c->logprobs < 0) return fail(c, -1, "rdx_get_logprobs: the logprobs option is off; rdx_set_logprobs first");
    if (!chosen_host || batch <= 0 || batch > c->cur_B || n_steps <= 0 || n_steps > c->cur_max_new)
        return fail(c, -1, "rdx_get_logprobs: batch %d / n_steps %d outside the conversation's logprobs (%d rows, %d steps)", batch, n_steps, c->cur_B, c->cur_max_new);
    const rdx_config& f = c->cfg;
    const int K = RDX_MAX_TOP_LOGPROBS, n = c->logprobs;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy2D(chosen_host, (size_t)n_steps * sizeof(float), c->lp_chosen, (size_t)f.max_len * sizeof(float), (size_t)n_steps * sizeof(float), batch,
                          hipMemcpyDeviceToHost));
    // [batch][n_steps][8] of the device rows, compacted to [batch][n_steps][top_n] on the host
    const size_t rowb = (size_t)n_steps * K;
    if (top_ids_host && n > 0) {
        std::vector<int32_t> tmp(rowb * batch);
        HIPCHK(c, hipMemcpy2D(tmp.data(), rowb * sizeof(int32_t), c->lp_top_ids, (size_t)f.max_len * K * sizeof(int32_t), rowb * sizeof(int32_t), batch, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < (size_t)batch * n_steps; ++i) for (int k = 0; k < n; ++k) top_ids_host[i * n + k] = tmp[i * K + k];
    }
    if (top_lp_host && n > 0) {
        std::vector<float> tmp(rowb * batch);
        HIPCHK(c, hipMemcpy2D(tmp.data(), rowb * sizeof(float), c->lp_top_lp, (size_t)f.max_len * K * sizeof(float), rowb * sizeof(float), batch, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < (size_t)batch * n_steps; ++i) for (int k = 0; k < n; ++k) top_lp_host[i * n + k] = tmp[i * K + k];
    }
    return 0;
}

static const rdx_sampling k_sampling_off = {0, 1.0f, 0, 1.0f, 0};

extern "C" int rdx_set_sampling(rdx_ctx* c, const rdx_sampling* sm) {
    if (!c) return -1;
    if (!sm || !sm->do_sample) { c->sampling = k_sampling_off; return 0; }
    if (int src = rows_refuse(c, "rdx_set_sampling")) return src;
    const rdx_sampling v = *sm;
    if (!(v.temperature > 0.f) || !std::isfinite(v.temperature)) return fail(c, -1, "rdx_set_sampling: temperature must be a finite float > 0 (1.0 = off)");
    if (v.top_k < 0) return fail(c, -1, "rdx_set_sampling: top_k %d is negative (0 = off)", v.top_k);
    if (!(v.top_p > 0.f) || !(v.top_p <= 1.0f)) return fail(c, -1, "rdx_set_sampling: top_p must be in (0, 1] (1.0 = off)");
    if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_set_sampling: llama weights not finalized");
    const rdx_config& f = c->cfg;
    if (!sample_step_supported(f.vocab)) return fail(c, -1, "rdx_set_sampling: a row of vocab %d does not fit the LDS of sample_step_k", f.vocab);
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->rule_logits) ALLOC(c, c->rule_logits, (size_t)f.max_batch * f.vocab * 2);
    if (!c->d_seed) ALLOC(c, c->d_seed, sizeof(unsigned long long));
    // in stream order behind every step already queued; the source is copied before the call returns (pageable memory)
    const unsigned long long seed = v.seed;
    HIPCHK(c, hipMemcpyAsync(c->d_seed, &seed, sizeof(seed), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sampling = v;
    c->sampling.do_sample = 1;
    c->sampling.seed = 0;           // lives on the device
    return 0;
}

static const rdx_logits_rules k_neutral_rules = {1.0f, 0, 0};

extern "C" int rdx_set_logits_rules(rdx_ctx* c, const rdx_logits_rules* rules) {
    if (!c) return -1;
    const rdx_logits_rules r = rules ? *rules : k_neutral_rules;
    if (!(r.repetition_penalty > 0.f) || !std::isfinite(r.repetition_penalty))
        return fail(c, -1, "rdx_set_logits_rules: repetition_penalty must be a finite float > 0 (1.0 = off)");
    if (r.no_repeat_ngram_size < 0) return fail(c, -1, "rdx_set_logits_rules: no_repeat_ngram_size %d is negative (0 = off)", r.no_repeat_ngram_size);
    if (r.min_new_tokens < 0) return fail(c, -1, "rdx_set_logits_rules: min_new_tokens %d is negative (0 = off)", r.min_new_tokens);
    const bool on = r.repetition_penalty != 1.0f || r.no_repeat_ngram_size != 0 || r.min_new_tokens != 0;
    if (on) {
        if (int src = rows_refuse(c, "rdx_set_logits_rules")) return src;
        if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_set_logits_rules: llama weights not finalized");
        const rdx_config& f = c->cfg;
        if (!select_step_supported(f.vocab)) return fail(c, -1, "rdx_set_logits_rules: vocab %d exceeds the LDS bitmaps of select_step_k", f.vocab);
        HIPCHK(c, hipSetDevice(c->device));
        // each buffer on its own: a call that failed half way leaves the rules off, and the next one allocates what is still missing
        if (!c->d_hist) ALLOC(c, c->d_hist, (size_t)f.max_batch * f.max_len * sizeof(int));
        if (!c->rule_logits) ALLOC(c, c->rule_logits, (size_t)f.max_batch * f.vocab * 2);
        if (!c->d_hist_len) {
            ALLOC(c, c->d_hist_len, (size_t)f.max_batch * sizeof(int));
            HIPCHK(c, hipMemset(c->d_hist_len, 0, (size_t)f.max_batch * sizeof(int)));
        }
    }
    if (on != c->rules_on) c->hist_ready = false;        // the history belongs to the prefill that filled it
    c->rules = on ? r : k_neutral_rules;
    c->rules_on = on;
    return 0;
}

// a decode step under rules continues the history its prefill started
static int rules_need_prefill(rdx_ctx* c, const char* who) {
    if (c->rules_on && !c->hist_ready) return fail(c, -1, "%s: logits rules were set after the last prefill; run a new prefill first", who);
    return 0;
}

// ---- the prompt: one layer loop per kernel family (prompt_plan), every unit's arguments from the builders of api_dispatch.hip ----
// What the prompt path refuses, decided from the arguments and the context alone. Its entry points ask before their first effect: before the workspace
// grows, before cur_* / hist_ready change and before the first launch, so that a refused call leaves the conversation it would have replaced as it was.
static int prompt_refuse(rdx_ctx* c, int B, int keep, int row0) {
    if (c->sw.kv_fp8 && (keep > 0 || row0 > 0)) return fail(c, -1, "the prompt path on the fp8 KV cache (kv_fp8) starts at slot 0 of row 0");
    if (B > 32 && !blk64_ok(c, B)) return fail(c, -8, "rdx_prefill: more than 32 rows per context need the Vicuna-7B widths (hidden 4096, inter 11008: the row-block decode family)");
    return 0;
}

// row-major rows: the <= 32-row kernels or the 128-row tile GEMMs, run_gemm picks per projection
static void prompt_rows(rdx_ctx* c, const PromptPlan& p, int B, int T, int keep, int row0) {
    for (int l = 0; l < c->cfg.layers; ++l) {
        const LlamaLayer* L = &c->ll[l];
        prompt_norm(c, p, L->attn_norm, 0);
        run_gemm(c, prompt_unit(c, p, L, UNIT_QKV), EPI_NONE);
        prompt_attention(c, p, l, B, T, keep, row0);
        run_gemm(c, prompt_unit(c, p, L, UNIT_O), EPI_RESID);
        prompt_norm(c, p, L->mlp_norm, 0);
        run_gemm(c, prompt_unit(c, p, L, UNIT_GATE_UP), EPI_SILU_MUL);
        run_gemm(c, prompt_unit(c, p, L, UNIT_DOWN), EPI_RESID);
    }
}

// one or two prompts (33-384 rows) on fragment-packed row tiles: the norms, the attention and the SwiGLU epilogue write the order the projections read
static void prompt_tiles(rdx_ctx* c, const PromptPlan& p, int B, int T, int keep, int row0) {
    const int dt = c->cfg.dtype;
    hipStream_t s = c->stream;
    auto proj = [&](const GemmArgs& a, int epi) {
        if (p.blk) launch_xstat_blk(dt, a, epi, s);
        else launch_wstat(dt, a, epi, s);
    };
    int pend = 0;       // slab groups a K-split down_proj left for the next RMSNorm
    for (int l = 0; l < c->cfg.layers; ++l) {
        const LlamaLayer* L = &c->ll[l];
        prompt_norm(c, p, L->attn_norm, pend);
        pend = 0;
        proj(prompt_unit(c, p, L, UNIT_QKV), EPI_NONE);
        prompt_attention(c, p, l, B, T, keep, row0);
        proj(prompt_unit(c, p, L, UNIT_O), EPI_RESID);
        prompt_norm(c, p, L->mlp_norm, 0);
        proj(prompt_unit(c, p, L, UNIT_GATE_UP), EPI_SILU_MUL);
        const GemmArgs d = prompt_unit(c, p, L, UNIT_DOWN);
        if (p.down_split) { launch_xsplit_blk(dt, d, c->pslab, s); pend = 4; }
        else launch_wstat(dt, d, EPI_RESID, s);
    }
    if (pend) prompt_norm(c, p, c->ll[0].attn_norm, pend);       // its packed output is read by nobody
}

// fp8 weights (BASELINE configs[4]): every projection of the prompt is an fp8 x fp8 MFMA GEMM (gemm8.hip) over e4m3 activations with one scale per row and
// K group -- quantised in the RMSNorm's epilogue, or by quant_rows_k on the attention / SwiGLU output; LoRA-B, RoPE, attention, SwiGLU and the residual adds
// stay in the model dtype
static void prompt_fp8(rdx_ctx* c, const PromptPlan& p, int B, int T, int keep, int row0) {
    const rdx_config& f = c->cfg;
    const int dt = f.dtype;
    hipStream_t s = c->stream;
    auto gemm8 = [&](const GemmArgs& a, int epi) {
        if (gemm8_supported(a, epi)) launch_gemm8(dt, a, epi, s);
        else c->unsupported = "fp8 weights: prefill projection shape not supported by gemm8 (N % 16, K % 64)";
    };
    for (int l = 0; l < f.layers; ++l) {
        const LlamaLayer* L = &c->ll[l];
        prompt_norm(c, p, L->attn_norm, 0);
        gemm8(prompt_unit(c, p, L, UNIT_QKV), EPI_NONE);
        prompt_attention(c, p, l, B, T, keep, row0);
        const GemmArgs o = prompt_unit(c, p, L, UNIT_O);
        launch_quant_rows(dt, c->patt, f.hidden, c->pxq, c->pxs, p.M, f.hidden, o.xgroups, s);
        gemm8(o, EPI_RESID);
        prompt_norm(c, p, L->mlp_norm, 0);
        gemm8(prompt_unit(c, p, L, UNIT_GATE_UP), EPI_SILU_MUL);
        const GemmArgs d = prompt_unit(c, p, L, UNIT_DOWN);
        launch_quant_rows(dt, c->pgu, f.inter, c->pxq, c->pxs, p.M, f.inter, d.xgroups, s);
        gemm8(d, EPI_RESID);
    }
}

// the embedding rows (+ image splice) of B x T tokens into px, then the layer loop of the prompt's kernel family behind `keep` kept slots. The position ids
// (d_pos_ids), the image positions and the key mask are the caller's: prompt_layers prepares them, a verify pass of api_lookup.hip finds them on the device.
void prompt_embed_layers(rdx_ctx* c, const int32_t* ids, int B, int T, int keep, bool splice, int row0) {
    const rdx_config& f = c->cfg;
    launch_embed_splice(f.dtype, ids, c->d_img_pos, c->embed, f.vocab, c->pimg, 32, c->px, B, T, f.hidden, splice ? 1 : 0, c->stream);
    const PromptPlan p = prompt_plan(c, B, T);
    switch (p.family) {
    case PROMPT_ROWS: prompt_rows(c, p, B, T, keep, row0); break;
    case PROMPT_TILES: prompt_tiles(c, p, B, T, keep, row0); break;
    case PROMPT_FP8: prompt_fp8(c, p, B, T, keep, row0); break;
    }
}

// The prompt through every layer: the residual stream of all B x T positions ends in c->px (row-major [B T][hidden]), K / V in the cache behind `keep` kept
// slots (keep > 0: `T` further tokens of a cached conversation, no image splice), the per-row decode state (d_pos / d_slot / d_step / d_unf, the key mask) is
// that of a prompt of T tokens. What the callers do with px is theirs: the prefill gathers the last row of each prompt for token 0, the scoring pass the rows
// whose successor is scored. The callers have asked prompt_refuse and sized the workspace (ensure_prefill_ws) for B x T rows. hist: start the token history
// of the logits rules from `ids`.
// row0 (a row session's refill; keep == 0, no history): the B prompts fill rows row0 .. row0 + B - 1 of the KV cache, the key mask and the decode state; the
// workspaces (px .., the splice rows, img_pos / pos_ids) are prompt-local and stay at base 0. The launches are those of row0 == 0.
static void prompt_layers(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int B, int T, const float* qformer_embs, int keep, int pad_id, bool hist, int row0 = 0) {
    const rdx_config& f = c->cfg;
    const int dt = f.dtype, H = f.hidden;
    hipStream_t s = c->stream;
    if (keep > 0) {
        launch_prep_append(B, T, keep, c->d_img_pos, c->d_pos_ids, c->d_pos, c->d_slot, c->d_step, c->d_unf, s);
        qformer_embs = nullptr;
    } else {
        launch_prep_prompt(ids, mask, B, T, 32000, pad_id, c->d_img_pos, c->d_pos_ids, c->key_mask + (size_t)row0 * f.max_len, f.max_len, c->d_pos + row0,
                           c->d_slot + row0, c->d_step + row0, c->d_unf + row0, s);
    }
    c->hist_ready = hist;
    if (hist) launch_hist_init(ids, B, T, c->d_hist, c->d_hist_len, f.max_len, s);
    if (qformer_embs) {
        // a8: img_proj_layer on the model-dtype copy of the Q-Former output (".half()", modeling_llama_imgemb.py:576-579)
        launch_from_f32(dt, qformer_embs, c->pqe, (size_t)B * 32 * f.qformer_dim, s);
        run_gemm(c, gargs(c->pqe, f.qformer_dim, c->img_proj_w, c->img_proj_b, c->pimg, H, B * 32), EPI_NONE);
    }
    prompt_embed_layers(c, ids, B, T, keep, qformer_embs != nullptr, row0);
}

// token 0 of B prompts whose layers have run: the last row of each (datt doubles as the [B][H] last-position buffer) through the lm_head and the selection
// (row0 / tokens: lm_head_and_greedy)
static int prompt_token0(rdx_ctx* c, int B, int T, void* logits, int row0 = 0, int32_t* tokens = nullptr) {
    launch_gather_last(c->cfg.dtype, c->px, c->datt, B, T, c->cfg.hidden, c->stream);
    lm_head_and_greedy(c, c->datt, B, logits, nullptr, 0, /*advance=*/0, row0, tokens);
    HIPCHK(c, hipGetLastError());
    return take_unsupported(c);
}

// keep == 0: a fresh prompt. keep > 0: `T` further prompt tokens behind the first `keep` cache slots of the previous call(s)
// (the shared prefix of a multi-turn conversation is not recomputed; no image splice in the continuation).
int prefill_impl(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int B, int T, const float* qformer_embs, int keep,
                        int max_new, int eos_id, int pad_id, int32_t* out_tokens, void* logits) {
    if (!c) return -1;
    if (int src = rows_refuse(c, keep > 0 ? "rdx_prefill_append" : "rdx_prefill")) return src;
    if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_prefill: llama weights not finalized");
    const rdx_config& f = c->cfg;
    if (!ids || !out_tokens || B <= 0 || B > f.max_batch) return fail(c, -1, "rdx_prefill: batch %d outside [1, %d]", B, f.max_batch);
    if (T <= 0 || keep + T + max_new > f.max_len) return fail(c, -1, "rdx_prefill: T (%d) + max_new (%d) exceeds max_len %d", keep + T, max_new, f.max_len);
    if (keep + T + max_new > f.max_pos) return fail(c, -1, "rdx_prefill: sequence exceeds max_position_embeddings %d", f.max_pos);
    if (qformer_embs && T < 32) return fail(c, -1, "rdx_prefill: image splice needs T >= 32");
    if (int prc = prompt_refuse(c, B, keep, 0)) return prc;
    HIPCHK(c, hipSetDevice(c->device));
    if (keep > 0) {
        if (B != c->cur_B) return fail(c, -1, "rdx_prefill_append: batch %d differs from the cached conversation's %d", B, c->cur_B);
        std::vector<int> slot(B);
        HIPCHK(c, hipMemcpyAsync(slot.data(), c->d_slot, B * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (int b = 0; b < B; ++b)
            if (keep > slot[b]) return fail(c, -1, "rdx_prefill_append: keep_len %d exceeds the %d cached positions of row %d", keep, slot[b], b);
    }
    int rc = ensure_prefill_ws(c, (size_t)B * T);
    if (rc) return rc;
    c->cur_B = B; c->cur_T = keep + T; c->cur_max_new = max_new; c->cur_eos = eos_id; c->cur_pad = pad_id; c->cur_tokens = out_tokens;
    c->cur_steps = 1;
    if (int lrc = logprobs_reset(c, B)) return lrc;
    prompt_layers(c, ids, mask, B, T, qformer_embs, keep, pad_id, c->rules_on || c->lk_run);       // (the draft rule searches the history too)
    return prompt_token0(c, B, T, logits);
}

int prefill_rows_at(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int R, int T, const float* qformer_embs, int row0, int32_t* tokens, void* logits) {
    if (int prc = prompt_refuse(c, R, 0, row0)) return prc;
    int rc = ensure_prefill_ws(c, (size_t)R * T);
    if (rc) return rc;
    prompt_layers(c, ids, mask, R, T, qformer_embs, 0, c->cur_pad, /*hist=*/false, row0);
    return prompt_token0(c, R, T, logits, row0, tokens);
}

extern "C" int rdx_prefill(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int B, int T, const float* qformer_embs,
                           int max_new, int eos_id, int pad_id, int32_t* out_tokens, void* logits) {
    return prefill_impl(c, ids, mask, B, T, qformer_embs, 0, max_new, eos_id, pad_id, out_tokens, logits);
}

extern "C" int rdx_prefill_append(rdx_ctx* c, const int32_t* ids_tail, int B, int T_tail, int keep_len, int max_new, int eos_id,
                                  int pad_id, int32_t* out_tokens, void* logits) {
    if (!c) return -1;
    if (int krc = kv8_refuse(c, "rdx_prefill_append", "the kept prefix is not held in the model dtype")) return krc;
    if (c->rules_on) return fail(c, -1, "rdx_prefill_append: not available under logits rules (the token history is not carried across calls); rdx_set_logits_rules(ctx, NULL) first");
    if (keep_len <= 0 || c->cur_B <= 0) return fail(c, -1, "rdx_prefill_append: no cached conversation to continue (keep_len %d)", keep_len);
    return prefill_impl(c, ids_tail, nullptr, B, T_tail, nullptr, keep_len, max_new, eos_id, pad_id, out_tokens, logits);
}

// ------------------------------------------------------------------------------------------------------------------
// Scoring given tokens (include/rdx.h): what LlamaForCausalLM.forward(input_ids, attention_mask, labels) computes in the reference
// (modeling_llama_imgemb.py:705-793) -- the prompt's layers as in the prefill, then the final RMSNorm, the lm_head and score_rows_k (score.hip) on the rows
// whose successor position is scored (every row when the caller wants the logits), in chunks of score_chunk rows through ONE logits workspace.
// ------------------------------------------------------------------------------------------------------------------
static int ensure_score_ws(rdx_ctx* c, size_t rows, size_t chunk) {
    const rdx_config& f = c->cfg;
    if (rows > c->sc_rows) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->sc_rows = 0;
        dfree(c, c->sc_x); dfree(c, c->sc_xn); dfree(c, c->sc_idx); dfree(c, c->sc_lp); dfree(c, c->sc_t1);
        ALLOC(c, c->sc_x, rows * f.hidden * 2); ALLOC(c, c->sc_xn, rows * f.hidden * 2);
        ALLOC(c, c->sc_idx, rows * 4 * sizeof(int)); ALLOC(c, c->sc_lp, rows * sizeof(float)); ALLOC(c, c->sc_t1, rows * sizeof(int));
        c->sc_rows = rows;
    }
    if (chunk > c->sc_ws_rows) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->sc_ws_rows = 0;
        dfree(c, c->sc_logits);
        ALLOC(c, c->sc_logits, chunk * (size_t)c->lm_head.Npad * 2);
        c->sc_ws_rows = chunk;
    }
    return 0;
}

extern "C" int rdx_score(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int B, int T, const float* qformer_embs, const int32_t* labels_host,
                         float* logprob, int32_t* top1, void* logits) {
    if (!c) return -1;
    if (int src = rows_refuse(c, "rdx_score")) return src;
    if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_score: llama weights not finalized");
    const rdx_config& f = c->cfg;
    if (!ids || !labels_host || !logprob || B <= 0 || B > f.max_batch) return fail(c, -1, "rdx_score: batch %d outside [1, %d]", B, f.max_batch);
    if (T <= 0 || T > f.max_len) return fail(c, -1, "rdx_score: T (%d) exceeds max_len %d", T, f.max_len);
    if (T > f.max_pos) return fail(c, -1, "rdx_score: sequence exceeds max_position_embeddings %d", f.max_pos);
    if (qformer_embs && T < 32) return fail(c, -1, "rdx_score: image splice needs T >= 32");
    if (fp8_weights(c->ll[0].wqkv) || fp8_weights(c->lm_head))
        return fail(c, -1, "rdx_score: not available on an fp8-weight context (an all-position lm_head needs a quantisation convention the oracle does not define below batch 3)");
    const int V = f.vocab, ld = c->lm_head.Npad, H = f.hidden;
    if (!score_rows_supported(V, ld)) return fail(c, -1, "rdx_score: a logits row of vocab %d (stride %d) does not fit the LDS of score_rows_k", V, ld);
    for (size_t i = 0; i < (size_t)B * T; ++i)
        if (labels_host[i] != -100 && (labels_host[i] < 0 || labels_host[i] >= V))
            return fail(c, -1, "rdx_score: label %d (row %d, position %d) outside [0, %d) and not -100", labels_host[i], (int)(i / T), (int)(i % T), V);
    HIPCHK(c, hipSetDevice(c->device));
    // row i of the tail = position (b, t): its logits score the label of position t + 1. With `logits` every position takes part.
    std::vector<int> rows, tgt, dst, ldst;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T; ++t) {
            const bool scored = t + 1 < T && labels_host[(size_t)b * T + t + 1] != -100;
            if (!scored && !logits) continue;
            rows.push_back(b * T + t); tgt.push_back(scored ? labels_host[(size_t)b * T + t + 1] : -100);
            dst.push_back(scored ? b * T + t + 1 : -1); ldst.push_back(logits ? b * T + t : -1);
        }
    const size_t n = rows.size();
    const size_t chunk = c->sw.score_chunk > 0 ? std::min<size_t>((size_t)c->sw.score_chunk, n) : n;
    if (int prc = n ? prompt_refuse(c, B, 0, 0) : 0) return prc;       // (nothing scored: no prompt runs)
    int rc = ensure_prefill_ws(c, (size_t)B * T);
    if (rc) return rc;
    if (n && (rc = ensure_score_ws(c, n, chunk))) return rc;
    hipStream_t s = c->stream;
    // no conversation behind this call: the decode steps and the append calls refuse until the next prefill
    c->cur_B = 0; c->cur_T = 0; c->cur_max_new = 0; c->cur_steps = 0; c->cur_tokens = nullptr;
    c->hist_ready = false;
    HIPCHK(c, hipMemsetAsync(logprob, 0, (size_t)B * T * sizeof(float), s));
    if (top1) HIPCHK(c, hipMemsetAsync(top1, 0xff, (size_t)B * T * sizeof(int32_t), s));       // -1
    if (n) {
        prompt_layers(c, ids, mask, B, T, qformer_embs, 0, /*pad_id=*/0, /*hist=*/false);
        int* d_rows = c->sc_idx; int *d_tgt = d_rows + n, *d_dst = d_tgt + n, *d_ldst = d_dst + n;
        HIPCHK(c, hipMemcpyAsync(d_rows, rows.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_tgt, tgt.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_dst, dst.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(d_ldst, ldst.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
        launch_gather_rows(f.dtype, c->px, d_rows, c->sc_x, (int)n, H, s);
        run_rmsnorm(c, NormArgs{c->sc_x, c->final_norm, c->sc_xn, nullptr, (int)n, H, f.rms_eps, ACT_ROWS, 0, nullptr, 0});
        for (size_t i0 = 0; i0 < n; i0 += chunk) {
            const int m = (int)std::min(chunk, n - i0);
            GemmArgs a = gargs((const char*)c->sc_xn + i0 * H * 2, H, c->lm_head, nullptr, c->sc_logits, ld, m);
            a.N = ld;      // whole tiles: the pad columns are written too and never read back
            run_gemm(c, a, EPI_NONE);
            launch_score_rows(f.dtype, c->sc_logits, ld, d_tgt + i0, V, c->sc_lp + i0, c->sc_t1 + i0, m, s);
            if (logits) launch_logits_out(f.dtype, c->sc_logits, ld, d_ldst + i0, logits, V, m, s);
        }
        launch_score_scatter(c->sc_lp, c->sc_t1, d_dst, logprob, top1, (int)n, s);
    }
    HIPCHK(c, hipStreamSynchronize(s));      // the index lists are this call's host vectors
    HIPCHK(c, hipGetLastError());
    return take_unsupported(c);
}

static int decode_loop(rdx_ctx* c, int B, int max_new, int eos_id, void* scores, int* n_steps_host, int use_graph);

// ---- the decode step: one layer loop per kernel family (decode_family), every unit's arguments from the builders of api_dispatch.hip ----
// 33-128 rows, model-dtype weights (api_dispatch.hip blk64_ok): 7 launches per layer
static void step_blk(rdx_ctx* c, int B) {
    const int dt = c->cfg.dtype;
    hipStream_t s = c->stream;
    for (int l = 0; l < c->cfg.layers; ++l) {
        const LlamaLayer* L = &c->ll[l];
        launch_xstat_blk(dt, norm_in_front(c, blk_unit(c, L, UNIT_QKV, B)), EPI_NONE, s);
        DecAttnArgs at = dec_attn_args(c, l);
        at.out_packed = ACT_TILES32; at.out_mt = (B + 15) / 16;
        run_decode_attention(c, at, l, B);
        launch_xstat_blk(dt, blk_unit(c, L, UNIT_O, B), EPI_RESID, s);
        launch_xstat_blk(dt, norm_in_front(c, blk_unit(c, L, UNIT_GATE_UP, B)), EPI_SILU_MUL, s);
        // down_proj: K-split over 4 workgroups per tile into fp32 slabs, combined (+ residual) by the next RMSNorm (xsplit32_k<.., BLK>: 21 us against
        // 29.5 us for the prompt's weight-stationary kernel at 64 rows); RDX_BLK_DOWN=0: wstat_k, the A/B leg
        const GemmArgs d = blk_unit(c, L, UNIT_DOWN, B);
        if (c->sw.blk_down && xsplit_blk_supported(d)) { launch_xsplit_blk(dt, d, c->kslab, s); c->pend_groups = 4; }
        else launch_wstat(dt, d, EPI_RESID, s);
    }
}

// 33-128 rows, fp8 weights: the 32-row fp8 kernels per row block (api_dispatch.hip blk64_ok); both residual projections K-split, their slabs + residual left to
// the next RMSNorm
static void step_blk8(rdx_ctx* c, int B) {
    const int dt = c->cfg.dtype;
    hipStream_t s = c->stream;
    auto ksplit = [&](const GemmArgs& a) { launch_xsplit_blk8(dt, a, c->kslab, s); c->pend_groups = xsplit_blk8_groups(a); };
    for (int l = 0; l < c->cfg.layers; ++l) {
        const LlamaLayer* L = &c->ll[l];
        launch_xstat_blk8(dt, norm_in_front(c, blk8_unit(c, L, UNIT_QKV, B)), EPI_NONE, s);
        DecAttnArgs at = dec_attn_args(c, l);
        at.out_packed = ACT_BLK64;
        run_decode_attention(c, at, l, B);
        ksplit(blk8_unit(c, L, UNIT_O, B));
        launch_xstat_blk8(dt, norm_in_front(c, blk8_unit(c, L, UNIT_GATE_UP, B)), EPI_SILU_MUL, s);
        ksplit(blk8_unit(c, L, UNIT_DOWN, B));
    }
}

// batch 3-16 (xs16.hip): five launches per layer -- QKV with the RMSNorm as its prologue, attention (output fragment-packed), o_proj with the
// residual epilogue, gate/up with the RMSNorm prologue (SwiGLU output fragment-packed), down_proj with the residual epilogue. Which units stream an int4 copy:
// the table (api_dispatch.hip stream_wants) through xs16_unit; launch_xs16 takes the int4 kernel where the arguments carry one.
static void step_xs16(rdx_ctx* c, int B) {
    for (int l = 0; l < c->cfg.layers; ++l) {
        const LlamaLayer* L = &c->ll[l];
        launch_xs16(c, xs16_unit(c, L, UNIT_QKV, B), EPI_NONE);
        DecAttnArgs at = dec_attn_args(c, l);
        at.out_packed = ACT_BLK32;
        run_decode_attention(c, at, l, B);
        launch_xs16(c, xs16_unit(c, L, UNIT_O, B), EPI_RESID);
        launch_xs16(c, xs16_unit(c, L, UNIT_GATE_UP, B), EPI_SILU_MUL);
        launch_xs16(c, xs16_unit(c, L, UNIT_DOWN, B), EPI_RESID);
    }
}

// attention + o_proj of the chained and the generic family: ONE fused launch where it exists (batch <= 2, RDX_FUSE_AO), else two
static void attn_oproj(rdx_ctx* c, int l, int B) {
    const int dt = c->cfg.dtype;
    const LlamaLayer& L = c->ll[l];
    DecAttnArgs at = dec_attn_args(c, l);
    const GemmArgs ao = unit_args(c, &L, UNIT_O, B);
    if (c->sw.fuse_ao && attn_oproj16_supported(c->ld, L.wo.N, L.wo.K, B)) {
        at.trace = l == c->ao_trace_layer ? c->ao_trace : nullptr;
        at.out = c->d_gran; at.epoch = c->d_epoch; at.layers = c->cfg.layers; at.layer = l;      // tagged granules instead of datt (handoff.h)
        GemmArgs ag = ao;
        ag.X = c->d_gran;
        launch_attn_oproj16(dt, at, ag, B, c->d_hint, c->d_err, c->stream);
        return;
    }
    // batch 3-32: attention writes its output fragment-packed and o_proj runs K-split over two workgroups per tile,
    // its residual epilogue folded into the RMSNorm in front of gate/up (xsplit32_k)
    const GemmArgs ap = ksplit_args(ao);
    const int kg = (B >= xs_min_rows() && c->kslab) ? xsplit32_groups(ap) : 0;
    at.out_packed = kg > 0 ? ap.xpacked : ACT_ROWS;
    run_decode_attention(c, at, l, B);
    if (kg) launch_ksplit(c, ap);
    else skinny(c, ao, EPI_RESID);
}

// the GEMV family (batch 1-2 without the chained launch, and every shape the activation-stationary kernels refuse) and, from 3 rows, the 32-row
// xstat32 / xsplit32 kernels behind stand-alone RMSNorms: skinny() picks per projection
static void step_generic(rdx_ctx* c, int B) {
    for (int l = 0; l < c->cfg.layers; ++l) {
        const LlamaLayer& L = c->ll[l];
        skinny(c, unit_args(c, &L, UNIT_QKV, B), EPI_NONE);
        attn_oproj(c, l, B);
        const bool split = down_split_ok(c, L, B);
        GemmArgs gu = unit_args(c, &L, UNIT_GATE_UP, B);
        gu.out_packed = split ? ksplit_args(unit_args(c, &L, UNIT_DOWN, B)).xpacked : ACT_ROWS;         // down_proj's K-split reads the SwiGLU output fragment-packed
        skinny(c, gu, EPI_SILU_MUL);
        launch_down(c, L, B, split);
    }
}

// batch <= 2: QKV of layer 0 and every gate/up stand-alone, attention + o_proj fused, down(l) -> QKV(l+1) chained inside one launch by the fence-free hand-off.
// The hand-off counter shards of the chained launches are cleared by greedy_step_k at the end of the previous step (and of the prefill): a memset node at the
// head of the step graph was observed to race with the first producers. The fused launch's tagged granules need no clearing: step_tail bumps their epoch. evs: an event pair around every chained launch (rdx_time 7).
// Which copy of its weight each launch streams: the table (api_dispatch.hip stream_wants) through chained_unit and chain_args.
static void step_chained(rdx_ctx* c, int B, std::vector<hipEvent_t>* evs) {
    auto mark = [&] { if (evs) { hipEvent_t e; hipEventCreate(&e); hipEventRecord(e, c->stream); evs->push_back(e); } };
    skinny(c, chained_unit(c, &c->ll[0], UNIT_QKV, B), EPI_NONE);
    for (int l = 0; l < c->cfg.layers; ++l) {
        attn_oproj(c, l, B);
        skinny(c, chained_unit(c, &c->ll[l], UNIT_GATE_UP, B), EPI_SILU_MUL);
        mark();
        launch_chain(c, l, B);
        mark();
    }
}

bool decode_step_launch(rdx_ctx* c, void* logits, const int* out_step, long step_stride, std::vector<hipEvent_t>* evs) {
    const int B = c->cur_B;
    const DecFamily fam = decode_family(c, B);
    switch (fam) {
    case DEC_UNSUPPORTED: c->unsupported = k_need_blk; return false;
    case DEC_BLK: step_blk(c, B); break;
    case DEC_BLK8: step_blk8(c, B); break;
    case DEC_XS16: step_xs16(c, B); break;
    case DEC_CHAINED: step_chained(c, B, evs); break;
    case DEC_GENERIC: step_generic(c, B); break;
    }
    lm_head_and_greedy(c, c->dx, B, logits, out_step, step_stride, /*advance=*/1);
    return fam == DEC_CHAINED;
}

extern "C" int rdx_decode_step(rdx_ctx* c, void* logits) {
    if (!c) return -1;
    if (int src = rows_refuse(c, "rdx_decode_step")) return src;
    if (!c->finalized || c->cur_B <= 0) return fail(c, -1, "rdx_decode_step: no prefill has run");
    // every step appends one KV row per batch row and advances the RoPE position: refuse to walk past what the prefill reserved
    if (c->cur_steps >= c->cur_max_new)
        return fail(c, -1, "rdx_decode_step: all %d tokens of this prompt (max_new) have been generated; run a new prefill", c->cur_max_new);
    if (c->cur_T + c->cur_steps > c->cfg.max_len || c->cur_T + c->cur_steps > c->cfg.max_pos)
        return fail(c, -1, "rdx_decode_step: KV cache full (%d prompt + %d generated slots of %d)", c->cur_T, c->cur_steps, c->cfg.max_len);
    if (int rrc = rules_need_prefill(c, "rdx_decode_step")) return rrc;
    HIPCHK(c, hipSetDevice(c->device));
    decode_step_launch(c, logits, nullptr, 0);
    ++c->cur_steps;
    HIPCHK(c, hipGetLastError());
    return take_unsupported(c);
}

// The caller drives the loop and supplies the token itself (what LlamaForCausalLM.forward(input_ids = [B, 1], past_key_values = ...) is
// in the reference, modeling_llama_imgemb.py:705-793 behind prepare_inputs_for_generation :795-836): the embedding rows of `ids` replace
// the rows of the token the previous step selected, then the ordinary decode step runs.
extern "C" int rdx_decode_step_ids(rdx_ctx* c, const int32_t* ids, void* logits) {
    if (!c) return -1;
    if (int src = rows_refuse(c, "rdx_decode_step_ids")) return src;
    if (!ids) return fail(c, -1, "rdx_decode_step_ids: null ids");
    if (!c->finalized || c->cur_B <= 0) return fail(c, -1, "rdx_decode_step_ids: no prefill has run");
    if (c->cur_steps >= c->cur_max_new)
        return fail(c, -1, "rdx_decode_step_ids: all %d tokens of this prompt (max_new) have been generated; run a new prefill", c->cur_max_new);
    if (c->cur_T + c->cur_steps > c->cfg.max_len || c->cur_T + c->cur_steps > c->cfg.max_pos)
        return fail(c, -1, "rdx_decode_step_ids: KV cache full (%d prompt + %d generated slots of %d)", c->cur_T, c->cur_steps, c->cfg.max_len);
    if (int rrc = rules_need_prefill(c, "rdx_decode_step_ids")) return rrc;
    HIPCHK(c, hipSetDevice(c->device));
    launch_embed_rows(c->cfg.dtype, ids, c->embed, c->cfg.vocab, c->dx, c->cur_B, c->cfg.hidden, c->stream);
    if (c->rules_on) launch_hist_set_last(ids, c->d_hist, c->d_hist_len, c->cfg.max_len, c->cur_B, c->stream);      // the caller's token is the history, not the one it replaces
    decode_step_launch(c, logits, nullptr, 0);
    ++c->cur_steps;
    HIPCHK(c, hipGetLastError());
    return take_unsupported(c);
}

int build_graph(rdx_ctx* c, void* scores, bool fixed) {
    const rdx_config& f = c->cfg;
    GraphKey k;
    k.B = c->cur_B; k.max_new = c->cur_max_new; k.eos = c->cur_eos; k.pad = c->cur_pad; k.tokens = c->cur_tokens; k.scores = scores; k.fixed = fixed;
    k.rules = c->rules;
    k.sampling = c->sampling;
    k.logprobs = c->logprobs;
    k.lookup = c->lk_run ? c->lk_corpus : nullptr;
    if (int rrc = rules_need_prefill(c, "decode step graph")) return rrc;
    if (c->graph && k == c->gkey) return 0;
    if (c->graph) { hipGraphExecDestroy(c->graph); c->graph = nullptr; }
    hipGraph_t g = nullptr;
    HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    decode_step_launch(c, scores, (scores && !fixed) ? c->d_step : nullptr, (long)c->cur_B * f.vocab);
    HIPCHK(c, hipStreamEndCapture(c->stream, &g));
    if (int urc = take_unsupported(c)) { hipGraphDestroy(g); return urc; }
    HIPCHK(c, hipGraphInstantiate(&c->graph, g, nullptr, nullptr, 0));
    HIPCHK(c, hipGraphDestroy(g));
    c->gkey = k;
    return 0;
}

extern "C" int rdx_generate(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int B, int T, const float* qformer_embs,
                            int max_new, int eos_id, int pad_id, int32_t* out_tokens, void* scores, int* n_steps_host,
                            int use_graph) {
    if (!c) return -1;
    if (max_new <= 0) return fail(c, -1, "rdx_generate: max_new must be positive");
    int rc = rdx_prefill(c, ids, mask, B, T, qformer_embs, max_new, eos_id, pad_id, out_tokens, scores);
    if (rc) return rc;
    return decode_loop(c, B, max_new, eos_id, scores, n_steps_host, use_graph);
}

extern "C" int rdx_generate_append(rdx_ctx* c, const int32_t* ids_tail, int B, int T_tail, int keep_len, int max_new, int eos_id,
                                   int pad_id, int32_t* out_tokens, void* scores, int* n_steps_host, int use_graph) {
    if (!c) return -1;
    if (max_new <= 0) return fail(c, -1, "rdx_generate_append: max_new must be positive");
    if (int krc = kv8_refuse(c, "rdx_generate_append", "the kept prefix is not held in the model dtype")) return krc;
    if (c->rules_on) return fail(c, -1, "rdx_generate_append: not available under logits rules (the token history is not carried across calls); rdx_set_logits_rules(ctx, NULL) first");
    int rc = rdx_prefill_append(c, ids_tail, B, T_tail, keep_len, max_new, eos_id, pad_id, out_tokens, scores);
    if (rc) return rc;
    return decode_loop(c, B, max_new, eos_id, scores, n_steps_host, use_graph);
}

static int decode_loop(rdx_ctx* c, int B, int max_new, int eos_id, void* scores, int* n_steps_host, int use_graph) {
    int rc = 0;
    const rdx_config& f = c->cfg;
    int done = 1;
    std::vector<int> unf(B, 1);
    auto all_finished = [&]() -> int {
        if (eos_id < 0) return 0;
        if (hipMemcpyAsync(unf.data(), c->d_unf, B * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return 0;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return 0;
        for (int b = 0; b < B; ++b) if (unf[b]) return 0;
        return 1;
    };
    if (max_new > 1 && !all_finished()) {
        if (use_graph) {
            rc = build_graph(c, scores);
            if (rc) return rc;
        }
        // EOS poll: a 4-byte-per-row copy + stream sync every 4th step (round 4: every 16th -- up to 15 wasted 3.9-ms steps per finished
        // batch); the sync costs one launch-queue drain (~20 us) per 4 steps of 2.6-3.9 ms. The switch "eos_poll" overrides (tools/eos_time.py)
        const int check_every = c->sw.eos_poll > 0 ? c->sw.eos_poll : 4;
        while (done < max_new) {
            if (use_graph) {
                HIPCHK(c, hipGraphLaunch(c->graph, c->stream));
            } else {
                void* lg = scores ? (char*)scores + (size_t)done * B * f.vocab * 2 : nullptr;
                decode_step_launch(c, lg, nullptr, 0);
            }
            ++done;
            if (eos_id >= 0 && (done % check_every == 0) && done < max_new && all_finished()) break;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipGetLastError());
    if (n_steps_host) *n_steps_host = done;
    c->cur_steps = std::max(done, c->cur_max_new);        // the conversation is complete: further single steps need a new prefill
    int herr = 0;
    HIPCHK(c, hipMemcpy(&herr, c->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (herr) {
        hipMemset(c->d_err, 0, sizeof(int));
        return fail(c, -5, "rdx_generate: a workgroup hand-off timed out inside a fused/chained launch (results invalid)");
    }
    return 0;
}


// ------------------------------------------------------------------------------------------------------------------
// beam search: transformers 4.28.1 GenerationMixin.beam_search + BeamSearchScorer, as
// LlamaForCausalLM.generate(num_beams = k) runs it from test.py:467,:629; _reorder_cache = modeling_llama_imgemb.py:838-843
// ------------------------------------------------------------------------------------------------------------------
namespace {
struct BeamHyp { float score; std::vector<int> toks; };
struct BeamHyps {           // transformers 4.28.1 BeamHypotheses
    int num_beams; float length_penalty; int early_stopping;
    std::vector<BeamHyp> beams; float worst = 1e9f;
    void add(const std::vector<int>& gen, int full_len, float sum_logprobs) {
        const float score = sum_logprobs / powf((float)full_len, length_penalty);
        if ((int)beams.size() < num_beams || score > worst) {
            beams.push_back(BeamHyp{score, gen});
            if ((int)beams.size() > num_beams) {
                // sorted([(s, idx)]): drop the lowest score (lowest index on a tie), the runner-up becomes the worst kept score
                int lo = 0;
                for (int i = 1; i < (int)beams.size(); ++i) if (beams[i].score < beams[lo].score) lo = i;
                beams.erase(beams.begin() + lo);
                float w = beams[0].score;
                for (const BeamHyp& h : beams) w = std::min(w, h.score);
                worst = w;
            } else {
                worst = std::min(score, worst);
            }
        }
    }
    bool is_done(float best_sum_logprobs, int cur_len) const {
        if ((int)beams.size() < num_beams) return false;
        if (early_stopping) return true;
        return worst >= best_sum_logprobs / powf((float)cur_len, length_penalty);
    }
};
}  // namespace

extern "C" int rdx_beam_search(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int groups, int num_beams, int T,
                               const float* qformer_embs, int max_new, int eos_id, int pad_id, float length_penalty,
                               int early_stopping, int32_t* out_tokens_host, int32_t* out_len_host, float* out_score_host,
                               void* step_scores, int* n_steps_host) {
    if (!c) return -1;
    if (int src = rows_refuse(c, "rdx_beam_search")) return src;
    if (int krc = kv8_refuse(c, "rdx_beam_search", "the beam reorder moves model-dtype cache rows")) return krc;
    if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_beam_search: llama weights not finalized");
    const rdx_config& f = c->cfg;
    if (c->logprobs >= 0) return fail(c, -1, "rdx_beam_search: not available while the logprobs option is on (beams return sequence scores); rdx_set_logprobs(ctx, -1) first");
    if (c->sampling.do_sample) return fail(c, -1, "rdx_beam_search: not available while sampling is on (beam-sample is not built); rdx_set_sampling(ctx, NULL) first");
    if (c->rules_on) return fail(c, -1, "rdx_beam_search: not available under logits rules (beam search applies them to log-softmax scores and reorders histories); rdx_set_logits_rules(ctx, NULL) first");
    const int rows = groups * num_beams;
    if (groups <= 0 || num_beams < 2 || num_beams > RDX_MAX_BEAMS) return fail(c, -1, "rdx_beam_search: num_beams must be in [2, %d]", RDX_MAX_BEAMS);
    if (rows > f.max_batch) return fail(c, -1, "rdx_beam_search: batch %d x %d beams exceeds max_batch %d", groups, num_beams, f.max_batch);
    if (max_new <= 0 || !out_tokens_host || !out_len_host) return fail(c, -1, "rdx_beam_search: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int K2 = 2 * num_beams, V = f.vocab;
    const int p_lo = T / 16 * 16, span = (T + max_new + 15) / 16 * 16 - p_lo;
    if (rows > c->bm_rows || max_new > c->bm_new) {
        HIPCHK(c, hipStreamSynchronize(s));
        dfree(c, c->bm_logits); dfree(c, c->bm_scores); dfree(c, c->bm_cand_s); dfree(c, c->bm_cand_i); dfree(c, c->bm_tok); dfree(c, c->bm_src); dfree(c, c->bm_out);
        const int R = std::max(rows, c->bm_rows), N = std::max(max_new, c->bm_new);
        c->bm_rows = 0;
        ALLOC(c, c->bm_logits, (size_t)R * V * 2); ALLOC(c, c->bm_scores, (size_t)R * 4);
        ALLOC(c, c->bm_cand_s, (size_t)R * 2 * 4); ALLOC(c, c->bm_cand_i, (size_t)R * 2 * 4);
        ALLOC(c, c->bm_tok, (size_t)R * 4); ALLOC(c, c->bm_src, (size_t)R * 2 * 4); ALLOC(c, c->bm_out, (size_t)R * N * 4);       // bm_src: src[R] | start[R]
        c->bm_rows = R; c->bm_new = N;
    }
    const size_t need = (size_t)f.layers * 2 * rows * f.heads * span * 256;
    if (need > c->bm_scratch_bytes) {
        HIPCHK(c, hipStreamSynchronize(s));
        dfree(c, c->bm_scratch); c->bm_scratch_bytes = 0;
        ALLOC(c, c->bm_scratch, need);
        c->bm_scratch_bytes = need;
    }
    // the prompt: every beam row runs it (HF expands input_ids to batch x beams rows, _expand_inputs_for_generation); EOS handling is
    // the scorer's, so the device-side greedy rule is disabled (eos -1); its argmax tokens go to a dummy buffer and are ignored
    int rc = prefill_impl(c, ids, mask, rows, T, qformer_embs, 0, max_new, -1, pad_id, c->bm_out, c->bm_logits);
    if (rc) return rc;
    rc = build_graph(c, c->bm_logits, /*fixed=*/true);
    if (rc) return rc;

    std::vector<float> beam_scores(rows, -1e9f), cs((size_t)groups * K2);
    for (int g = 0; g < groups; ++g) beam_scores[(size_t)g * num_beams] = 0.f;
    std::vector<int> ci((size_t)groups * K2), next_tok(rows), src(2 * (size_t)rows);       // src[rows] | first differing cache position[rows]
    std::vector<std::vector<int>> hist(rows), nh(rows);
    std::vector<BeamHyps> hyps(groups);
    for (BeamHyps& h : hyps) { h.num_beams = num_beams; h.length_penalty = length_penalty; h.early_stopping = early_stopping; }
    std::vector<char> done(groups, 0);
    const bool full_copy = c->sw.beam_fullcopy != 0;     // tests: move every generated position (A/B leg)
    int cur_len = T, steps = 0;
    for (int step = 0; step < max_new; ++step) {
        HIPCHK(c, hipMemcpyAsync(c->bm_scores, beam_scores.data(), rows * sizeof(float), hipMemcpyHostToDevice, s));
        void* lp = step_scores ? (char*)step_scores + (size_t)step * rows * V * 2 : nullptr;
        launch_beam_topk(f.dtype, c->bm_logits, c->bm_scores, groups, num_beams, V, c->bm_cand_s, c->bm_cand_i, lp, s);
        HIPCHK(c, hipMemcpyAsync(cs.data(), c->bm_cand_s, cs.size() * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(ci.data(), c->bm_cand_i, ci.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        ++steps;
        // BeamSearchScorer.process
        for (int g = 0; g < groups; ++g) {
            const int r0 = g * num_beams;
            if (done[g]) {
                for (int b = 0; b < num_beams; ++b) { beam_scores[r0 + b] = 0.f; next_tok[r0 + b] = pad_id; src[r0 + b] = r0 + b; }
                continue;
            }
            int nb = 0;
            for (int rank = 0; rank < K2 && nb < num_beams; ++rank) {
                const float sc = cs[(size_t)g * K2 + rank];
                const int flat = ci[(size_t)g * K2 + rank], from = r0 + flat / V, tok = flat % V;
                if (eos_id >= 0 && tok == eos_id) {
                    if (rank >= num_beams) continue;
                    hyps[g].add(hist[from], cur_len, sc);
                } else {
                    beam_scores[r0 + nb] = sc; next_tok[r0 + nb] = tok; src[r0 + nb] = from;
                    ++nb;
                }
            }
            if (nb < num_beams) return fail(c, -7, "rdx_beam_search: fewer than %d live candidates in group %d (eos-only top-2k)", num_beams, g);
            done[g] = done[g] || hyps[g].is_done(cs[(size_t)g * K2], cur_len);
        }
        // _reorder_cache moves only what differs: row r's cache holds the positions of hist[r], its new parent's those of hist[src[r]];
        // both are token paths from the same prompt, so the common prefix is already in place (same tokens, same kernels, same launch)
        for (int r = 0; r < rows; ++r) {
            const std::vector<int>& mine = hist[r];
            const std::vector<int>& par = hist[src[r]];
            size_t cpre = 0;
            while (cpre < mine.size() && cpre < par.size() && mine[cpre] == par[cpre]) ++cpre;
            src[rows + r] = full_copy ? 0 : (T + (int)cpre) / 16 * 16;
        }
        for (int r = 0; r < rows; ++r) { nh[r] = hist[src[r]]; nh[r].push_back(next_tok[r]); }
        hist.swap(nh);
        ++cur_len;
        bool all_done = true;
        for (int g = 0; g < groups; ++g) all_done = all_done && done[g];
        if (all_done || cur_len >= T + max_new) break;
        // next forward: _reorder_cache (generated slots only -- the beams of a group share their prompt), chosen tokens in
        HIPCHK(c, hipMemcpyAsync(c->bm_src, src.data(), 2 * rows * sizeof(int), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(c->bm_tok, next_tok.data(), rows * sizeof(int), hipMemcpyHostToDevice, s));
        bool identity = true;
        for (int r = 0; r < rows; ++r) identity = identity && src[r] == r;
        if (step > 0 && !identity)
            launch_kv_beam_reorder(c->kcache, c->vcache, c->bm_scratch, c->bm_src, c->bm_src + rows, rows, f.heads, f.layers, f.max_len, c->kv_layer_elems * 2,
                                   p_lo, std::min((T + step + 15) / 16 * 16, p_lo + span), s);
        launch_embed_rows(f.dtype, c->bm_tok, c->embed, V, c->dx, rows, f.hidden, s);
        HIPCHK(c, hipGraphLaunch(c->graph, s));
    }
    HIPCHK(c, hipStreamSynchronize(s));
    HIPCHK(c, hipGetLastError());
    c->cur_steps = c->cur_max_new;
    int herr = 0;
    HIPCHK(c, hipMemcpy(&herr, c->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (herr) { hipMemset(c->d_err, 0, sizeof(int)); return fail(c, -5, "rdx_beam_search: a workgroup hand-off timed out inside a fused launch"); }
    // BeamSearchScorer.finalize: open beams of unfinished groups become hypotheses, the best one per group is returned
    for (int g = 0; g < groups; ++g) {
        if (!done[g]) for (int b = 0; b < num_beams; ++b) hyps[g].add(hist[(size_t)g * num_beams + b], cur_len, beam_scores[(size_t)g * num_beams + b]);
        int best = 0;                     // sorted(..., key = score) is stable and .pop() takes the last: the latest of equal scores
        for (int i = 1; i < (int)hyps[g].beams.size(); ++i) if (hyps[g].beams[i].score >= hyps[g].beams[best].score) best = i;
        const BeamHyp& h = hyps[g].beams[best];
        const int n = std::min((int)h.toks.size(), max_new);
        for (int i = 0; i < max_new; ++i) out_tokens_host[(size_t)g * max_new + i] = i < n ? h.toks[i] : pad_id;
        out_len_host[g] = n;
        if (out_score_host) out_score_host[g] = h.score;
    }
    if (n_steps_host) *n_steps_host = steps;
    return 0;
}
