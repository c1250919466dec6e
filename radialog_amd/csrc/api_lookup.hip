// librdx C ABI, part 3b: prompt-lookup decoding (include/rdx.h: rdx_set_lookup / rdx_generate_lookup) -- batch-1 greedy decode whose drafts come from the
// sequence itself and are verified by passes of the append path. The device side is ONE kernel, lookup_accept_k (lookup.hip), behind every lm_head.
#include "rdx_ctx.h"

static const rdx_lookup k_lookup_off = {0, 0, 0};

extern "C" int rdx_set_lookup(rdx_ctx* c, const rdx_lookup* lk) {
    if (!c) return -1;
    if (!lk || lk->draft_len == 0) { c->lookup = k_lookup_off; return 0; }
    const rdx_lookup v = *lk;
    if (v.draft_len < 1 || v.draft_len > LOOKUP_MAX_DRAFT) return fail(c, -1, "rdx_set_lookup: draft_len %d outside [1, %d] (0 = off)", v.draft_len, LOOKUP_MAX_DRAFT);
    if (v.ngram_max < 1 || v.ngram_max > LOOKUP_MAX_NGRAM) return fail(c, -1, "rdx_set_lookup: ngram_max %d outside [1, %d]", v.ngram_max, LOOKUP_MAX_NGRAM);
    if (v.ngram_min < 1 || v.ngram_min > v.ngram_max) return fail(c, -1, "rdx_set_lookup: ngram_min %d outside [1, ngram_max = %d]", v.ngram_min, v.ngram_max);
    if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "rdx_set_lookup: llama weights not finalized");
    const rdx_config& f = c->cfg;
    HIPCHK(c, hipSetDevice(c->device));
    // each buffer on its own: a call that failed half way leaves the option as it was, and the next one allocates what is still missing
    constexpr size_t rows = LOOKUP_MAX_DRAFT + 1;
    if (!c->d_hist) ALLOC(c, c->d_hist, (size_t)f.max_batch * f.max_len * sizeof(int));
    if (!c->d_hist_len) {
        ALLOC(c, c->d_hist_len, (size_t)f.max_batch * sizeof(int));
        HIPCHK(c, hipMemset(c->d_hist_len, 0, (size_t)f.max_batch * sizeof(int)));
    }
    if (!c->lk_tail) ALLOC(c, c->lk_tail, rows * sizeof(int));
    if (!c->lk_status) ALLOC(c, c->lk_status, LKS_INTS * sizeof(int));
    if (!c->lk_trace) ALLOC(c, c->lk_trace, (size_t)f.max_len * 2 * sizeof(int));
    if (!c->lk_par) ALLOC(c, c->lk_par, LKP_INTS * sizeof(int));
    if (!c->lk_part_val) ALLOC(c, c->lk_part_val, rows * c->n_vtiles * sizeof(float));
    if (!c->lk_part_idx) ALLOC(c, c->lk_part_idx, rows * c->n_vtiles * sizeof(int));
    if (!c->lk_logits) ALLOC(c, c->lk_logits, rows * (size_t)f.vocab * 2);
    if (!c->lk_corpus) { ALLOC(c, c->lk_corpus, 1024 * sizeof(int)); c->lk_corpus_cap = 1024; }
    c->lookup = v;
    return 0;
}

// the corpus buffer grows like the prompt's workspaces: drain, release, allocate; the step graph's key holds its address
static int ensure_corpus(rdx_ctx* c, size_t n) {
    if (n <= c->lk_corpus_cap) return 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->lk_corpus_cap = 0;
    dfree(c, c->lk_corpus);
    const size_t cap = (n + 1023) & ~(size_t)1023;
    ALLOC(c, c->lk_corpus, cap * sizeof(int));
    c->lk_corpus_cap = cap;
    return 0;
}

void lookup_accept(rdx_ctx* c, StepTail t, int d, const float* pv, const int* pi, const void* logits) {
    t.hist = c->d_hist; t.hist_len = c->d_hist_len; t.hist_ld = c->cfg.max_len;
    LookupArgs a;
    a.part_val = pv; a.part_idx = pi; a.n_tiles = c->n_vtiles; a.d = d;
    a.logits = logits; a.scores = logits ? c->lk_scores : nullptr;
    a.tail = c->lk_tail; a.slot = c->d_slot; a.pos_ids = c->d_pos_ids; a.img_pos = c->d_img_pos;
    a.status = c->lk_status; a.trace = c->lk_trace; a.trace_cap = c->cfg.max_len;
    a.par = c->lk_par; a.corpus = c->lk_corpus;
    launch_lookup_accept(c->cfg.dtype, a, t, c->stream);
}

// One verify pass: the d + 1 tail tokens the last lookup_accept_k left (ids in lk_tail, position ids in d_pos_ids) through the prompt's layer loop behind
// `keep` kept slots -- their K / V rows land at slots keep .. keep + d --, then the final RMSNorm and the lm_head over all d + 1 rows, then the accept kernel.
// Slots behind the accepted ones keep the rejected drafts' rows. Nothing reads them before they are overwritten, and it is the SLOT BOUND that makes this
// true, not the key mask (prep_prompt_k sets the mask of every slot >= T to 1 once): decode attention reads keys [0, slot_b] only (attn_body.h: nk = slot + 1)
// and writes slot_b itself first; the append attention of a later pass reads keys [0, keep + T) causally, all of them rewritten by that pass from `keep` on.
static void verify_pass(rdx_ctx* c, int d, int keep) {
    const rdx_config& f = c->cfg;
    const int M = d + 1, H = f.hidden;
    prompt_embed_layers(c, c->lk_tail, 1, M, keep, /*splice=*/false, 0);
    run_rmsnorm(c, NormArgs{c->px, c->final_norm, c->pxn, nullptr, M, H, f.rms_eps, ACT_ROWS, 0, nullptr, 0});
    void* rows = c->lk_scores ? c->lk_logits : nullptr;
    GemmArgs a = gargs(c->pxn, H, c->lm_head, nullptr, rows, f.vocab, M);
    a.N = c->lm_head.Npad; a.n_valid = f.vocab; a.part_val = c->lk_part_val; a.part_idx = c->lk_part_idx;
    skinny(c, a, EPI_LOGITS);
    lookup_accept(c, step_tail_args(c, /*advance=*/1), d, c->lk_part_val, c->lk_part_idx, rows);
}

extern "C" int rdx_generate_lookup(rdx_ctx* c, const int32_t* ids, const int32_t* mask, int B, int T, const float* qformer_embs, const int32_t* corpus_host,
                                   int n_corpus, int max_new, int eos_id, int pad_id, int32_t* out_tokens, void* scores, int* n_tokens_host, int* stats_host,
                                   int* trace_host, int trace_cap) {
    if (!c) return -1;
    const char* who = "rdx_generate_lookup";
    // every refusal stands in front of the first effect: the conversation the call would have replaced stays as it was
    if (int src = rows_refuse(c, who)) return src;
    if (!c->finalized || !c->cfg.enable_llama) return fail(c, -1, "%s: llama weights not finalized", who);
    const rdx_config& f = c->cfg;
    if (c->lookup.draft_len <= 0) return fail(c, -1, "%s: the lookup option is off; rdx_set_lookup first", who);
    if (B != 1) return fail(c, -1, "%s: batch %d: prompt-lookup decoding is built for batch 1 only", who, B);
    if (c->rules_on) return fail(c, -1, "%s: not available under logits rules (a pass would have to process every row's logits); rdx_set_logits_rules(ctx, NULL) first", who);
    if (c->sampling.do_sample) return fail(c, -1, "%s: not available while sampling is on (speculative sampling is not built); rdx_set_sampling(ctx, NULL) first", who);
    if (c->logprobs >= 0) return fail(c, -1, "%s: not available while the logprobs option is on; rdx_set_logprobs(ctx, -1) first", who);
    if (int krc = kv8_refuse(c, who, "the kept prefix is not held in the model dtype")) return krc;
    if (fp8_weights(c->ll[0].wqkv) || fp8_weights(c->lm_head))
        return fail(c, -1, "%s: not available on an fp8-weight context (the all-row lm_head of a pass needs a quantisation convention the oracle does not define below batch 3)", who);
    if (max_new <= 0) return fail(c, -1, "%s: max_new must be positive", who);
    if (!ids || !out_tokens || !n_tokens_host || !stats_host) return fail(c, -1, "%s: null ids / out_tokens / n_tokens_host / stats_host", who);
    if (T <= 0 || T + max_new > f.max_len) return fail(c, -1, "%s: T (%d) + max_new (%d) exceeds max_len %d", who, T, max_new, f.max_len);
    if (T + max_new > f.max_pos) return fail(c, -1, "%s: sequence exceeds max_position_embeddings %d", who, f.max_pos);
    if (qformer_embs && T < 32) return fail(c, -1, "%s: image splice needs T >= 32", who);
    if (n_corpus < 0 || (n_corpus > 0 && !corpus_host)) return fail(c, -1, "%s: n_corpus %d without a corpus", who, n_corpus);
    if (trace_host && trace_cap < 0) return fail(c, -1, "%s: negative trace_cap", who);
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_corpus(c, (size_t)n_corpus)) return rc;
    hipStream_t s = c->stream;
    if (n_corpus) HIPCHK(c, hipMemcpyAsync(c->lk_corpus, corpus_host, (size_t)n_corpus * sizeof(int), hipMemcpyHostToDevice, s));
    int* par = c->lk_par_host;
    par[LKP_NCORPUS] = n_corpus; par[LKP_DRAFT_LEN] = c->lookup.draft_len; par[LKP_NGRAM_MAX] = c->lookup.ngram_max; par[LKP_NGRAM_MIN] = c->lookup.ngram_min;
    par[LKP_SLOT_END] = T + max_new;
    HIPCHK(c, hipMemcpyAsync(c->lk_par, par, LKP_INTS * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));      // the corpus is the caller's host memory

    struct Run {        // the selection is lookup_accept_k for the length of this call, on every return path
        rdx_ctx* c;
        Run(rdx_ctx* c_, void* sc) : c(c_) { c->lk_run = true; c->lk_scores = sc; }
        ~Run() { c->lk_run = false; c->lk_scores = nullptr; }
    } run(c, scores);

    // the prefill as in rdx_generate: token 0, the history, and -- from the accept kernel behind its lm_head -- the first draft
    if (int rc = prefill_impl(c, ids, mask, 1, T, qformer_embs, 0, max_new, eos_id, pad_id, out_tokens, scores)) return rc;
    int st[2] = {0, 0};
    auto status = [&]() -> int {        // the per-forward host traffic: 8 bytes and one sync
        HIPCHK(c, hipMemcpyAsync(st, c->lk_status, sizeof(st), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        return 0;
    };
    if (int rc = status()) return rc;
    int forwards = 0;
    bool graph_ready = false;
    while (!(st[LKS_NEXT] >> 8) && forwards < max_new) {
        const int d = st[LKS_NEXT] & 0xff;
        if (d == 0) {
            if (!graph_ready) { if (int rc = build_graph(c, scores)) return rc; graph_ready = true; }
            HIPCHK(c, hipGraphLaunch(c->graph, s));
        } else {
            verify_pass(c, d, st[LKS_SLOT]);
            if (int urc = take_unsupported(c)) return urc;
        }
        ++forwards;
        if (int rc = status()) return rc;
    }
    HIPCHK(c, hipGetLastError());
    int n = 0;
    HIPCHK(c, hipMemcpy(&n, c->d_step, sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int> tr((size_t)forwards * 2);
    if (forwards) HIPCHK(c, hipMemcpy(tr.data(), c->lk_trace, tr.size() * sizeof(int), hipMemcpyDeviceToHost));
    stats_host[0] = stats_host[1] = stats_host[2] = 0;
    for (int i = 0; i < forwards; ++i) {
        if (tr[2 * i] > 0) { ++stats_host[0]; stats_host[1] += tr[2 * i]; stats_host[2] += tr[2 * i + 1]; }
        if (trace_host && i < trace_cap) { trace_host[2 * i] = tr[2 * i]; trace_host[2 * i + 1] = tr[2 * i + 1]; }
    }
    *n_tokens_host = n;
    c->cur_steps = n;        // an ordinary conversation of n steps: the single-step calls continue it while n < max_new
    int herr = 0;
    HIPCHK(c, hipMemcpy(&herr, c->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (herr) {
        hipMemset(c->d_err, 0, sizeof(int));
        return fail(c, -5, "%s: a workgroup hand-off timed out inside a fused/chained launch (results invalid)", who);
    }
    return 0;
}
