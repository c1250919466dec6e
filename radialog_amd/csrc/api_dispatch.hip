// Host-side GEMM dispatch shared by the encoder and the decoder: which kernel family a shape goes to.
#include "rdx_ctx.h"

GemmArgs gargs(const void* X, int ldx, const GemmW& W, const float* bias, void* out, int ldo, int M) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.X = X; a.ldx = ldx; a.W = W.w; a.bias = bias; a.out = out; a.ldo = ldo;
    a.M = M; a.N = W.N; a.K = W.K; a.n_valid = W.N;
    a.W8 = W.w8; a.wscale = W.scale;
    return a;
}

// ---- the decode step's units: one definition each (rdx_ctx.h) ----
DecAttnArgs dec_attn_args(rdx_ctx* c, int layer) {
    const LlamaLayer& L = c->ll[layer];
    DecAttnArgs at;
    at.d = c->ld; at.qkv = c->dqkv; at.lbq = L.lora_bq; at.lbv = L.lora_bv; at.cos_t = c->rope_cos; at.sin_t = c->rope_sin;
    at.pos = c->d_pos; at.slot_b = c->d_slot; at.key_mask = c->key_mask; at.cur_rope = c->d_cur_rope;
    at.kcache = kv_ptr(c, c->kcache, layer); at.vcache = kv_ptr(c, c->vcache, layer); at.out = c->datt;
    return at;
}

void run_decode_attention(rdx_ctx* c, const DecAttnArgs& at, int layer, int B) {
    if (c->sw.kv_fp8) launch_decode_attention_kv8(c->cfg.dtype, at, kvx_ptr(c, c->kexp, layer), kvx_ptr(c, c->vexp, layer), B, attn_sw(c), c->stream);
    else launch_decode_attention(c->cfg.dtype, at, B, attn_sw(c), c->stream);
}

GemmArgs unit_args(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B) {
    const rdx_config& f = c->cfg;
    const int H = f.hidden;
    GemmArgs a;
    switch (u) {
    case UNIT_QKV: a = gargs(c->dx, H, L->wqkv, nullptr, c->dqkv, c->ld.qkv_ld, B); a.N = L->wqkv.Npad; a.norm_w = L->attn_norm; break;
    case UNIT_O: a = gargs(c->datt, H, L->wo, nullptr, c->dx, H, B); a.resid = c->dx; a.ldr = H; break;
    case UNIT_GATE_UP: a = gargs(c->dx, H, L->wgu, nullptr, c->dgu, f.inter, B); a.norm_w = L->mlp_norm; break;
    case UNIT_DOWN: a = gargs(c->dgu, f.inter, L->wdown, nullptr, c->dx, H, B); a.resid = c->dx; a.ldr = H; break;
    default:
        a = gargs(c->dx, H, c->lm_head, nullptr, nullptr, f.vocab, B);
        a.N = c->lm_head.Npad; a.n_valid = f.vocab; a.norm_w = c->final_norm; a.part_val = c->part_val; a.part_idx = c->part_idx;
    }
    if (a.norm_w) a.eps = f.rms_eps;
    return with_switches(c, a);
}

// ---- which copy of a weight each unit streams (rdx_ctx.h): THE table. The copies a family reads for a unit of a layer where the weight holds them, int4
// before coded; every other family and unit -- and every tile a copy's header flags -- reads the packed W. ----
static unsigned stream_wants(DecFamily fam, DecUnit u, int layer) {
    constexpr unsigned C = 1u << WS_CODED, Q = 1u << WS_W4;
    //                                  QKV    o_proj  gate/up  down_proj  lm_head (of a decode step; not quantised)
    static const unsigned chained[5] = {Q | C, 0,      Q | C,   Q | C,     C};        // batch <= 2; o_proj: hidden under the attention of the fused launch
    static const unsigned xs16[5]    = {Q,     0,      Q,       Q,         0};        // 3-16 rows: xstat16_w4_k / xrow16_w4_k
    // layer 0's QKV is the family's stand-alone launch (18.0 / 18.5 us raw, 18.7 / 18.6 coded: never coded); QKV of layers 1.. and down_proj: the chained launch
    if (fam == DEC_CHAINED) return u == UNIT_QKV && layer == 0 ? Q : chained[u];
    return fam == DEC_XS16 ? xs16[u] : 0;
}
// the table names copy s (coded or int4), its option is on (bf16 only) and W holds it
static bool can_stream(rdx_ctx* c, DecFamily fam, DecUnit u, int layer, const GemmW& W, WStream s) {
    if (!(stream_wants(fam, u, layer) >> s & 1) || c->cfg.dtype != DT_BF16) return false;
    return s == WS_W4 ? c->sw.w4 && W.w4 && W.w4h : c->sw.wcode && W.wc && W.wch;
}
WStream unit_stream(rdx_ctx* c, DecFamily fam, DecUnit u, int layer, const GemmW& W) {
    return can_stream(c, fam, u, layer, W, WS_W4) ? WS_W4 : can_stream(c, fam, u, layer, W, WS_CODED) ? WS_CODED : WS_RAW;
}
bool stream_wanted(DecUnit u, int layer, WStream s) {
    return ((stream_wants(DEC_CHAINED, u, layer) | stream_wants(DEC_XS16, u, layer)) >> s & 1) != 0;       // (the families with a row in the table)
}

static const GemmW& unit_weight(rdx_ctx* c, const LlamaLayer* L, DecUnit u) { return u == UNIT_QKV ? L->wqkv : u == UNIT_O ? L->wo : u == UNIT_GATE_UP ? L->wgu : u == UNIT_DOWN ? L->wdown : c->lm_head; }
// a stand-alone launch of unit u with the copy of its weight that family fam streams (QKV: the table's layer-0 entry, whichever layer's weight it is)
static GemmArgs with_stream(rdx_ctx* c, DecFamily fam, GemmArgs a, const LlamaLayer* L, DecUnit u) {
    const GemmW& W = unit_weight(c, L, u);
    const WStream s = unit_stream(c, fam, u, 0, W);
    if (s == WS_W4) { a.W4 = W.w4; a.w4hdr = W.w4h; }
    if (s == WS_CODED) { a.WC = W.wc; a.wchdr = W.wch; }
    return a;
}

GemmArgs chained_unit(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B) {
    return u == UNIT_DOWN ? unit_args(c, L, u, B) : with_stream(c, DEC_CHAINED, unit_args(c, L, u, B), L, u);       // (down_proj's entry is its role in chain_args)
}

GemmArgs xs16_unit(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B) {
    GemmArgs a = unit_args(c, L, u, B);
    if (u == UNIT_GATE_UP) a.out_packed = ACT_BLK32;
    if (u == UNIT_O || u == UNIT_DOWN) a.xpacked = ACT_BLK32;
    return with_stream(c, DEC_XS16, a, L, u);
}

ChainArgs chain_args(rdx_ctx* c, int l, int B) {
    const rdx_config& f = c->cfg;
    const LlamaLayer &L0 = c->ll[0], &L = c->ll[l];
    const LlamaLayer* Ln = l + 1 < f.layers ? &c->ll[l + 1] : nullptr;      // the last launch has no QKV role
    ChainArgs ca; memset(&ca, 0, sizeof(ca));
    ca.hidden = f.hidden; ca.inter = f.inter; ca.qkv_n = L0.wqkv.Npad; ca.qkv_ld = c->ld.qkv_ld; ca.B = B; ca.eps = f.rms_eps; ca.layer = l;
    ca.dx = c->dx; ca.dqkv = c->dqkv; ca.dgu = c->dgu; ca.ctr = c->d_cctr; ca.err = c->d_err; ca.naps = c->chain_naps;
    ca.w8 = (L0.wqkv.w8 && L0.wdown.w8 && f.hidden % 64 == 0 && f.inter % 64 == 0) ? 1 : 0;       // fp8 weights: the chained roles stream the e4m3 bytes too
    ca.wdown = L.wdown.w; ca.wdown8 = L.wdown.w8; ca.sdown = L.wdown.scale;
    if (Ln) { ca.wqkv = Ln->wqkv.w; ca.wqkv8 = Ln->wqkv.w8; ca.sqkv = Ln->wqkv.scale; ca.attn_norm = Ln->attn_norm; }
    // one copy per launch: int4 if both roles' weights hold a stream (decode_chain_w4_k), else coded if both hold a copy (decode_chain_wc_k), else the
    // packed weights; never beside the fp8 bytes. (The coded pointers travel whenever the copies exist, as they always have: wc = 0 reads none of them.)
    auto both = [&](WStream t) { return can_stream(c, DEC_CHAINED, UNIT_DOWN, l, L.wdown, t) && (!Ln || can_stream(c, DEC_CHAINED, UNIT_QKV, l + 1, Ln->wqkv, t)); };
    ca.wc = ca.w8 ? WS_RAW : both(WS_W4) ? WS_W4 : both(WS_CODED) ? WS_CODED : WS_RAW;
    const bool q = ca.wc == WS_W4;
    ca.cdown = q ? L.wdown.w4 : L.wdown.wc; ca.hdown = q ? L.wdown.w4h : L.wdown.wch;
    if (Ln) { ca.cqkv = q ? Ln->wqkv.w4 : Ln->wqkv.wc; ca.hqkv = q ? Ln->wqkv.w4h : Ln->wqkv.wch; }
    return ca;
}

GemmArgs blk_unit(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B) {
    GemmArgs a = unit_args(c, L, u, B);
    a.xpacked = ACT_TILES32; a.mtiles = (B + 15) / 16; a.out_packed = u == UNIT_GATE_UP ? ACT_TILES32 : ACT_ROWS;
    return a;
}

GemmArgs blk8_unit(rdx_ctx* c, const LlamaLayer* L, DecUnit u, int B) {
    GemmArgs a = unit_args(c, L, u, B);
    a.xpacked = (u == UNIT_O || u == UNIT_DOWN) ? ACT_BLK64 : ACT_BLK64_E4M3; a.mtiles = (B + 15) / 16; a.out_packed = u == UNIT_GATE_UP ? ACT_BLK64 : ACT_ROWS;
    a.xscale = c->dxs; a.xgroups = 1;
    return a;
}

GemmArgs ksplit_args(GemmArgs a) {
    a.xpacked = (a.W8 && a.wscale) ? ACT_BLK64 : ACT_BLK32;
    return a;
}

GemmArgs prenormed(rdx_ctx* c, GemmArgs a) {
    a.X = c->dxn; a.ldx = a.K; a.norm_w = nullptr;
    return a;
}

void run_rmsnorm(rdx_ctx* c, const NormArgs& n) {
    if (launch_rmsnorm(c->cfg.dtype, n, c->stream)) return;
    char buf[200];
    snprintf(buf, sizeof(buf), "RMSNorm: no kernel for %d x %d rows into layout %d (%d row tiles, %d slab groups%s)", n.rows, n.H, (int)n.layout, n.mtiles,
             n.slab ? n.groups : 0, n.w ? "" : ", no weight");
    c->unsupported = buf;
}

GemmArgs norm_in_front(rdx_ctx* c, GemmArgs a) {
    // a K-split projection before this unit left its residual epilogue to this RMSNorm: x += T(sum of slabs)
    const int pend = (a.X == c->dx) ? c->pend_groups : 0;
    if (pend) c->pend_groups = 0;
    run_rmsnorm(c, NormArgs{const_cast<void*>(a.X), a.norm_w, c->dxn, c->dxs, a.M, a.K, a.eps, a.xpacked, a.mtiles, pend ? c->kslab : nullptr, pend});
    return prenormed(c, a);
}

DecFamily decode_family(rdx_ctx* c, int B) {
    if (B > 32) return !blk64_ok(c, B) ? DEC_UNSUPPORTED : blk64_fp8(c) ? DEC_BLK8 : DEC_BLK;
    // batch <= 2: down(l) -> QKV(l+1) chained inside one launch by the fence-free hand-off, attention + o_proj in the fused launch
    if (c->sw.chain && c->sw.fuse_ao && chain_supported(c->ld, c->cfg.inter, B) && attn_oproj16_supported(c->ld, c->cfg.hidden, c->cfg.hidden, B))
        return DEC_CHAINED;
    return xs16_ok(c, B) ? DEC_XS16 : DEC_GENERIC;
}

// ---- the prompt's units (rdx_ctx.h): the family is decided once, every unit's arguments come from one builder in that family's layout ----
PromptPlan prompt_plan(rdx_ctx* c, int B, int T) {
    PromptPlan p;
    p.family = PROMPT_ROWS; p.M = B * T; p.mtiles = (p.M + 15) / 16; p.blk = p.down_split = false;
    const LlamaLayer* L = &c->ll[0];
    if (fp8_weights(L->wqkv)) { p.family = PROMPT_FP8; return p; }
    // few rows (one or two prompts): the projections are weight-stream bound -> weight-stationary kernels over fragment-packed
    // activations (wstat.hip); the producers (RMSNorm, attention, the SwiGLU epilogue) write that order directly
    constexpr int ws_maxm = 384;
    // measured (tools/prefill_only.py, 32 layers): wstat's time grows with the row tiles of 16, the 128-row tile GEMMs' with the row tiles of 128 --
    // M = 64: 4.84 vs 5.34 ms, 100: 6.06 / 6.26, 160: 7.30 / 7.64, 320: 11.43 / 11.92, but 250: 9.56 / 8.86. Take wstat when the 128-row
    // tiling would pad by 24 rows or more.
    constexpr int ws_minpad = 24;
    if (p.M <= 32 || p.M > ws_maxm || (p.M + 127) / 128 * 128 - p.M < ws_minpad) return p;
    p.family = PROMPT_TILES;
    const GemmArgs qkv = prompt_unit(c, p, L, UNIT_QKV), down = prompt_unit(c, p, L, UNIT_DOWN);
    if (!wstat_supported(qkv, EPI_NONE) || !wstat_supported(down, EPI_RESID)) { p.family = PROMPT_ROWS; return p; }
    // up to 192 rows the K = 4096 projections run activation-stationary in row blocks of 32 whose workgroups share an XCD's L2
    // (xstat32_k<.., BLK>: the weights cross each CU once per row block instead of the activations once per 32 columns); down_proj
    // (K = 11008) and longer prompts keep the weight-stationary kernel
    p.blk = c->sw.prompt_blk && xstat_blk_supported(qkv, EPI_NONE) && xstat_blk_supported(prompt_unit(c, p, L, UNIT_O), EPI_RESID) &&
            xstat_blk_supported(prompt_unit(c, p, L, UNIT_GATE_UP), EPI_SILU_MUL);
    // down_proj of a prompt of <= 128 rows (<= 4 row blocks: 160 rows measured 55.9 us against wstat_k 49.5; 64 rows 3.96 -> 3.69 ms per prefill) K-split over
    // 4 workgroups per tile into fp32 slabs (xsplit32_k<.., BLK>), combined (+ residual) by the next layer's RMSNorm -- after the last layer by one more norm
    // launch whose packed output nobody reads
    p.down_split = c->sw.prompt_blk && p.M <= 128 && xsplit_blk_supported(down);
    return p;
}

GemmArgs prompt_unit(rdx_ctx* c, const PromptPlan& p, const LlamaLayer* L, DecUnit u) {
    const rdx_config& f = c->cfg;
    const int H = f.hidden;
    const GemmW& W = unit_weight(c, L, u);
    GemmArgs a;
    switch (u) {
    case UNIT_QKV: a = gargs(c->pxn, H, W, nullptr, c->pqkv, c->ld.qkv_ld, p.M); a.N = W.Npad; break;
    case UNIT_O: a = gargs(c->patt, H, W, nullptr, c->px, H, p.M); a.resid = c->px; a.ldr = H; break;
    case UNIT_GATE_UP: a = gargs(c->pxn, H, W, nullptr, c->pgu, f.inter, p.M); break;
    default: a = gargs(c->pgu, f.inter, W, nullptr, c->px, H, p.M); a.resid = c->px; a.ldr = H;
    }
    switch (p.family) {
    case PROMPT_ROWS: break;
    case PROMPT_TILES: a.xpacked = ACT_TILES32; a.mtiles = p.mtiles; a.out_packed = u == UNIT_GATE_UP ? ACT_TILES32 : ACT_ROWS; break;
    case PROMPT_FP8:        // gemm8 over the e4m3 rows in pxq and whole weight tiles; the rows' scales: 1 K group behind an RMSNorm, 2 for o_proj, 4 for down_proj
        a.X = c->pxq; a.N = W.Npad; a.xscale = c->pxs; a.xgroups = u == UNIT_O ? 2 : u == UNIT_DOWN ? 4 : 1; a.ldr = H;
    }
    return with_switches(c, a);
}

void prompt_norm(rdx_ctx* c, const PromptPlan& p, const void* w, int pend) {
    const bool fp8 = p.family == PROMPT_FP8;        // quantised to e4m3 in the norm's epilogue
    run_rmsnorm(c, NormArgs{c->px, w, fp8 ? c->pxq : c->pxn, c->pxs, p.M, c->cfg.hidden, c->cfg.rms_eps,
                            fp8 ? ACT_ROWS_E4M3 : p.family == PROMPT_TILES ? ACT_TILES32 : ACT_ROWS, fp8 ? 0 : p.mtiles, pend ? c->pslab : nullptr, pend});
}

void prompt_attention(rdx_ctx* c, const PromptPlan& p, int l, int B, int T, int keep, int row0) {
    const rdx_config& f = c->cfg;
    const LlamaLayer& L = c->ll[l];
    const int H = f.hidden;
    hipStream_t s = c->stream;
    // where the layer's new K / V rows land (behind the kept slots) and what the attention reads: cache rows row0 .. of layer l ...
    LlamaDims d = c->ld;
    void *K = nullptr, *V = nullptr;
    if (!c->sw.kv_fp8) {
        const size_t kv_row = (size_t)row0 * f.heads * f.max_len * 128 * 2;
        K = (char*)kv_ptr(c, c->kcache, l) + kv_row; V = (char*)kv_ptr(c, c->vcache, l) + kv_row;
    } else {
        // ... fp8 KV cache: the one-layer staging buffer in the model dtype ([B][heads][ceil16(T)][128], row-major K), which is what the prompt's own attention
        // reads -- unquantised, so the prompt computes what a plain context computes -- and which is then quantised into the cache. Both kernels run unchanged
        // on dims and strides that describe the staging buffer. keep == 0 and row0 == 0 (prompt_refuse).
        K = c->kv_kstage; V = c->kv_vstage;
        d.max_len = (T + 15) / 16 * 16; d.k_perm = 0;
    }
    launch_rope_kv_prefill(f.dtype, d, c->pqkv, L.lora_bq, L.lora_bv, c->rope_cos, c->rope_sin, c->d_pos_ids, c->pq, K, V, B, T, keep, s);
    AttnArgs at;
    memset(&at, 0, sizeof(at));
    at.Q = c->pq; at.q_bs = (long)T * H; at.q_ts = H; at.q_hs = 128;
    at.K = K; at.V = V; at.key_mask = c->key_mask + (size_t)row0 * f.max_len;
    at.k_bs = at.v_bs = (long)f.heads * d.max_len * 128; at.k_ts = at.v_ts = 128; at.k_hs = at.v_hs = (long)d.max_len * 128;
    at.O = c->patt; at.o_bs = (long)T * H; at.o_ts = H; at.o_hs = 128;
    at.B = B; at.H = f.heads; at.Tq = T; at.Tk = keep + T; at.causal = 1; at.k_perm = d.k_perm; at.km_bs = f.max_len;
    at.flash_min = c->sw.flash_min;
    at.o_packed_mt = p.family == PROMPT_TILES ? p.mtiles : 0;
    launch_attention(f.dtype, 128, at, s);
    if (c->sw.kv_fp8)
        launch_kv8_quant_rows(f.dtype, K, V, d.max_len, kv_ptr(c, c->kcache, l), kvx_ptr(c, c->kexp, l), kv_ptr(c, c->vcache, l), kvx_ptr(c, c->vexp, l),
                              (size_t)B * f.heads, f.max_len, T, 0, s);
}

// Skinny GEMM with an optional fused RMSNorm: fused when the activations fit the GEMV's LDS stage; otherwise the RMSNorm runs as its own launch
// in front of it (norm_in_front). Returns the arguments of the GEMM proper (activations = c->dxn)
GemmArgs skinny_prenorm(rdx_ctx* c, GemmArgs a, int epi) {
    // (batch 3-4 rows would fit the GEMV's LDS stage with the norm fused, but the activation-stationary kernel behind a
    // stand-alone RMSNorm is faster there too: gate/up 41.7 -> 31 + 5 us at batch 4)
    if (!a.norm_w) return a;
    const bool xs = xstat32_supported(prenormed(c, a), epi);
    if (skinny_fits_lds(a.M, a.K) && !(a.M >= xs_min_rows() && c->kslab && xs)) return a;
    if (xs && a.W8 && a.wscale) {
        // fp8 weights: the normalised rows are quantised to e4m3 (one scale per row) in the consumer's 64-deep fragment order: fp8 x fp8 MFMA
        a.xpacked = ACT_BLK64_E4M3; a.xscale = c->dxs; a.xgroups = 1;
    } else if (xs) {
        a.xpacked = ACT_BLK32;       // the normalised rows go straight into the consumer's register-fragment order
    }
    return norm_in_front(c, a);
}

void skinny(rdx_ctx* c, GemmArgs a, int epi) {
    a = skinny_prenorm(c, with_switches(c, a), epi);
    if (!a.W && a.W8) {
        // fp8-only weights: the kernels that read e4m3 are the batch <= 2 GEMV with LDS-staged activations (expanded in registers) and, from
        // batch 3, the activation-stationary fp8 x fp8 kernel (K = 4096, many tiles). Anything else has no kernel in this mode.
        const bool gemv8 = skinny_fits_lds(a.M, a.K) && a.K % 64 == 0 && a.M < xs_min_rows();
        const bool xs8 = a.xpacked == ACT_BLK64_E4M3 && xstat32_supported(a, epi);
        if (!gemv8 && !xs8) {
            char buf[200];
            snprintf(buf, sizeof(buf), "fp8 weights: no kernel for a %d x %d x %d projection at this batch (batch <= 2: M K <= 16 Ki; batch 3-32: K = 4096)", a.M, a.N, a.K);
            c->unsupported = buf;
            return;
        }
    }
    ++c->n_stream[rdx_ctx::WK_GEMV][launch_skinny_gemm(c->cfg.dtype, a, epi, c->stream)];       // the launcher's own choice, counted
}

void launch_chain(rdx_ctx* c, int l, int B) {
    ChainArgs ca = chain_args(c, l, B);
    ca.trace = l == c->chain_trace_layer ? c->chain_trace : nullptr;
    ++c->n_stream[rdx_ctx::WK_CHAIN][ca.wc];
    launch_decode_chain(c->cfg.dtype, ca, l + 1 < c->cfg.layers, c->stream);
}

void launch_xs16(rdx_ctx* c, const GemmArgs& a, int epi) {
    const int dt = c->cfg.dtype;
    const bool row = epi == EPI_RESID, w4 = row ? xrow16_w4_supported(dt, a) : xstat16_w4_supported(dt, a, epi);
    ++c->n_stream[row ? rdx_ctx::WK_XROW16 : rdx_ctx::WK_XSTAT16][w4 ? WS_W4 : WS_RAW];
    if (row) { if (w4) launch_xrow16_w4(a, c->stream); else launch_xrow16(dt, a, c->stream); }
    else { if (w4) launch_xstat16_w4(a, epi, c->stream); else launch_xstat16(dt, a, epi, c->stream); }
}

int take_unsupported(rdx_ctx* c) {
    if (c->unsupported.empty()) return 0;
    const int rc = fail(c, -8, "%s", c->unsupported.c_str());
    c->unsupported.clear();
    return rc;
}

// batch 3-32 decode: gate/up (xstat32_k) can hand its SwiGLU output to down_proj fragment-packed, and down_proj then runs
// K-split over 4 workgroups per tile (xsplit32_k), its residual epilogue deferred to the next RMSNorm
bool down_split_ok(rdx_ctx* c, const LlamaLayer& L, int B) {
    if (B < xs_min_rows() || !c->kslab) return false;
    if (!xstat32_supported(prenormed(c, unit_args(c, &L, UNIT_GATE_UP, B)), EPI_SILU_MUL)) return false;
    return xsplit32_groups(ksplit_args(unit_args(c, &L, UNIT_DOWN, B))) > 0;
}

// A K-split projection (o_proj, down_proj at batch 3-32): its fp32 slabs stay pending for the stand-alone RMSNorm of the
// projection that follows (norm_in_front), which adds them, rounds and applies the residual.
// (fp8 weights: W8A16 -- the e4m3 weight fragments are expanded in registers and multiply the producer's model-dtype activation fragments)
void launch_ksplit(rdx_ctx* c, const GemmArgs& a) {
    launch_xsplit32(c->cfg.dtype, a, c->kslab, c->stream);
    c->pend_groups = xsplit32_groups(a);
}

void launch_down(rdx_ctx* c, const LlamaLayer& L, int B, bool split) {
    const GemmArgs a = unit_args(c, &L, UNIT_DOWN, B);
    if (split) launch_ksplit(c, ksplit_args(a));
    else skinny(c, a, EPI_RESID);
}

// 33-128 rows (round 5; VERDICT r4 "missing" 3): the decoder's rows as NB = ceil(rows / 32) blocks of 32. Every K = 4096 projection runs activation-stationary per block,
// the two block workgroups of a tile walker on one XCD (xstat32_k<.., BLK>: a weight fragment comes from HBM once, from that L2 once more); o_proj is
// un-split (final rows: no slabs), down_proj (K = 11008) K-split into fp32 slabs (or, "blk_down" off, on the prompt's weight-stationary kernel); the RMSNorms write the
// fragment-packed [k / 32][row tiles][lane][8] the consumers read. fp8 weights (blk64_fp8) take the 32-row fp8 kernels per row block instead.
bool blk64_fp8(rdx_ctx* c) { return !c->ll.empty() && fp8_weights(c->ll[0].wqkv); }

bool blk64_ok(rdx_ctx* c, int B) {
    if (B <= 32 || B > RDX_MAX_ROWS || c->ll.empty() || c->cfg.hidden != 4096) return false;
    const LlamaLayer* L = &c->ll[0];
    if (blk64_fp8(c)) {
        // fp8 weights (round 5): the 32-row fp8 kernels per row block -- e4m3 blocks + xscale for QKV / gate-up / lm_head (fp8 x fp8); o_proj and down_proj K-split
        // over model-dtype activation blocks (xsplit32_k<.., BLK>: W8A16), slabs combined by the next RMSNorm
        return c->kslab && c->dxs && xstat_blk8_supported(prenormed(c, blk8_unit(c, L, UNIT_QKV, B)), EPI_NONE) && xsplit_blk8_groups(blk8_unit(c, L, UNIT_O, B)) == 2 &&
               xstat_blk8_supported(prenormed(c, blk8_unit(c, L, UNIT_GATE_UP, B)), EPI_SILU_MUL) && xsplit_blk8_groups(blk8_unit(c, L, UNIT_DOWN, B)) == 4 &&
               xstat_blk8_supported(prenormed(c, blk8_unit(c, L, UNIT_LM_HEAD, B)), EPI_LOGITS);
    }
    return xstat_blk_supported(prenormed(c, blk_unit(c, L, UNIT_QKV, B)), EPI_NONE) && xstat_blk_supported(blk_unit(c, L, UNIT_O, B), EPI_RESID) &&
           xstat_blk_supported(prenormed(c, blk_unit(c, L, UNIT_GATE_UP, B)), EPI_SILU_MUL) && wstat_supported(blk_unit(c, L, UNIT_DOWN, B), EPI_RESID) &&
           xstat_blk_supported(prenormed(c, blk_unit(c, L, UNIT_LM_HEAD, B)), EPI_LOGITS);
}

bool xs16_ok(rdx_ctx* c, int B) {
    if (!c->sw.xs16 || !xs16_rows_ok(B) || c->ll.empty()) return false;
    const LlamaLayer* L = &c->ll[0];
    return xstat16_supported(xs16_unit(c, L, UNIT_QKV, B), EPI_NONE) && xstat16_supported(xs16_unit(c, L, UNIT_GATE_UP, B), EPI_SILU_MUL) &&
           xstat16_supported(xs16_unit(c, L, UNIT_LM_HEAD, B), EPI_LOGITS) && xrow16_supported(xs16_unit(c, L, UNIT_O, B)) && xrow16_supported(xs16_unit(c, L, UNIT_DOWN, B));
}

void run_gemm(rdx_ctx* c, GemmArgs a, int epi) {
    if (!a.W && a.W8 && a.M > 32) { c->unsupported = "fp8 weights: this GEMM has no fp8 kernel (only the Llama projections are quantised)"; return; }
    ConvGeom cg;
    memset(&cg, 0, sizeof(cg));
    if (a.M <= 32) skinny(c, a, epi == EPI_RESID_RELU ? EPI_RESID : epi);
    else if (c->ws_ok && c->zero16 && wsgemm_supported(a, cg, epi))
        launch_wsgemm(c->cfg.dtype, a, cg, epi, c->zero16, c->sw.ws_cfg, c->stream);       // the encoder's short-K residual GEMMs
    else if (gemm_dma_supported(a)) launch_gemm_dma(c->cfg.dtype, a, epi, c->gemm_ws, c->gemm_ws_floats, c->stream);
    else launch_tiled_gemm(c->cfg.dtype, a, cg, epi, c->stream);
}

// side of the trunk's output grid: conv1 /2, maxpool /2, then three stride-2 stages of (g - 1) / 2 + 1 (3x3 pad 1 and the
// 1x1 downsample agree): 448 -> 14, 488 -> 16
int v_grid(const rdx_config& f) {
    int g = f.v_img / 4;
    for (int i = 0; i < 3; ++i) g = (g - 1) / 2 + 1;
    return g;
}

void conv_gemm(rdx_ctx* c, const void* X, const GemmW& W, const float* bias, const void* resid, void* out, int B,
                      int Hin, int Win, int Cin, int KH, int KW, int stride, int pad, int Hout, int Wout, int epi) {
    GemmArgs a = gargs(X, Cin, W, bias, out, W.N, B * Hout * Wout);
    a.resid = resid; a.ldr = W.N;
    ConvGeom cg;
    cg.mode = 1; cg.Hin = Hin; cg.Win = Win; cg.Cin = Cin; cg.Hout = Hout; cg.Wout = Wout;
    cg.KH = KH; cg.KW = KW; cg.stride = stride; cg.pad = pad;
    if (KH == 1 && KW == 1 && stride == 1 && pad == 0) cg.mode = 0;
    // memory-bound 1x1 convolutions (K <= 256, tens of thousands of rows): weight-stationary streaming kernel
    if (conv1x1_stream_supported(a, cg, epi)) { launch_conv1x1_stream(c->cfg.dtype, a, cg, epi, c->stream); return; }
    if (c->ws_ok && c->zero16 && wsgemm_supported(a, cg, epi)) { launch_wsgemm(c->cfg.dtype, a, cg, epi, c->zero16, c->sw.ws_cfg, c->stream); return; }
    // 1x1 stride-1 convolutions are plain GEMMs; everything else needs the gather path of the tiled kernel
    if (cg.mode == 0 && gemm_dma_supported(a)) launch_gemm_dma(c->cfg.dtype, a, epi, c->gemm_ws, c->gemm_ws_floats, c->stream);
    else if (c->zero16 && !resid && gemm_dma_conv_supported(a, cg, epi)) launch_gemm_dma_conv(c->cfg.dtype, a, cg, epi, c->zero16, c->gemm_ws, c->gemm_ws_floats, c->stream);
    else launch_tiled_gemm(c->cfg.dtype, a, cg, epi, c->stream);
}

