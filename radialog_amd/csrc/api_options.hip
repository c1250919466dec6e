// librdx C ABI, the runtime switches: ONE table. Every switch of the library is one row of `rows`; its environment variable is read once, at rdx_create
// (options_from_env), into rdx_ctx::sw; after that only rdx_set_option changes it, per context. No launcher, dispatch function or entry point reads the
// environment. (INTEGRATION.md "Runtime switches" is this table for the caller; tests/test_gpu_options.py holds the two against each other.)
#include <limits.h>

#include "rdx_ctx.h"

namespace {

enum Kind { BOOL, INT, LETTER };        // BOOL: stored as value != 0. INT: refused outside [lo, hi]. LETTER: an INT whose environment variable may also say 'A' + value - 1
enum When { ANY_TIME, PRE_FINAL };      // PRE_FINAL: rdx_finalize_weights allocates or lays out by it; refused afterwards

struct Row {
    const char* name;       // of rdx_set_option / rdx_get_option
    const char* env;        // read at rdx_create, or null
    int Switches::*field;
    Kind kind;
    int def, lo, hi;
    When when;
    bool drops_graph;       // a captured step graph holds the launches the old value chose
    const char* values;     // what the numbers mean: the tail of the out-of-range message
};

// A switch that gained its option name here (fuse_ao, chain, blk_down, pconv_ksplit, and the ones that were environment-only) is ANY_TIME where every consumer reads it
// when it launches and no allocation depends on it; the row says which consumers those are.
const Row rows[] = {
    // batch <= 2: attention and o_proj as ONE 16-wave launch with a fence-free hand-off (chain.hip attn_oproj16_k), or 0: two launches. Read per step by decode_family / attn_oproj
    {"fuse_ao", "RDX_FUSE_AO", &Switches::fuse_ao, BOOL, 1, 0, 1, ANY_TIME, true, ""},
    // batch <= 2: down(l) -> QKV(l+1) as one chained launch, one workgroup per CU (chain.hip decode_chain_k), or 0: one kernel per unit. Read per step (decode_family, the step tail's counter reset)
    {"chain", "RDX_CHAIN", &Switches::chain, BOOL, 1, 0, 1, ANY_TIME, true, ""},
    // batched causal prefill attention: flash_prefill_k from this many 64-query workgroups
    {"flash_min", "RDX_FLASH_MIN", &Switches::flash_min, INT, 512, INT_MIN, INT_MAX, ANY_TIME, false, "0 = never, 1 = always"},
    // batch 3-16 decode on the one-row-tile family (xs16.hip: norm-prologue projections + un-split o_proj / down, 5 launches per layer), or 0: the 32-row family of xstat32.hip (7 launches)
    {"xs16", "RDX_XS16", &Switches::xs16, BOOL, 1, 0, 1, ANY_TIME, true, ""},
    // one prompt's K = 4096 projections on xstat32_k<.., BLK> and its K-split down_proj, or 0: wstat_k
    {"prompt_blk", "RDX_PBLK", &Switches::prompt_blk, BOOL, 1, 0, 1, ANY_TIME, false, ""},
    // 33-128 rows, model-dtype weights: down_proj K-split into fp32 slabs (xsplit32_k<.., BLK>), or 0: wstat_k. Read per step by step_blk; the slabs exist either way
    {"blk_down", "RDX_BLK_DOWN", &Switches::blk_down, BOOL, 1, 0, 1, ANY_TIME, true, ""},
    // the ResNet trunk and the Q-Former GEMMs on fragment-packed activations (pconv.hip), or 0: the row-major kernels
    {"pconv", "RDX_PCONV", &Switches::pconv, BOOL, 1, 0, 1, ANY_TIME, false, ""},
    // pconv_k may split K inside a workgroup, or 0: never. Read per encoder launch (PConvArgs::no_ksplit); the encoder is in no captured graph
    {"pconv_ksplit", "RDX_PCONV_KSPLIT", &Switches::pconv_ksplit, BOOL, 1, 0, 1, ANY_TIME, false, ""},
    // the K cache in the fragment order of decode attention: rdx_finalize_weights resolves -1 to max_batch * heads <= 256 and lays the cache out by it
    {"kperm", "RDX_KPERM", &Switches::kperm, INT, -1, -1, 1, PRE_FINAL, false, "-1 = by max_batch * heads, 0 = row-major, 1 = fragment order"},
    // batch <= 2 chained family, bf16: gate/up, down_proj, QKV and the lm_head stream their coded copy (GemmW::wc), or 0: the raw packed one; same bits
    {"wcode", nullptr, &Switches::wcode, BOOL, 1, 0, 1, ANY_TIME, true, ""},
    // ... their int4 stream (GemmW::w4) where the weight has one, and so do QKV, gate/up and down_proj of the 3-16-row family, or 0: the packed bf16 bytes of W'; same bits
    {"w4", nullptr, &Switches::w4, BOOL, 1, 0, 1, ANY_TIME, true, ""},
    // the decoder's KV cache as e4m3 codes + one power-of-two exponent per row (radialog_amd/kv8.py)
    {"kv_fp8", nullptr, &Switches::kv_fp8, BOOL, 0, 0, 1, PRE_FINAL, false, ""},
    // rdx_score: logits rows per lm_head launch (profiles/r11_score.md)
    {"score_chunk", nullptr, &Switches::score_chunk, INT, 2048, 0, INT_MAX, ANY_TIME, false, "0 = all rows at once"},
    // decode attention's build, forced (tests). Read per launch by the launchers of attn.hip through DecAttnSw
    {"att_tp", "RDX_ATT_TP", &Switches::att_tp, INT, 0, 0, 2, ANY_TIME, true, "0 = by heads x rows, 1 = the 4-wave throughput build, 2 = the 8-wave one"},
    // 257-512 (head, row) pairs take the 8-wave build, or 0: the 4-wave one (A/B). Read per launch, like att_tp
    {"att_mid", "RDX_ATT_MID", &Switches::att_mid, BOOL, 1, 0, 1, ANY_TIME, true, ""},
    // the padding rows of a 32-row block re-read real rows, or 0: they load their own lines (A/B). Read per launch into GemmArgs::xdup_off
    {"xdup", "RDX_XDUP", &Switches::xdup, BOOL, 1, 0, 1, ANY_TIME, true, ""},
    // wsgemm_k's tile shape, forced (tests; RDX_WS_CFG also takes the letter). Read per encoder launch
    {"ws_cfg", "RDX_WS_CFG", &Switches::ws_cfg, LETTER, 0, 0, 5, ANY_TIME, false, "0 = by shape, 1..5 = tile shapes A..E"},
    // rdx_beam_search moves every generated position of a re-ordered beam, not only those that differ (A/B). Read per call, on the host
    {"beam_fullcopy", "RDX_BEAM_FULLCOPY", &Switches::beam_fullcopy, BOOL, 0, 0, 1, ANY_TIME, false, ""},
    // rdx_generate polls the rows' EOS flags every this many steps. Read per call, on the host
    {"eos_poll", "RDX_EOS_POLL", &Switches::eos_poll, INT, 4, INT_MIN, INT_MAX, ANY_TIME, false, "<= 0 = 4"},
};
constexpr int n_rows = (int)(sizeof(rows) / sizeof(rows[0]));

const Row* find(const char* name) {
    for (const Row& r : rows) if (!strcmp(name, r.name)) return &r;
    return nullptr;
}

// v as row r stores it, or the message of a value outside its range
int checked(rdx_ctx* c, const char* who, const Row& r, int v, int* out) {
    if (r.kind == BOOL) v = v != 0;
    else if (v < r.lo || v > r.hi) {
        if (r.lo == 0 && v < 0) return fail(c, -1, "%s: %s %d is negative (%s)", who, r.name, v, r.values);
        return fail(c, -1, "%s: %s %d is outside [%d, %d] (%s)", who, r.name, v, r.lo, r.hi, r.values);
    }
    *out = v;
    return 0;
}

void drop_graph(rdx_ctx* c) { if (c->graph) { hipGraphExecDestroy(c->graph); c->graph = nullptr; c->gkey = GraphKey(); } }

}  // namespace

int options_from_env(rdx_ctx* c) {
    for (const Row& r : rows) {
        c->sw.*r.field = r.def;
        const char* e = r.env ? getenv(r.env) : nullptr;
        if (!e) continue;
        const bool letter = r.kind == LETTER && *e >= 'A' && *e < 'A' + r.hi;
        if (int rc = checked(c, r.env, r, letter ? *e - 'A' + 1 : atoi(e), &(c->sw.*r.field))) return rc;
    }
    return 0;
}

extern "C" int rdx_set_option(rdx_ctx* c, const char* name, int value) {
    if (!c || !name) return -1;
    const Row* r = find(name);
    if (!r) return fail(c, -1, "rdx_set_option: unknown option '%s'", name);
    if (r->when == PRE_FINAL && c->finalized) return fail(c, -1, "rdx_set_option: %s decides what rdx_finalize_weights allocates; set it before that call", name);
    if (int rc = checked(c, "rdx_set_option", *r, value, &(c->sw.*r->field))) return rc;
    if (r->drops_graph) drop_graph(c);
    return 0;
}

extern "C" int rdx_get_option(rdx_ctx* c, const char* name, int* value) {
    if (!c || !name || !value) return -1;
    const Row* r = find(name);
    if (!r) return fail(c, -1, "rdx_get_option: unknown option '%s'", name);
    *value = c->sw.*r->field;
    return 0;
}

extern "C" const char* rdx_option_name(int index) { return index >= 0 && index < n_rows ? rows[index].name : nullptr; }
