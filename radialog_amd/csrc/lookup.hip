// Prompt-lookup decoding (include/rdx.h: rdx_generate_lookup): what follows the lm_head of one forward over the rows [last emitted token, draft_1 .. draft_d].
#include "../../include/rdx.h"
#include "rdx_common.h"

namespace rdx {

// ---- lookup_accept_k: ONE workgroup of 256 threads for the one sequence, behind the lm_head launch (plain loads) -----------------------------------------
// 1. Row r's argmax from its [n_tiles] partials: thread t takes the tiles t, t + 256, .. in that order, a fixed 256-leaf LDS tree joins them; ties go to the
//    lowest index (greedy_step_k's reduction, once per row), so d == 0 selects the token greedy_step_k selects.
// 2. Thread 0 applies the accept rule (a draft is accepted while argmax_j == draft_{j+1}), walks the a + 1 emitted tokens through the EOS / pad rule of
//    step_tail (an EOS ends the emission), writes them to out_tokens and the history, and advances step / slot / position by the number emitted.
// 3. All threads: the emitted rows of the pass's logits into `scores`, pads behind an EOS, the next plain step's input embedding and cos | sin row, and the
//    draft rule for the next forward over H = corpus | history: for n = ngram_max .. ngram_min the LARGEST start j with H[j .. j+n) == the last n tokens and
//    j + n < len(H) -- thread t tests the starts len - n - 1 - t, - 256, .. downwards and stops at its first hit, an integer maximum joins the threads.
// The history entries thread 0 appended are read back by the other threads behind a workgroup barrier (same CU, same L1: visible).
// No scratch, 2.3 KB of LDS; the serial part is at most 16 tokens long.
__device__ __forceinline__ int lk_h(const int* __restrict__ corpus, int nc, const int* __restrict__ hist, int i) { return i < nc ? corpus[i] : hist[i - nc]; }

template <typename T>
__global__ __launch_bounds__(256) void lookup_accept_k(LookupArgs a, StepTail t) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ int am[LOOKUP_MAX_DRAFT + 1];
    __shared__ int pat[LOOKUP_MAX_NGRAM];
    __shared__ int n_s, step0_s, pos_s, slot_s, tok_s, fin_s, eos_s, hlen_s;
    const int tid = threadIdx.x;
    const int d = a.d < 0 ? 0 : (a.d > LOOKUP_MAX_DRAFT ? LOOKUP_MAX_DRAFT : a.d);
    if (t.ctr_zero) for (int i = tid; i < t.n_zero; i += 256) t.ctr_zero[i] = 0;       // the next plain step's hand-off counters (greedy_step_k does the same)

    for (int r = 0; r <= d; ++r) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < a.n_tiles; i += 256) {
            const float v = a.part_val[(size_t)r * a.n_tiles + i];
            const int ix = a.part_idx[(size_t)r * a.n_tiles + i];
            if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
        }
        sv[tid] = bv; si[tid] = bi;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) {
                const float v = sv[tid + o];
                const int ix = si[tid + o];
                if (v > sv[tid] || (v == sv[tid] && ix < si[tid])) { sv[tid] = v; si[tid] = ix; }
            }
            __syncthreads();
        }
        if (tid == 0) am[r] = si[0];
        __syncthreads();
    }

    const int nc = a.par[LKP_NCORPUS];
    if (tid == 0) {
        const int step0 = t.step_b[0];
        int acc = 0;
        while (acc < d && am[acc] == a.tail[acc + 1]) ++acc;
        int unf = t.eos_id >= 0 ? t.unfinished[0] : 1;
        int hl = t.hist_len[0];
        int n = 0, tok = 0, eos_cut = 0;
        for (int j = 0; j <= acc; ++j) {
            tok = unf ? am[j] : t.pad_id;
            if (t.eos_id >= 0 && tok == t.eos_id) unf = 0;
            if (step0 + j < t.max_new) t.out_tokens[step0 + j] = tok;
            if (hl < t.hist_ld) t.hist[hl++] = tok;          // history index = cache slot: T + max_new <= max_len bounds it
            n = j + 1;
            if (!unf) { eos_cut = j < acc; break; }
        }
        if (t.eos_id >= 0) t.unfinished[0] = unf;
        t.hist_len[0] = hl;
        t.step_b[0] = step0 + n;
        if (t.epoch) *reinterpret_cast<unsigned*>(t.epoch) += 1u;
        int slot = a.slot[0], pos = t.pos_ro[0];
        if (t.slot_b) {                                       // a decode forward: n tokens consumed, as n plain steps would have
            slot += n; pos += n;
            t.slot_b[0] = slot; t.pos[0] = pos;
            const int fwd = a.status[LKS_FWD];
            if (a.trace && fwd < a.trace_cap) { a.trace[2 * fwd] = d; a.trace[2 * fwd + 1] = eos_cut ? n : acc; }
            a.status[LKS_FWD] = fwd + 1;
        } else {
            a.status[LKS_FWD] = 0;
        }
        n_s = n; step0_s = step0; pos_s = pos; slot_s = slot; tok_s = tok; eos_s = !unf; hlen_s = nc + hl;
        fin_s = !unf || step0 + n >= t.max_new;
    }
    __syncthreads();
    const int n = n_s, step0 = step0_s, fin = fin_s;

    // the emitted rows of the pass's logits (a [.][32001] row starts at an odd element: 2-byte pieces)
    if (d > 0 && a.scores && a.logits) {
        const unsigned short* src = (const unsigned short*)a.logits;
        unsigned short* dst = (unsigned short*)a.scores;
        for (int j = 0; j < n; ++j) {
            if (step0 + j >= t.max_new) break;
            const unsigned short* s = src + (size_t)j * t.vocab;
            unsigned short* o = dst + (size_t)(step0 + j) * t.vocab;
            for (int i = tid; i < t.vocab; i += 256) o[i] = s[i];
        }
    }
    if (eos_s) for (int i = step0 + n + tid; i < t.max_new; i += 256) t.out_tokens[i] = t.pad_id;
    {
        int id = tok_s;
        id = id < 0 ? 0 : (id >= t.vocab ? t.vocab - 1 : id);
        const T* src = (const T*)t.embed + (size_t)id * t.H;
        T* x_next = (T*)t.x_next;
        for (int i = tid * 8; i < t.H; i += 256 * 8) stg16(x_next + i, ldg16(src + i));
        if (t.cur_rope && tid < 32) {
            const int half = tid >> 4, c8 = (tid & 15) * 8;
            const T* tab = (const T*)(half ? t.sin_t : t.cos_t);
            stg16((T*)t.cur_rope + half * 128 + c8, ldg16(tab + (size_t)pos_s * 128 + c8));
        }
    }

    // the draft for the next forward, clipped to what may still be emitted (one token of every forward is the model's own) and to the call's cache slots
    const int hlen = hlen_s;
    int dmax = a.par[LKP_DRAFT_LEN];
    dmax = min(dmax, t.max_new - (step0 + n) - 1);
    dmax = min(dmax, a.par[LKP_SLOT_END] - 1 - slot_s);
    dmax = min(dmax, LOOKUP_MAX_DRAFT);
    if (fin) dmax = 0;
    int dn = 0, p = 0;
    if (dmax > 0) {
        const int* __restrict__ hist = t.hist;
        const int ng_hi = min(a.par[LKP_NGRAM_MAX], LOOKUP_MAX_NGRAM), ng_lo = max(a.par[LKP_NGRAM_MIN], 1);
        for (int ng = ng_hi; ng >= ng_lo; --ng) {       // (uniform: every thread sees the same hit)
            if (ng >= hlen) continue;
            __syncthreads();
            if (tid < ng) pat[tid] = lk_h(a.corpus, nc, hist, hlen - ng + tid);
            __syncthreads();
            int hit = -1;
            for (int j = hlen - ng - 1 - tid; j >= 0; j -= 256) {
                bool eq = true;
                for (int i = 0; i < ng; ++i) eq = eq && lk_h(a.corpus, nc, hist, j + i) == pat[i];
                if (eq) { hit = j; break; }
            }
            si[tid] = hit;
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if (tid < o) si[tid] = max(si[tid], si[tid + o]);
                __syncthreads();
            }
            const int j = si[0];
            if (j >= 0) { p = j + ng; dn = min(dmax, hlen - p); break; }
        }
    }
    if (tid == 0) a.tail[0] = tok_s;
    if (tid < dn) a.tail[1 + tid] = lk_h(a.corpus, nc, t.hist, p + tid);
    if (tid <= dn) a.pos_ids[tid] = pos_s + tid;
    if (tid == 0) {
        a.img_pos[0] = 0;
        a.status[LKS_NEXT] = dn | (fin << 8);
        a.status[LKS_SLOT] = slot_s;
    }
}

void launch_lookup_accept(int dtype, const LookupArgs& a, const StepTail& t, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((lookup_accept_k<T>), dim3(1), dim3(256), 0, s, a, t));
}

}  // namespace rdx
