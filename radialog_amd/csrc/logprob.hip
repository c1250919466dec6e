// Generation log-probs: what the step's selection was sure of -- the chosen token's log-prob and the top-n alternatives of the scores row it was chosen from.
#include "../../include/rdx.h"
#include "rdx_common.h"

namespace rdx {

// ---- logprob_step_k: one workgroup per batch row, behind the step's selection launch (greedy_step_k / select_step_k / sample_step_k) --------------------
// The selection's tail has advanced d_step[b], so the step this launch describes is step = d_step[b] - 1; its token is tokens[b * max_new + step] (what the
// tail wrote: the pad token for a row that had finished) and its scores row x lies where the lm_head wrote it and the selection left it (raw, processed or
// warped): logits + step * step_stride + b * row_stride elements, model dtype, columns 0 .. vocab - 1. With m = max x, S = sum exp(float(x_i) - m):
//   chosen[b][step] = (float(x_tok) - m) - log(S)       (fp32, never rounded to the model dtype: score_rows_k's formula),
//   top_ids[b][step][k], k < top_n: the columns with the largest x in descending order, lowest index on ties; top_lp[..][k] their log-probs likewise.
// NaN columns never enter the top-n; a slot without a candidate holds (-1, 0.0f). -inf columns follow the finite ones, with log-prob -inf.
// A step outside [0, max_new) writes nothing. Entries k >= top_n are left as they are.
// The row is read from memory ONCE into LDS. A [B][32001] buffer's rows start at odd elements: scalar head up to the first 16-byte boundary, 16-byte pieces
// (four in flight per thread), scalar tail (select_step_k's walk). Element i lands at LDS element i whatever the row's alignment, and every later pass is
// indexed by i alone: thread t owns the 8-element groups t, t + 256, ... and adds their terms element by element, then a 256-leaf LDS tree joins the partial
// sums (score_rows_k's order). No floating-point atomics, nothing depends on the address: the same row gives the same bits wherever it lies.
// The top-n works on integers. The sum pass leaves, in place of each value, its order-preserving 16-bit key (a < b <=> key(a) < key(b); -0 and +0 share one;
// 0 for NaN and for the LDS elements behind vocab - 1). key << 16 | (0xffff - index) is then unique per column and its order IS (value descending, index
// ascending): round k takes the block maximum of the composite keys below round k - 1's pick -- one compare, one select and one max per element, no branch,
// and an integer maximum does not depend on the order it is taken in.
template <typename T> struct InfBits;
template <> struct InfBits<f16> { static constexpr unsigned v = 0x7c00u; };
template <> struct InfBits<bf16> { static constexpr unsigned v = 0x7f80u; };
template <typename T> __device__ __forceinline__ unsigned lp_key(unsigned u) {          // u: the 16 bits of a T
    if (u == 0x8000u) u = 0u;
    const unsigned k = (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
    return (u & 0x7fffu) > InfBits<T>::v ? 0u : k;
}
__device__ __forceinline__ unsigned lp_unkey(unsigned k) { return (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu); }
// the maximum over the 256 threads, in every thread (sw: 4 words of LDS); exact, so any order will do
template <typename V> __device__ __forceinline__ V lp_block_max(V v, V* sw) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const V w = __shfl_xor(v, o); v = w > v ? w : v; }
    __syncthreads();                     // the previous user of sw is done
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = v;
    __syncthreads();
    const V a = sw[0] > sw[1] ? sw[0] : sw[1], c = sw[2] > sw[3] ? sw[2] : sw[3];
    return a > c ? a : c;
}

template <typename T>
__global__ __launch_bounds__(256) void logprob_step_k(LogprobArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lp_row[];
    __shared__ float sv[256];
    __shared__ float swf[4];
    __shared__ unsigned swu[4];
    const int b = blockIdx.x, tid = threadIdx.x, V = a.vocab;
    if (b >= a.B) return;
    const int step = a.d_step[b] - 1;
    if (step < 0 || step >= a.max_new) return;
    const T* row = (const T*)a.logits + (size_t)step * a.step_stride + (size_t)b * a.row_stride;

    // ---- the row into LDS, its maximum on the way (exact whatever the order; NaN never compares greater) ----
    float bv = -INFINITY;
    auto one = [&](int i) {
        const T v = row[i];
        lp_row[i] = bits16<T>(v);
        const float f = tof<T>(v);
        bv = f > bv ? f : bv;
    };
    const int head = min(V, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 1));
    const int nvec = (V - head) >> 3;
    if (tid < head) one(tid);
    for (int i = head + nvec * 8 + tid; i < V; i += 256) one(i);
    for (int q0 = tid; q0 < nvec; q0 += 4 * 256) {
        u4 raw[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) raw[u] = ldg16(row + head + (size_t)min(q0 + u * 256, nvec - 1) * 8);       // clamped: loaded twice, stored once
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = q0 + u * 256;
            if (q < nvec) {
                const int i = head + q * 8;
                const auto v = as_vec8<T>(raw[u]);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    lp_row[i + j] = bits16<T>(v[j]);
                    const float f = tof<T>(v[j]);
                    bv = f > bv ? f : bv;
                }
            }
        }
    }
    const float m = lp_block_max<float>(bv, swf);        // (its barriers: the row is complete for every thread)
    float xt = 0.f;
    int tok = -1;
    if (tid == 0) {
        tok = a.tokens[(size_t)b * a.max_new + step];
        if (tok >= 0 && tok < V) xt = tof<T>(from_bits16<T>(lp_row[tok]));
    }
    __syncthreads();                     // the token's value is read before the sum pass turns the row into keys

    // ---- S: thread t adds the terms of groups t, t + 256, ... in index order, then the tree; the group goes back as keys ----
    const int ngroups = (V + 7) >> 3;    // the LDS row holds whole groups; the elements behind V - 1 are never read as values
    u4* rowq = reinterpret_cast<u4*>(lp_row);
    const bool want_keys = a.top_n > 0;
    float s = 0.f;
    for (int g = tid; g < ngroups; g += 256) {
        const u4 raw = rowq[g];
        const auto v = as_vec8<T>(raw);
        unsigned kq[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = g * 8 + j < V;
            const float e = expf(tof<T>(v[j]) - m);
            s += in ? e : 0.f;           // (+ 0.0f leaves the non-negative sum as it is)
            const unsigned k = in ? lp_key<T>(bits16<T>(v[j])) : 0u;
            kq[j >> 1] = (j & 1) ? (kq[j >> 1] | (k << 16)) : k;
        }
        if (want_keys) rowq[g] = (u4){kq[0], kq[1], kq[2], kq[3]};
    }
    sv[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sv[tid] += sv[tid + o];
        __syncthreads();
    }
    const float log_s = logf(sv[0]);

    const size_t e = (size_t)b * a.out_ld + step;
    if (tid == 0) a.chosen[e] = (tok >= 0 && tok < V) ? (xt - m) - log_s : 0.0f;

    // ---- top-n: round k takes the largest composite key below the previous pick ----
    unsigned pk = 0xffffffffu;
    for (int k = 0; k < a.top_n; ++k) {
        unsigned best = 0u;
        for (int g = tid; g < ngroups; g += 256) {
            const u4 kv = rowq[g];
            const unsigned ib = 0xffffu - (unsigned)(g * 8);         // V <= 65536: the index fits 16 bits
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const unsigned d = w == 0 ? kv.x : w == 1 ? kv.y : w == 2 ? kv.z : kv.w;
                const unsigned c0 = (d << 16) | (ib - 2 * w), c1 = (d & 0xffff0000u) | (ib - 2 * w - 1);
                const unsigned m0 = c0 < pk ? c0 : 0u, m1 = c1 < pk ? c1 : 0u;
                best = max(best, max(m0, m1));
            }
        }
        pk = lp_block_max<unsigned>(best, swu);
        if (tid == 0) {
            const bool none = (pk >> 16) == 0u;          // fewer than k + 1 columns that are not NaN (nothing below "none" has a key either: the later rounds find none)
            const float pv = tof<T>(from_bits16<T>((unsigned short)lp_unkey(pk >> 16)));
            a.top_ids[e * RDX_MAX_TOP_LOGPROBS + k] = none ? -1 : (int)(0xffffu - (pk & 0xffffu));
            a.top_lp[e * RDX_MAX_TOP_LOGPROBS + k] = none ? 0.0f : (pv - m) - log_s;
        }
    }
}

// of the CU's 160 KB (two 64-KB rows share a CU); the composite keys of the top-n hold the column index in 16 bits
bool logprob_step_supported(int vocab) { return vocab > 0 && vocab <= 65536 && logprob_step_lds(vocab) <= 144 * 1024; }

void launch_logprob_step(int dtype, const LogprobArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    const size_t lds = logprob_step_lds(a.vocab);
    static DevOnce once[2];
    RDX_DISPATCH_T(dtype, T, {
        if (once[dtype == DT_BF16].first()) (void)hipFuncSetAttribute((const void*)logprob_step_k<T>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        hipLaunchKernelGGL((logprob_step_k<T>), dim3(a.B), dim3(256), lds, s, a);
    });
}

}  // namespace rdx
