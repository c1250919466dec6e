// Scoring given tokens: log p(target | row) and the argmax of logits rows, without the host ever seeing a [rows][vocab] tensor.
#include "rdx_common.h"

namespace rdx {

// ---- score_rows_k: one workgroup per logits row ---------------------------------------------------------------------------
// Row `r` of `logits` ([M][ld], model dtype, ld % 8 == 0 and the base 16-byte aligned, so every row is) holds `vocab` real columns and ld - vocab
// pad columns with whatever the GEMM left there: only columns 0 .. vocab - 1 are looked at. With m = max x, S = sum exp(float(x_i) - m):
//   logprob[r] = (float(x_target) - m) - log(S)   (fp32, never rounded to the model dtype),   top1[r] = argmax, lowest index on ties (greedy_step_k's rule).
// A row whose target is -100 (HF's ignore_index) writes (0.0f, -1) and reads nothing: a NaN in it goes nowhere.
// The row is read from memory ONCE, in 16-byte pieces, into LDS (2 ld bytes, as sample_step_k keeps its row); pass 1 (max, argmax) runs on the registers
// that were just loaded, pass 2 (the sum) on each thread's OWN pieces in LDS. Order of every reduction is fixed -- thread t sums its pieces t, t + 256, ...
// element by element, then a 256-leaf LDS tree -- and there are no floating-point atomics: the same input gives the same bits.
template <typename T>
__global__ __launch_bounds__(256) void score_rows_k(const T* __restrict__ logits, long ld, const int* __restrict__ target, int vocab,
                                                    float* __restrict__ logprob, int* __restrict__ top1) {
    extern __shared__ u4 row_s[];
    __shared__ float sv[256];
    __shared__ int si[256];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int tg = target[r];
    if (tg < 0 || tg >= vocab) {         // -100 (anything outside the vocabulary is treated alike: the callers refuse it beforehand)
        if (tid == 0) { logprob[r] = 0.0f; top1[r] = -1; }
        return;
    }
    const T* src = logits + (size_t)r * ld;
    const int nchunks = (vocab + 7) >> 3;            // the last piece may reach into the pad columns (ld % 8 == 0 keeps it inside the row): masked below
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = tid; c < nchunks; c += 256) {
        const u4 raw = ldg16(src + (size_t)c * 8);
        row_s[c] = raw;
        const auto v = as_vec8<T>(raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ix = c * 8 + j;
            const float x = tof<T>(v[j]);
            if (ix < vocab && (x > bv || (x == bv && ix < bi))) { bv = x; bi = ix; }
        }
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
    const float m = sv[0];
    const int am = si[0];
    __syncthreads();                     // sv is reused by the sum
    float s = 0.f;
    for (int c = tid; c < nchunks; c += 256) {
        const auto v = as_vec8<T>(row_s[c]);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (c * 8 + j < vocab) s += expf(tof<T>(v[j]) - m);
    }
    sv[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sv[tid] += sv[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const float xt = tof<T>(reinterpret_cast<const T*>(row_s)[tg]);
        logprob[r] = (xt - m) - logf(sv[0]);
        top1[r] = am == 0x7fffffff ? -1 : am;        // a row of NaN only: no argmax
    }
}

bool score_rows_supported(int vocab, long ld) { return vocab > 0 && ld >= vocab && ld % 8 == 0 && score_rows_lds(vocab) <= 144 * 1024; }

void launch_score_rows(int dtype, const void* logits, long ld, const int* target, int vocab, float* logprob, int* top1, int M, hipStream_t s) {
    if (M <= 0) return;
    const size_t lds = score_rows_lds(vocab);
    static DevOnce once[2];
    RDX_DISPATCH_T(dtype, T, {
        if (once[dtype == DT_BF16].first()) (void)hipFuncSetAttribute((const void*)score_rows_k<T>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
        hipLaunchKernelGGL((score_rows_k<T>), dim3(M), dim3(256), lds, s, (const T*)logits, ld, target, vocab, logprob, top1);
    });
}

// ---- the index-list forms of gather_last_k and its inverse ----------------------------------------------------------------
// out[i] = x[rows[i]] for i < n: the residual rows whose successor position is scored, compacted for the final RMSNorm and the lm_head
template <typename T>
__global__ void gather_rows_k(const T* __restrict__ x, const int* __restrict__ rows, T* __restrict__ out, int H) {
    const T* src = x + (size_t)rows[blockIdx.x] * H;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) stg16(out + (size_t)blockIdx.x * H + i, ldg16(src + i));
}
void launch_gather_rows(int dtype, const void* x, const int* rows, void* out, int n, int H, hipStream_t s) {
    if (n <= 0) return;
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((gather_rows_k<T>), dim3(n), dim3(256), 0, s, (const T*)x, rows, (T*)out, H));
}

// the chunk's results back to [batch][T]: entry dst[i] receives row i (logprob; top1 when asked for)
__global__ void score_scatter_k(const float* __restrict__ lp, const int* __restrict__ t1, const int* __restrict__ dst, float* __restrict__ logprob,
                                int* __restrict__ top1, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int d = dst[i];
    if (d < 0) return;
    logprob[d] = lp[i];
    if (top1) top1[d] = t1[i];
}
void launch_score_scatter(const float* lp, const int* t1, const int* dst, float* logprob, int* top1, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(score_scatter_k, dim3((n + 255) / 256), dim3(256), 0, s, lp, t1, dst, logprob, top1, n);
}

// logits rows [n][ld] -> out[dst[i]][0 .. vocab): the chunk copied out without its pad columns. vocab may be odd, so a destination row is only
// 2-byte aligned: element-wise stores.
template <typename T>
__global__ void logits_out_k(const T* __restrict__ ws, long ld, const int* __restrict__ dst, T* __restrict__ out, int vocab) {
    const int d = dst[blockIdx.x];
    if (d < 0) return;
    const T* src = ws + (size_t)blockIdx.x * ld;
    T* o = out + (size_t)d * vocab;
    for (int i = threadIdx.x; i < vocab; i += blockDim.x) o[i] = src[i];
}
void launch_logits_out(int dtype, const void* ws, long ld, const int* dst, void* out, int vocab, int n, hipStream_t s) {
    if (n <= 0) return;
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((logits_out_k<T>), dim3(n), dim3(256), 0, s, (const T*)ws, ld, dst, (T*)out, vocab));
}

}  // namespace rdx
