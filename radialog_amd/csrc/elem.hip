// Normalisation, layout and bookkeeping kernels (HBM-bound, vectorised where the layout allows).
#include <algorithm>
#include "rdx_common.h"
#include "rdx_kernels.h"
#include "philox.h"

namespace rdx {

// ---- e4m3 activation quantisation of the fp8 path (gemm8.hip, xstat32.hip): q = RNE_e4m3(x * (448 / absmax)), scale = absmax / 448 ----------
// (the arithmetic of pack_weight_fp8_k and of the oracle's fake quantisation: an all-zero range gets scale 1)

// Row-wise e4m3 quantisation of model-dtype activations [rows][K] (row stride ldx) into row-major bytes [rows][K] + scales [rows][G]:
// K group q = 128-deep blocks [NB q / G, NB (q + 1) / G), NB = K / 128 (G <= 4; K % 128 == 0), one absmax / 448 scale per (row, group). One
// workgroup per row.
template <typename T>
__global__ __launch_bounds__(256) void quant_rows_k(const T* __restrict__ x, long ldx, unsigned char* __restrict__ out8, float* __restrict__ xscale,
                                                    int K, int G) {
    typedef typename Vec8<T>::type V8;
    __shared__ float red[32];
    __shared__ float gmax[4];
    const size_t row = blockIdx.x;
    const T* xr = x + row * ldx;
    const int NB = K >> 7;
    int end[4];                                                 // first element past group q
#pragma unroll
    for (int q = 0; q < 4; ++q) end[q] = q < G ? ((NB * (q + 1)) / G) * 128 : K;
    auto group_of = [&](int i) { return (i >= end[0]) + (i >= end[1]) + (i >= end[2]); };
    float mx[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x * 8; i < K; i += blockDim.x * 8) {
        const float m = amax8<T>(as_vec8<T>(ldg16(xr + i)));
        const int gq = group_of(i);
#pragma unroll
        for (int q = 0; q < 4; ++q) mx[q] = (q == gq) ? fmaxf(mx[q], m) : mx[q];
    }
    for (int q = 0; q < G; ++q) {
        const float m = block_max(mx[q], red);
        if (threadIdx.x == 0) gmax[q] = m;
    }
    __syncthreads();
    if ((int)threadIdx.x < G) { float sc, inv; fp8_scale(gmax[threadIdx.x], sc, inv); xscale[row * G + threadIdx.x] = sc; }
    for (int i = threadIdx.x * 8; i < K; i += blockDim.x * 8) {
        float sc, inv;
        fp8_scale(gmax[group_of(i)], sc, inv);
        const u2 q = quant8<T>(as_vec8<T>(ldg16(xr + i)), inv);
        *reinterpret_cast<u2*>(out8 + row * K + i) = q;
    }
}

void launch_quant_rows(int dtype, const void* x, long ldx, void* out8, float* xscale, int rows, int K, int groups, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((quant_rows_k<T>), dim3(rows), dim3(256), 0, s, (const T*)x, ldx, (unsigned char*)out8, xscale, K, groups));
}

// ---- LlamaRMSNorm (modeling_llama_imgemb.py:85-93): fp32 statistics, (x*rstd).to(T), then weight*h in T ---------------
// One workgroup per row of the output layout L (ActLayout, rdx_kernels.h; act_offset): rows >= n_rows are its zero padding. The e4m3 layouts quantise
// the normalised row with ONE absmax / 448 scale (xscale[row]). slab: the pending K-split partials [groups][srows][H] are added into x first (written back).
template <ActLayout L> constexpr bool norm_e4m3 = L == ACT_BLK64_E4M3 || L == ACT_ROWS_E4M3;
template <typename T, ActLayout L> __device__ __forceinline__ void norm_store(T* out, size_t row, int k, int mtl, int H, typename Vec8<T>::type v, float inv) {
    if (norm_e4m3<L>) *reinterpret_cast<u2*>(reinterpret_cast<unsigned char*>(out) + act_offset(L, row, k, mtl, H)) = quant8<T>(v, inv);
    else stg16(out + act_offset(L, row, k, mtl, H), as_u4<T>(v));
}
template <typename T, ActLayout L> __device__ __forceinline__ void norm_store_zero(T* out, size_t row, int k, int mtl, int H) {
    if (norm_e4m3<L>) *reinterpret_cast<u2*>(reinterpret_cast<unsigned char*>(out) + act_offset(L, row, k, mtl, H)) = (u2){0u, 0u};
    else stg16(out + act_offset(L, row, k, mtl, H), (u4){0u, 0u, 0u, 0u});
}

// any H, w nullable (re-layout only: the test hooks), any number of slab groups; one 32-row block of slabs (rmsnorm_supported)
template <typename T, ActLayout L>
__global__ __launch_bounds__(256) void rmsnorm_k(T* x, const T* __restrict__ w, T* __restrict__ out, int H, float eps, int n_rows,
                                                 const float* __restrict__ slab, int groups, float* __restrict__ xscale, int mtl) {
    typedef typename Vec8<T>::type V8;
    __shared__ float red[32];
    const size_t row = blockIdx.x;
    if (L != ACT_ROWS && (int)row >= n_rows) {
        for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) norm_store_zero<T, L>(out, row, i, mtl, H);
        if (norm_e4m3<L> && threadIdx.x == 0) xscale[row] = 1.0f;
        return;
    }
    T* xr = x + row * H;
    float ss = 0.f;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) {
        V8 v = as_vec8<T>(ldg16(xr + i));
        if (slab) {
            // pending K-split projection (xsplit32_k): x[row] += T(sum of the groups' fp32 partials, fixed order) -- the residual
            // epilogue of o_proj / down_proj, done here at the launch boundary; the completed row is written back (same thread
            // re-reads it below)
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int gq = 0; gq < groups; ++gq) {
                const float* sp = slab + ((size_t)gq * 32 + row) * H + i;
                const float4 s0 = *reinterpret_cast<const float4*>(sp), s1 = *reinterpret_cast<const float4*>(sp + 4);
                acc[0] += s0.x; acc[1] += s0.y; acc[2] += s0.z; acc[3] += s0.w;
                acc[4] += s1.x; acc[5] += s1.y; acc[6] += s1.z; acc[7] += s1.w;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = fromf<T>(tof<T>(v[j]) + rnd<T>(acc[j]));
            stg16(xr + i, as_u4<T>(v));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = tof<T>(v[j]); ss += f * f; }
    }
    ss = block_sum(ss, red);
    const float rs = rsqrtf(ss / (float)H + eps);
    auto normed = [&](int i) -> V8 {
        V8 v = as_vec8<T>(ldg16(xr + i));
        if (!w) return v;
        V8 o;
        V8 wv = as_vec8<T>(ldg16(w + i));
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = fromf<T>(tof<T>(wv[j]) * rnd<T>(tof<T>(v[j]) * rs));
        return o;
    };
    float inv = 0.f;
    if (norm_e4m3<L>) {
        float am = 0.f;
        for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) am = fmaxf(am, amax8<T>(normed(i)));
        am = block_max(am, red);
        float sc;
        fp8_scale(am, sc, inv);
        if (threadIdx.x == 0) xscale[row] = sc;
    }
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) norm_store<T, L>(out, row, i, mtl, H, normed(i), inv);
}

// One-round-trip version for H = 4096 (decode at batch 3-128: two of these per layer sit on the step's critical path): a
// thread owns 2 x 8 elements, every load (row, slabs, norm weight) is issued up front, the row stays in registers between the
// statistics and the scaling. Same arithmetic and rounding points as rmsnorm_k. Up to 4 slab groups; srows = the slabs' rows per group.
template <typename T, ActLayout L>
__global__ __launch_bounds__(256) void rmsnorm4096_k(T* x, const T* __restrict__ w, T* __restrict__ out, float eps, int n_rows,
                                                     const float* __restrict__ slab, int groups, int srows, float* __restrict__ xscale, int mtl) {
    typedef typename Vec8<T>::type V8;
    constexpr int H = 4096;
    __shared__ float red[32];
    const size_t row = blockIdx.x;
    const int i0 = threadIdx.x * 8, i1 = i0 + 2048;
    if (L != ACT_ROWS && (int)row >= n_rows) {
        norm_store_zero<T, L>(out, row, i0, mtl, H);
        norm_store_zero<T, L>(out, row, i1, mtl, H);
        if (norm_e4m3<L> && threadIdx.x == 0) xscale[row] = 1.0f;
        return;
    }
    T* xr = x + row * H;
    V8 v[2] = {as_vec8<T>(ldg16(xr + i0)), as_vec8<T>(ldg16(xr + i1))};
    const V8 wv[2] = {as_vec8<T>(ldg16(w + i0)), as_vec8<T>(ldg16(w + i1))};
    if (slab) {
        float4 sp[4][2][2];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float* p = slab + ((size_t)min(gq, groups - 1) * srows + row) * H + (k ? i1 : i0);
                sp[gq][k][0] = *reinterpret_cast<const float4*>(p);
                sp[gq][k][1] = *reinterpret_cast<const float4*>(p + 4);
            }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
                if (gq < groups) {
                    acc[0] += sp[gq][k][0].x; acc[1] += sp[gq][k][0].y; acc[2] += sp[gq][k][0].z; acc[3] += sp[gq][k][0].w;
                    acc[4] += sp[gq][k][1].x; acc[5] += sp[gq][k][1].y; acc[6] += sp[gq][k][1].z; acc[7] += sp[gq][k][1].w;
                }
#pragma unroll
            for (int j = 0; j < 8; ++j) v[k][j] = fromf<T>(tof<T>(v[k][j]) + rnd<T>(acc[j]));
            stg16(xr + (k ? i1 : i0), as_u4<T>(v[k]));
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = tof<T>(v[k][j]); ss += f * f; }
    ss = block_sum(ss, red);
    const float rs = rsqrtf(ss / (float)H + eps);
    V8 o[2];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) o[k][j] = fromf<T>(tof<T>(wv[k][j]) * rnd<T>(tof<T>(v[k][j]) * rs));
    float inv = 0.f;
    if (norm_e4m3<L>) {
        const float am = block_max(fmaxf(amax8<T>(o[0]), amax8<T>(o[1])), red);
        float sc;
        fp8_scale(am, sc, inv);
        if (threadIdx.x == 0) xscale[row] = sc;
    }
    norm_store<T, L>(out, row, i0, mtl, H, o[0], inv);
    norm_store<T, L>(out, row, i1, mtl, H, o[1], inv);
}

// what the two kernels cover between them: rmsnorm_k holds one 32-row block of slabs and of e4m3 bytes
static bool norm_4096(const NormArgs& n) { return n.H == 4096 && n.w && (!n.slab || n.groups <= 4); }
static int norm_blocks(const NormArgs& n) { return n.layout == ACT_BLK64_E4M3 && n.mtiles > 2 ? (n.mtiles + 1) / 2 : 1; }

bool rmsnorm_supported(const NormArgs& n) {
    const bool e4m3 = n.layout == ACT_BLK64_E4M3 || n.layout == ACT_ROWS_E4M3, rowmajor = n.layout == ACT_ROWS || n.layout == ACT_ROWS_E4M3;
    if (!n.x || !n.out || n.rows <= 0 || n.H <= 0 || n.H % (rowmajor ? 8 : (n.layout == ACT_BLK32 || n.layout == ACT_TILES32) ? 32 : 64) || (e4m3 && !n.xscale) || (n.slab && n.groups < 1)) return false;
    if (n.layout < ACT_ROWS || n.layout > ACT_ROWS_E4M3 || (n.layout == ACT_TILES32 && n.mtiles < 1)) return false;
    const int held = n.layout == ACT_TILES32 ? 16 * n.mtiles : 32 * norm_blocks(n);      // rows the packed orders hold; row-major slabs hold 32
    if ((!rowmajor || n.slab) && n.rows > held) return false;
    return norm_4096(n) || !((n.layout == ACT_TILES32 && n.slab) || norm_blocks(n) > 1);
}

bool launch_rmsnorm(int dtype, const NormArgs& n, hipStream_t s) {
    if (!rmsnorm_supported(n)) return false;
    const int mtl = n.layout == ACT_TILES32 ? n.mtiles : 2 * norm_blocks(n);
    const int held = n.layout == ACT_TILES32 ? 16 * mtl : 32 * norm_blocks(n);
    const dim3 grid(n.layout == ACT_ROWS || n.layout == ACT_ROWS_E4M3 ? n.rows : held);
    const bool k4096 = norm_4096(n);
    const float* slab = n.slab;
    const int groups = slab ? n.groups : 0;
#define RDX_NORM(LAY)                                                                                                                                    \
    case LAY:                                                                                                                                            \
        if (k4096) hipLaunchKernelGGL((rmsnorm4096_k<T, LAY>), grid, dim3(256), 0, s, (T*)n.x, (const T*)n.w, (T*)n.out, n.eps, n.rows, slab, groups, held, n.xscale, mtl); \
        else hipLaunchKernelGGL((rmsnorm_k<T, LAY>), grid, dim3(256), 0, s, (T*)n.x, (const T*)n.w, (T*)n.out, n.H, n.eps, n.rows, slab, groups, n.xscale, mtl);            \
        break;
    RDX_DISPATCH_T(dtype, T, switch (n.layout) { RDX_NORM(ACT_ROWS) RDX_NORM(ACT_BLK32) RDX_NORM(ACT_BLK64) RDX_NORM(ACT_TILES32) RDX_NORM(ACT_BLK64_E4M3) RDX_NORM(ACT_ROWS_E4M3) });
#undef RDX_NORM
    return true;
}

// ---- LayerNorm over the last dim (Q-Former post-LN, eps 1e-12; fp32 statistics, two-pass variance) -------------------
template <typename T>
__global__ __launch_bounds__(256) void layernorm_k(const T* __restrict__ x, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, T* __restrict__ out,
                                                   float* __restrict__ out_f32, int H, float eps) {
    __shared__ float red[32];
    const size_t row = blockIdx.x;
    const T* xr = x + row * H;
    float s = 0.f;
    for (int i = threadIdx.x; i < H; i += blockDim.x) s += tof<T>(xr[i]);
    const float mean = block_sum(s, red) / (float)H;
    float v = 0.f;
    for (int i = threadIdx.x; i < H; i += blockDim.x) { const float d = tof<T>(xr[i]) - mean; v += d * d; }
    const float rstd = rsqrtf(block_sum(v, red) / (float)H + eps);
    for (int i = threadIdx.x; i < H; i += blockDim.x) {
        const float y = (tof<T>(xr[i]) - mean) * rstd * gamma[i] + beta[i];
        if (out) out[row * H + i] = fromf<T>(y);
        if (out_f32) out_f32[row * H + i] = y;
    }
}

void launch_layernorm(int dtype, const void* x, const float* gamma, const float* beta, void* out, float* out_f32, int rows,
                      int H, float eps, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((layernorm_k<T>), dim3(rows), dim3(256), 0, s, (const T*)x, gamma, beta,
                                                (T*)out, out_f32, H, eps));
}

// ---- LayerNorm with row strides and an optional additive per-token embedding (ViT pooler: norm1(x) + pos/type emb) ---
template <typename T>
__global__ __launch_bounds__(256) void layernorm_ex_k(const T* __restrict__ x, long ldx, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, const T* __restrict__ emb, int emb_rows,
                                                      T* __restrict__ out, long ldo, int H, float eps) {
    __shared__ float red[32];
    const size_t row = blockIdx.x;
    const T* xr = x + row * ldx;
    float s = 0.f;
    for (int i = threadIdx.x; i < H; i += blockDim.x) s += tof<T>(xr[i]);
    const float mean = block_sum(s, red) / (float)H;
    float v = 0.f;
    for (int i = threadIdx.x; i < H; i += blockDim.x) { const float d = tof<T>(xr[i]) - mean; v += d * d; }
    const float rstd = rsqrtf(block_sum(v, red) / (float)H + eps);
    const T* er = emb ? emb + (size_t)(row % emb_rows) * H : nullptr;
    for (int i = threadIdx.x; i < H; i += blockDim.x) {
        float y = (tof<T>(xr[i]) - mean) * rstd * gamma[i] + beta[i];
        if (er) y += tof<T>(er[i]);
        out[row * ldo + i] = fromf<T>(y);
    }
}
void launch_layernorm_ex(int dtype, const void* x, long ldx, const float* gamma, const float* beta, const void* emb, int emb_rows,
                         void* out, long ldo, int rows, int H, float eps, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((layernorm_ex_k<T>), dim3(rows), dim3(256), 0, s, (const T*)x, ldx, gamma, beta,
                                                (const T*)emb, emb_rows, (T*)out, ldo, H, eps));
}

// ---- ViT pooler token plumbing: tokens[b][j] = (j < L ? current : previous) image's patch j % L; final concat ----------
template <typename T>
__global__ void pool_gather_k(const T* __restrict__ src, T* __restrict__ dst, int B, int L, int C) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;        // one thread = 8 channels
    const int C8 = C >> 3;
    if (i >= (size_t)B * 2 * L * C8) return;
    const int c8 = (int)(i % C8);
    const size_t tok = i / C8;
    const int j = (int)(tok % (2 * L)), b = (int)(tok / (2 * L));
    const size_t srow = (size_t)(j < L ? b : B + b) * L + (j % L);
    stg16(dst + tok * C + c8 * 8, ldg16(src + srow * C + c8 * 8));
}
void launch_pool_gather(int dtype, const void* src, void* dst, int B, int L, int C, hipStream_t s) {
    const size_t n = (size_t)B * 2 * L * (C >> 3);
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((pool_gather_k<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const T*)src,
                                                (T*)dst, B, L, C));
}
template <typename T>
__global__ void pool_concat_k(const T* __restrict__ patch, const T* __restrict__ tokens, T* __restrict__ dst, int B, int L, int C) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;        // dst [B*L][2C]: [patch_x | diff_x]
    const int C8 = C >> 3;
    if (i >= (size_t)B * L * 2 * C8) return;
    const int c8 = (int)(i % (2 * C8));
    const size_t row = i / (2 * C8);
    const int b = (int)(row / L), j = (int)(row % L);
    const T* srcp = c8 < C8 ? patch + row * C + c8 * 8 : tokens + ((size_t)b * 2 * L + j) * C + (c8 - C8) * 8;
    stg16(dst + row * 2 * C + c8 * 8, ldg16(srcp));
}
void launch_pool_concat(int dtype, const void* patch, const void* tokens, void* dst, int B, int L, int C, hipStream_t s) {
    const size_t n = (size_t)B * L * 2 * (C >> 3);
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((pool_concat_k<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const T*)patch,
                                                (const T*)tokens, (T*)dst, B, L, C));
}

// ---- the NCHW reshape scramble + ln_vision (blip2_qformer.py:469, blip2.py:199-205) ----------------------------------
// The projector output is produced NHWC ([B][P][C]); the reference reshapes its NCHW tensor [B][C][P] to [B][P][C] without a
// permute, so token row r, column c is flat element f = r*C + c of the [C][P] matrix: channel f / P, position f % P.
template <typename T>
__global__ __launch_bounds__(256) void scramble_layernorm_k(const T* __restrict__ pp, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, T* __restrict__ out,
                                                            float* __restrict__ out_f32, int P, int C, float eps) {
    __shared__ float red[32];
    extern __shared__ float rowbuf[];
    const int rrow = blockIdx.x, b = blockIdx.y;
    const T* src = pp + (size_t)b * P * C;
    float s = 0.f;
    if ((C & 7) == 0) {
        // the row's C elements are the flat range [rrow C, rrow C + C) of the [C][P] matrix: <= C / P + 2 channels x all P positions. Gathered as 16-byte
        // pieces (8 channels of one position) instead of one 2-byte element per 64-byte sector (round 3 PMC: 227 MB fetched for an 18 MB input at batch 32);
        // the sums below run over rowbuf in the order they always did, so the result is bit-identical.
        typedef typename Vec8<T>::type V8;
        const int f0 = rrow * C, ch_lo = (f0 / P) & ~7, ch_hi = (f0 + C - 1) / P;
        const int nch8 = ((ch_hi - ch_lo) >> 3) + 1;
        for (int it = threadIdx.x; it < P * nch8; it += blockDim.x) {
            const int pos = it / nch8, ch8 = ch_lo + (it - pos * nch8) * 8;
            if (ch8 >= C) continue;
            const V8 v = as_vec8<T>(ldg16(src + (size_t)pos * C + ch8));
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = (ch8 + j) * P + pos - f0;
                if (c >= 0 && c < C) rowbuf[c] = tof<T>(v[j]);
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += blockDim.x) s += rowbuf[c];
    } else {
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            const size_t f = (size_t)rrow * C + c;
            const int ch = (int)(f / P), pos = (int)(f % P);
            const float v = tof<T>(src[(size_t)pos * C + ch]);
            rowbuf[c] = v;
            s += v;
        }
    }
    const float mean = block_sum(s, red) / (float)C;
    float v2 = 0.f;
    for (int c = threadIdx.x; c < C; c += blockDim.x) { const float d = rowbuf[c] - mean; v2 += d * d; }
    const float rstd = rsqrtf(block_sum(v2, red) / (float)C + eps);
    const size_t o = ((size_t)b * P + rrow) * C;
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float y = (rowbuf[c] - mean) * rstd * gamma[c] + beta[c];
        if (out) out[o + c] = fromf<T>(y);
        if (out_f32) out_f32[o + c] = y;
    }
}

void launch_scramble_layernorm(int dtype, const void* pp_nhwc, const float* gamma, const float* beta, void* out,
                               float* out_f32, int B, int P, int C, float eps, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((scramble_layernorm_k<T>), dim3(P, B), dim3(256), (size_t)C * sizeof(float), s,
                                                (const T*)pp_nhwc, gamma, beta, (T*)out, out_f32, P, C, eps));
}

// ---- image prep: float32 NCHW [B,3,S,S] -> T NHWC, zero-padded spatially, 4 channels (4th = 0) -------------------------
template <typename T>
__global__ __launch_bounds__(256) void img_prep_k(const float* __restrict__ img, T* __restrict__ out, int S, int pad, int Hp,
                                                  int Wp) {
    const int b = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= Wp) return;
    typedef T T4 __attribute__((ext_vector_type(4)));
    T4 o;
    o[0] = o[1] = o[2] = o[3] = fromf<T>(0.f);
    const int iy = y - pad, ix = x - pad;
    if (iy >= 0 && iy < S && ix >= 0 && ix < S) {
        const size_t plane = (size_t)S * S;
        const float* p = img + (size_t)b * 3 * plane + (size_t)iy * S + ix;
        o[0] = fromf<T>(p[0]); o[1] = fromf<T>(p[plane]); o[2] = fromf<T>(p[2 * plane]);
    }
    *reinterpret_cast<T4*>(out + (((size_t)b * Hp + y) * Wp + x) * 4) = o;
}

void launch_img_prep(int dtype, const float* img, void* out, int B, int S, int pad, int Hp, int Wp, hipStream_t s) {
    dim3 grid((Wp + 255) / 256, Hp, B), block(256);
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((img_prep_k<T>), grid, block, 0, s, img, (T*)out, S, pad, Hp, Wp));
}

// ---- 3x3 stride-2 pad-1 max pool, NHWC, 8 channels per thread -------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void maxpool_k(const T* __restrict__ in, T* __restrict__ out, int H, int W, int C, int Ho,
                                                 int Wo, size_t total) {
    typedef typename Vec8<T>::type V8;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int C8 = C >> 3;
    const int c8 = (int)(idx % C8);
    size_t rest = idx / C8;
    const int ow = (int)(rest % Wo); rest /= Wo;
    const int oh = (int)(rest % Ho);
    const int b = (int)(rest / Ho);
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = oh * 2 - 1 + kh;
        if (ih < 0 || ih >= H) continue;
        for (int kw = 0; kw < 3; ++kw) {
            const int iw = ow * 2 - 1 + kw;
            if (iw < 0 || iw >= W) continue;
            V8 v = as_vec8<T>(ldg16(in + (((size_t)b * H + ih) * W + iw) * C + c8 * 8));
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = fmaxf(m[j], tof<T>(v[j]));
        }
    }
    V8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = fromf<T>(m[j]);
    stg16(out + (((size_t)b * Ho + oh) * Wo + ow) * C + c8 * 8, as_u4<T>(o));
}

void launch_maxpool(int dtype, const void* in, void* out, int B, int H, int W, int C, hipStream_t s) {
    const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
    const size_t total = (size_t)B * Ho * Wo * (C >> 3);
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((maxpool_k<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                                                (const T*)in, (T*)out, H, W, C, Ho, Wo, total));
}

// ---- small copies / conversions --------------------------------------------------------------------------------------------
template <typename T>
__global__ void broadcast_rows_k(const T* __restrict__ src, T* __restrict__ dst, size_t per, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) dst[i] = src[i % per];
}
void launch_broadcast_rows(int dtype, const void* src, void* dst, int rows, int H, int B, hipStream_t s) {
    const size_t per = (size_t)rows * H, total = per * B;
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((broadcast_rows_k<T>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                                                (const T*)src, (T*)dst, per, total));
}

template <typename T> __global__ void to_f32_k(const T* __restrict__ src, float* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = tof<T>(src[i]);
}
template <typename T> __global__ void from_f32_k(const float* __restrict__ src, T* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = fromf<T>(src[i]);
}
void launch_to_f32(int dtype, const void* src, float* dst, size_t n, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((to_f32_k<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const T*)src, dst, n));
}
void launch_from_f32(int dtype, const float* src, void* dst, size_t n, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((from_f32_k<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, (T*)dst, n));
}

// ---- prompt preparation: split_at_img position, attention mask, position ids (:498-520, :805-810) ---------------------
__global__ void prep_prompt_k(const int* __restrict__ ids, const int* __restrict__ mask_in, int T_, int img_id, int pad_id,
                              int* __restrict__ img_pos, int* __restrict__ pos_ids, uint8_t* __restrict__ key_mask, long km_bs,
                              int max_len_fill, int* __restrict__ pos_next, int* __restrict__ slot_b, int* __restrict__ step_b,
                              int* __restrict__ unfinished) {
    const int b = blockIdx.x;
    const int* row = ids + (size_t)b * T_;
    uint8_t* km = key_mask + (size_t)b * km_bs;
    if (threadIdx.x == 0) {
        int first = -1, cum = 0;
        for (int t = 0; t < T_; ++t) {
            if (first < 0 && row[t] == img_id) first = t;
            const int m = mask_in ? (mask_in[(size_t)b * T_ + t] != 0) : (row[t] != pad_id);
            cum += m;
            pos_ids[(size_t)b * T_ + t] = m ? (cum - 1) : 1;
            km[t] = (uint8_t)m;
        }
        img_pos[b] = first < 0 ? 0 : first;
        pos_next[b] = cum;        // position id of the first generated token = cumsum(mask) - 1 after appending a 1
        slot_b[b] = T_;
        step_b[b] = 0;
        unfinished[b] = 1;
    }
    for (int t = T_ + threadIdx.x; t < max_len_fill; t += blockDim.x) km[t] = 1;   // generated tokens are always attended
}
void launch_prep_prompt(const int* ids, const int* mask_in, int B, int T_, int img_id, int pad_id, int* img_pos, int* pos_ids,
                        uint8_t* key_mask, long km_bs, int* pos_next, int* slot_b, int* step_b, int* unfinished, hipStream_t s) {
    hipLaunchKernelGGL(prep_prompt_k, dim3(B), dim3(256), 0, s, ids, mask_in, T_, img_id, pad_id, img_pos, pos_ids, key_mask,
                       km_bs, (int)km_bs, pos_next, slot_b, step_b, unfinished);
}

// ---- continuation of a cached conversation: `T_` new prompt tokens go behind the first `keep_len` cache slots of every row
// (multi-turn re-prompting, test.py:440-674 / demo.py:277-305, without recomputing the shared prefix). A row's pad count is
// slot - next position, constant since its first prefill; the key mask of the kept slots stays, later slots are already 1.
__global__ void prep_append_k(int T_, int keep_len, int* __restrict__ img_pos, int* __restrict__ pos_ids, int* __restrict__ pos_next,
                              int* __restrict__ slot_b, int* __restrict__ step_b, int* __restrict__ unfinished) {
    const int b = blockIdx.x;
    const int pads = slot_b[b] - pos_next[b];
    const int base = keep_len - pads;
    for (int t = threadIdx.x; t < T_; t += blockDim.x) pos_ids[(size_t)b * T_ + t] = base + t;
    __syncthreads();
    if (threadIdx.x == 0) {
        img_pos[b] = 0;
        pos_next[b] = base + T_;
        slot_b[b] = keep_len + T_;
        step_b[b] = 0;
        unfinished[b] = 1;
    }
}
void launch_prep_append(int B, int T_, int keep_len, int* img_pos, int* pos_ids, int* pos_next, int* slot_b, int* step_b,
                        int* unfinished, hipStream_t s) {
    hipLaunchKernelGGL(prep_append_k, dim3(B), dim3(256), 0, s, T_, keep_len, img_pos, pos_ids, pos_next, slot_b, step_b, unfinished);
}

// ---- embedding gather + image splice (:571-594): rows [p, p+32) take the projected image embedding ----------------------
template <typename T>
__global__ __launch_bounds__(256) void embed_splice_k(const int* __restrict__ ids, const int* __restrict__ img_pos,
                                                      const T* __restrict__ embed, int vocab, const T* __restrict__ img_emb,
                                                      int n_img, T* __restrict__ out, int T_, int H, int use_img) {
    const int t = blockIdx.x, b = blockIdx.y;
    const T* src;
    const int p = img_pos[b];
    if (use_img && t >= p && t < p + n_img) {
        src = img_emb + ((size_t)b * n_img + (t - p)) * H;
    } else {
        int id = ids[(size_t)b * T_ + t];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        src = embed + (size_t)id * H;
    }
    T* dst = out + ((size_t)b * T_ + t) * H;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) stg16(dst + i, ldg16(src + i));
}
void launch_embed_splice(int dtype, const int* ids, const int* img_pos, const void* embed, int vocab, const void* img_emb,
                         int n_img, void* out, int B, int T_, int H, int use_img, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((embed_splice_k<T>), dim3(T_, B), dim3(256), 0, s, ids, img_pos, (const T*)embed,
                                                vocab, (const T*)img_emb, n_img, (T*)out, T_, H, use_img));
}

template <typename T>
__global__ void gather_last_k(const T* __restrict__ x, T* __restrict__ out, int T_, int H) {
    const int b = blockIdx.x;
    const T* src = x + ((size_t)b * T_ + (T_ - 1)) * H;
    for (int i = threadIdx.x * 8; i < H; i += blockDim.x * 8) stg16(out + (size_t)b * H + i, ldg16(src + i));
}
void launch_gather_last(int dtype, const void* x, void* out, int B, int T_, int H, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((gather_last_k<T>), dim3(B), dim3(256), 0, s, (const T*)x, (T*)out, T_, H));
}

// ---- greedy step (transformers 4.28.1 greedy_search rule) ----------------------------------------------------------------
// next = argmax(logits) (lowest index wins ties); finished rows emit pad; a row finishes when it emits eos.
// Also advances the per-row decode state and gathers the next input embedding, so the whole step stays on the device.

// hand-off counters of the NEXT decode step's fused launches: zeroed by the last kernel of this step
__device__ __forceinline__ void zero_handoff_counters(int* __restrict__ ctr_zero, int n_zero) {
    if (ctr_zero && blockIdx.x == 0) for (int i = threadIdx.x; i < n_zero; i += blockDim.x) ctr_zero[i] = 0;
}

// (value, index) argmax over the 256 threads of a workgroup, ties -> lowest index (torch.argmax): a fixed LDS tree, no float atomics, so the
// same inputs give the same token. The result is valid in thread 0.
__device__ __forceinline__ int block_argmax256(float bv, int bi) {
    __shared__ float sv[256];
    __shared__ int si[256];
    sv[threadIdx.x] = bv; si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const float v = sv[threadIdx.x + o];
            const int ix = si[threadIdx.x + o];
            if (v > sv[threadIdx.x] || (v == sv[threadIdx.x] && ix < si[threadIdx.x])) { sv[threadIdx.x] = v; si[threadIdx.x] = ix; }
        }
        __syncthreads();
    }
    return si[0];
}

// What follows the selection of row b's token, shared by greedy_step_k and select_step_k: the EOS / pad rule, the per-row decode state, the token
// history (select_step_k only: hist != null), the next input embedding and the cos | sin row of the next position. `tok` is read in thread 0.
template <typename T>
__device__ __forceinline__ void step_tail(const StepTail& t, int b, int tok) {
    __shared__ int tok_s, pos_s;
    if (threadIdx.x == 0) {
        const int step = t.step_b[b];
        if (t.eos_id >= 0) {
            const int unf = t.unfinished[b];
            tok = unf ? tok : t.pad_id;
            if (tok == t.eos_id) t.unfinished[b] = 0;
        }
        if (step < t.max_new) t.out_tokens[(size_t)b * t.max_new + step] = tok;
        t.step_b[b] = step + 1;
        if (b == 0 && t.epoch) *reinterpret_cast<unsigned*>(t.epoch) += 1u;      // a step has run: the next fused launches' tags differ from every one so far (handoff.h)
        if (t.slot_b) t.slot_b[b] += 1;      // null on the prefill call: token 0 is consumed by the first decode step
        int pcur = t.pos_ro ? t.pos_ro[b] : 0;
        if (t.pos) { pcur = t.pos[b] + 1; t.pos[b] = pcur; }
        if (t.hist) {                        // select_step_k: history index = cache slot index: T + max_new <= max_len bounds it; the check keeps a timing replay inside the row
            const int L = t.hist_len[b];
            if (L < t.hist_ld) { t.hist[(size_t)b * t.hist_ld + L] = tok; t.hist_len[b] = L + 1; }
        }
        pos_s = pcur;
        tok_s = tok;
    }
    __syncthreads();
    int id = tok_s;
    id = id < 0 ? 0 : (id >= t.vocab ? t.vocab - 1 : id);
    const T* src = (const T*)t.embed + (size_t)id * t.H;
    T* x_next = (T*)t.x_next;
    for (int i = threadIdx.x * 8; i < t.H; i += blockDim.x * 8) stg16(x_next + (size_t)b * t.H + i, ldg16(src + i));
    // cos | sin row of the position the NEXT decode step works at, so that decode attention needs no pos -> table load chain
    if (t.cur_rope && threadIdx.x < 32) {
        const int half = threadIdx.x >> 4, c8 = (threadIdx.x & 15) * 8;
        const T* tab = (const T*)(half ? t.sin_t : t.cos_t);
        stg16((T*)t.cur_rope + (size_t)b * 256 + half * 128 + c8, ldg16(tab + (size_t)pos_s * 128 + c8));
    }
}

template <typename T>
__global__ __launch_bounds__(256) void greedy_step_k(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                     int n_tiles, StepTail t) {
    const int b = blockIdx.x;
    zero_handoff_counters(t.ctr_zero, t.n_zero);
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n_tiles; i += blockDim.x) {
        const float v = part_val[(size_t)b * n_tiles + i];
        const int ix = part_idx[(size_t)b * n_tiles + i];
        if (v > bv || (v == bv && ix < bi)) { bv = v; bi = ix; }
    }
    step_tail<T>(t, b, block_argmax256(bv, bi));
}

// ---- greedy step under logits rules (transformers 4.28.1 _get_logits_processor: repetition penalty -> n-gram ban -> min-new-tokens) ----------
// One workgroup per batch row, behind the lm_head launch that wrote the row (plain loads). The row's history -- the prompt as passed, then every token
// selected so far -- marks two LDS bitmaps over the vocabulary: `seen` (penalised once however often a token occurs) and `ban` (-inf). One pass
// over the row applies both, writes the changed elements back in place (the processed row is what the caller's scores hold) and takes the
// argmax of the processed values; no element is read after another thread wrote it. Then the tail of greedy_step_k.
// The row starts at an odd element when vocab is odd (32001): scalar head up to the first 16-byte boundary, 16-byte pieces, scalar tail.
__device__ __forceinline__ unsigned bits8(const unsigned* m, int i) {       // bits i .. i + 7 of a bitmap (i + 7 inside it)
    const int w = i >> 5, sh = i & 31;
    const unsigned long long lo = m[w], hi = sh > 24 ? m[w + 1] : 0u;
    return (unsigned)(((hi << 32) | lo) >> sh) & 0xffu;
}
template <typename T>
__device__ __forceinline__ T apply_rules(T v, bool seen, bool ban, float p) {
    if (seen) {                          // torch.where(x < 0, x * p, x / p) on a model-dtype tensor: fp32 arithmetic, IEEE division, one RNE rounding
        const float f = tof<T>(v);
        v = fromf<T>(f < 0.f ? f * p : __fdiv_rn(f, p));
    }
    return ban ? fromf<T>(-INFINITY) : v;
}
// The rules phase both selection kernels share: row b's history marks `seen` and `ban` ([W] words each, W = ceil(V / 32)). hist null: no history.
__device__ __forceinline__ void mark_rules_bitmaps(const SelectArgs& a, const StepTail& t, int b, int gen, unsigned* seen, unsigned* ban, int W) {
    const int V = t.vocab;
    for (int i = threadIdx.x; i < W; i += blockDim.x) { seen[i] = 0u; ban[i] = 0u; }
    __syncthreads();
    const int L = t.hist ? min(t.hist_len[b], t.hist_ld) : 0, n = a.ngram;
    const int* h = t.hist + (size_t)b * t.hist_ld;
    if (a.penalty != 1.0f)
        for (int j = threadIdx.x; j < L; j += blockDim.x) {
            const int id = h[j];
            if (id >= 0 && id < V) atomicOr(&seen[id >> 5], 1u << (id & 31));
        }
    if (n > 0 && L + 1 >= n)             // every earlier occurrence of the last n - 1 tokens bans the token that followed it
        for (int j = threadIdx.x; j + n - 1 < L; j += blockDim.x) {
            bool same = true;
            for (int k = 0; k < n - 1 && same; ++k) same = h[j + k] == h[L - n + 1 + k];
            const int id = h[j + n - 1];
            if (same && id >= 0 && id < V) atomicOr(&ban[id >> 5], 1u << (id & 31));
        }
    if (threadIdx.x == 0 && a.min_new > 0 && t.eos_id >= 0 && t.eos_id < V && gen < a.min_new) atomicOr(&ban[t.eos_id >> 5], 1u << (t.eos_id & 31));
    __syncthreads();
}
template <typename T>
__global__ __launch_bounds__(256) void select_step_k(SelectArgs a, StepTail t) {
    extern __shared__ unsigned sel_bits[];           // seen[W] | ban[W]
    const int b = blockIdx.x, V = t.vocab, W = (V + 31) >> 5;
    unsigned* seen = sel_bits;
    unsigned* ban = sel_bits + W;
    zero_handoff_counters(t.ctr_zero, t.n_zero);
    const int gen = a.n_gen[b];
    mark_rules_bitmaps(a, t, b, gen, seen, ban, W);

    T* row = (T*)a.logits + (size_t)gen * a.step_stride + (size_t)b * V;
    const float p = a.penalty;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    auto one = [&](int i) {
        const T v0 = row[i];
        const bool s = (seen[i >> 5] >> (i & 31)) & 1u, x = (ban[i >> 5] >> (i & 31)) & 1u;
        const T v1 = apply_rules<T>(v0, s, x, p);
        if (s || x) row[i] = v1;
        const float f = tof<T>(v1);
        if (f > bv || (f == bv && i < bi)) { bv = f; bi = i; }
    };
    const int head = min(V, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 1));
    const int nvec = (V - head) >> 3;
    if ((int)threadIdx.x < head) one(threadIdx.x);
    for (int i = head + nvec * 8 + threadIdx.x; i < V; i += blockDim.x) one(i);
    for (int q = threadIdx.x; q < nvec; q += blockDim.x) {
        const int i = head + q * 8;
        typename Vec8<T>::type v = as_vec8<T>(ldg16(row + i));
        const unsigned s = bits8(seen, i), x = bits8(ban, i);
        if (s | x) {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = apply_rules<T>(v[j], (s >> j) & 1u, (x >> j) & 1u, p);
            stg16(row + i, as_u4<T>(v));
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float f = tof<T>(v[j]);
            if (f > bv || (f == bv && i + j < bi)) { bv = f; bi = i + j; }
        }
    }
    const int tok = block_argmax256(bv, bi);
    if (a.sel_out) {                     // the kernel-test hook: the selection alone, no decode state behind it
        if (threadIdx.x == 0) a.sel_out[b] = tok;
        return;
    }
    step_tail<T>(t, b, tok);
}
// ---- sampled step (transformers 4.28.1 sample: processors -> temperature -> top-k -> top-p -> multinomial; include/rdx.h, rdx_sampling) ----------
// One workgroup per batch row, behind the lm_head launch, in select_step_k's place. The row is read ONCE from memory: rules and temperature are applied on
// the way into LDS (a 32001-element row is 64 KB), every later pass runs from there, and one pass at the end stores the processed row (kept: s_i,
// dropped: -inf). top-k and top-p are radix selections over the order-preserving 16-bit key of the model-dtype value, two 256-bin passes each (high byte,
// low byte): top-k counts elements, top-p sums integer masses q_i = rint(exp(s_i - max) * 2^32). Integer LDS atomics only, so no result depends on the
// order the threads arrive in. The draw: every thread sums the masses of one contiguous index chunk, a block scan of the 256 sums, and the one thread
// whose chunk holds target = (u24 * C_last) >> 24 walks it. u24 comes from Philox at counter (row, tokens generated), key = the seed word in memory.
typedef unsigned long long u64s;
typedef unsigned short v8us __attribute__((ext_vector_type(8)));
// a < b as values <=> okey(a) < okey(b); -0 and +0 share one key; -inf has the lowest key of all non-NaN values
__device__ __forceinline__ unsigned okey(unsigned u) {
    if (u == 0x8000u) u = 0u;
    return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}
template <typename T> __device__ __forceinline__ u64s mass_q(unsigned short u, float smax) {
    return __float2ull_rn(__expf(tof<T>(from_bits16<T>(u)) - smax) * 4294967296.f);     // exp(0) = 1 -> 2^32; NaN (an all -inf row) -> 0
}
// inclusive prefix sum over the 256 threads in thread order; buf = [2][256]; *total = the sum of all. Integer: the same for every schedule.
__device__ __forceinline__ u64s block_scan256(u64s v, u64s* buf, u64s* total) {
    __syncthreads();                     // the previous user of buf is done
    buf[threadIdx.x] = v;
    __syncthreads();
    int src = 0;
#pragma unroll
    for (int o = 1; o < 256; o <<= 1) {
        u64s x = buf[src * 256 + threadIdx.x];
        if ((int)threadIdx.x >= o) x += buf[src * 256 + threadIdx.x - o];
        buf[(src ^ 1) * 256 + threadIdx.x] = x;
        src ^= 1;
        __syncthreads();
    }
    *total = buf[src * 256 + 255];
    return buf[src * 256 + threadIdx.x];
}

template <typename T>
__global__ __launch_bounds__(256) void sample_step_k(SelectArgs a, SampleArgs sp, StepTail t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smp_lds[];
    const int b = blockIdx.x, V = t.vocab, W = (V + 31) >> 5, tid = threadIdx.x;
    // layout = sample_step_lds(): bitmaps | masses[256] | scan[2][256] | counts[256] | words[16] | row
    unsigned* seen = (unsigned*)smp_lds;
    unsigned* ban = seen + W;
    u64s* hmass = (u64s*)(smp_lds + (((size_t)2 * W * 4 + 15) & ~(size_t)15));
    u64s* scan = hmass + 256;
    int* hcnt = (int*)(scan + 512);
    int* words = hcnt + 256;             // 0: max key, 1: selected high byte, 2: rank / unused, 3: low byte, 4: token, 5..6: base mass
    unsigned short* srow = (unsigned short*)(words + 16);
    zero_handoff_counters(t.ctr_zero, t.n_zero);
    const int gen = a.n_gen[b];
    const bool ruled = a.penalty != 1.0f || a.ngram != 0 || a.min_new != 0;
    if (tid < 16) words[tid] = tid == 4 ? 0x7fffffff : (tid == 1 || tid == 3 ? -1 : 0);
    if (ruled) mark_rules_bitmaps(a, t, b, gen, seen, ban, W);

    // ---- the row into LDS: rules, then temperature. Element i lives at srow[pad + i], so that the 16-byte pieces of the row in memory are 16-byte pieces here
    T* row = (T*)a.logits + (size_t)gen * a.step_stride + (size_t)b * V;
    const int head = min(V, (int)(((16u - (unsigned)((uintptr_t)row & 15u)) & 15u) >> 1));
    const int nvec = (V - head) >> 3, pad = (8 - head) & 7;
    unsigned short* sr = srow + pad;
    const float p = a.penalty, temp = sp.temperature;
    int kmax = 0;
    auto cook = [&](T v, bool s, bool x) -> unsigned short {
        if (ruled) v = apply_rules<T>(v, s, x, p);
        if (temp != 1.0f) v = fromf<T>(__fdiv_rn(tof<T>(v), temp));        // scores / temperature on a model-dtype tensor: fp32 IEEE division, one rounding
        const unsigned short u = bits16<T>(v);
        kmax = max(kmax, (int)okey(u));
        return u;
    };
    auto one = [&](int i) {
        const bool s = ruled && ((seen[i >> 5] >> (i & 31)) & 1u), x = ruled && ((ban[i >> 5] >> (i & 31)) & 1u);
        sr[i] = cook(row[i], s, x);
    };
    if (tid < head) one(tid);
    for (int i = head + nvec * 8 + tid; i < V; i += 256) one(i);
    for (int q = tid; q < nvec; q += 256) {
        const int i = head + q * 8;
        typename Vec8<T>::type v = as_vec8<T>(ldg16(row + i));
        const unsigned s = ruled ? bits8(seen, i) : 0u, x = ruled ? bits8(ban, i) : 0u;
        v8us o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = cook(v[j], (s >> j) & 1u, (x >> j) & 1u);
        *(v8us*)(sr + i) = o;
    }
    __syncthreads();                     // words[] initialised (and the row complete for the other threads)
    atomicMax(&words[0], kmax);
    __syncthreads();
    const int maxkey = words[0];
    unsigned short maxbits = (unsigned short)((maxkey & 0x8000) ? (maxkey & 0x7fff) : (~maxkey & 0xffff));
    const float smax = tof<T>(from_bits16<T>(maxbits));

    // ---- top-k: the key of the min(k, V)-th largest value; smaller keys are dropped, ties with it stay
    int floor_key = 0;
    if (sp.top_k > 0 && sp.top_k < V) {
        int want = sp.top_k, hb = 0;
        for (int pass = 0; pass < 2; ++pass) {
            hcnt[tid] = 0;
            __syncthreads();
            for (int i = tid; i < V; i += 256) {
                const int k = (int)okey(sr[i]);
                if (pass == 0) atomicAdd(&hcnt[k >> 8], 1);
                else if ((k >> 8) == hb) atomicAdd(&hcnt[k & 255], 1);
            }
            __syncthreads();
            const int bin = 255 - tid;   // from the top: thread order = descending bins
            const u64s cnt = (u64s)hcnt[bin];
            u64s tot;
            const u64s S = block_scan256(cnt, scan, &tot);
            if (S >= (u64s)want && S - cnt < (u64s)want) { words[1 + 2 * pass] = bin; words[2] = want - (int)(S - cnt); }
            __syncthreads();
            if (pass == 0) { hb = words[1]; want = words[2]; }
        }
        floor_key = (words[1] << 8) | words[3];
        __syncthreads();
        if (tid == 0) { words[1] = -1; words[3] = -1; }
    }

    // ---- top-p over the survivors: the lowest key v with M(v) = mass(keys <= v) / mass(all) > 1 - p; smaller keys are dropped
    if (sp.top_p < 1.0f) {
        int pb = 0;
        u64s base = 0;
        double thr = 0.0;
        for (int pass = 0; pass < 2; ++pass) {
            hmass[tid] = 0;
            __syncthreads();
            for (int i = tid; i < V; i += 256) {
                const unsigned short u = sr[i];
                const int k = (int)okey(u);
                if (k < floor_key) continue;
                if (pass == 0) atomicAdd(&hmass[k >> 8], mass_q<T>(u, smax));
                else if ((k >> 8) == pb) atomicAdd(&hmass[k & 255], mass_q<T>(u, smax));
            }
            __syncthreads();
            const u64s m = hmass[tid];   // ascending bins
            u64s tot;
            const u64s S = block_scan256(m, scan, &tot) + base;
            if (pass == 0) thr = (1.0 - (double)sp.top_p) * (double)tot;
            if ((double)S > thr && !((double)(S - m) > thr)) {
                words[1 + 2 * pass] = tid;
                words[5] = (int)(unsigned)(S - m); words[6] = (int)(unsigned)((S - m) >> 32);
            }
            __syncthreads();
            if (pass == 0) {
                pb = words[1];
                base = (u64s)(unsigned)words[5] | ((u64s)(unsigned)words[6] << 32);
                if (pb < 0) break;       // uniform: no bin passes the threshold (a p below 2^-53, or an all -inf row): the maximum alone stays
            }
        }
        const int pkey = (words[1] < 0 || words[3] < 0) ? maxkey : ((words[1] << 8) | words[3]);
        floor_key = max(floor_key, pkey);
    }
    floor_key = min(floor_key, maxkey);  // the maximum always stays

    // ---- the draw: contiguous chunks in index order
    const int chunk = (V + 255) >> 8, i0 = min(V, tid * chunk), i1 = min(V, i0 + chunk);
    u64s mine = 0;
    for (int i = i0; i < i1; ++i) {
        const unsigned short u = sr[i];
        if ((int)okey(u) >= floor_key) mine += mass_q<T>(u, smax);
    }
    u64s c_last;
    const u64s incl = block_scan256(mine, scan, &c_last);
    uint32_t u24 = 0;
    {
        const u64s seed = *sp.seed;
        u24 = sample_u24((uint64_t)seed, (uint32_t)b, (uint32_t)gen);
    }
    const u64s target = __umul64hi((u64s)u24 << 40, c_last);         // (u24 * C_last) >> 24 < C_last
    if (c_last > 0 && incl > target && incl - mine <= target) {
        u64s cacc = incl - mine;
        int tok = i1 - 1;
        for (int i = i0; i < i1; ++i) {
            const unsigned short u = sr[i];
            if ((int)okey(u) >= floor_key) {
                cacc += mass_q<T>(u, smax);
                if (cacc > target) { tok = i; break; }
            }
        }
        words[4] = tok;
    }
    if (c_last == 0)                     // no mass anywhere (an all -inf or NaN row): the lowest index of the maximum, like the greedy kernels
        for (int i = i0; i < i1; ++i) if ((int)okey(sr[i]) == maxkey) { atomicMin(&words[4], i); break; }

    // ---- the processed row back to memory: what the caller's logits / scores hold (HF's .scores)
    const unsigned short ninf = bits16<T>(fromf<T>(-INFINITY));
    auto out1 = [&](unsigned short u) -> unsigned short { return (int)okey(u) >= floor_key ? u : ninf; };
    if (tid < head) row[tid] = from_bits16<T>(out1(sr[tid]));
    for (int i = head + nvec * 8 + tid; i < V; i += 256) row[i] = from_bits16<T>(out1(sr[i]));
    for (int q = tid; q < nvec; q += 256) {
        const int i = head + q * 8;
        v8us o = *(const v8us*)(sr + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = out1(o[j]);
        stg16(row + i, __builtin_bit_cast(u4, o));
    }
    __syncthreads();
    int tok = words[4];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    if (a.sel_out) {                     // the kernel-test hook: the selection alone, no decode state behind it
        if (tid == 0) a.sel_out[b] = tok;
        return;
    }
    step_tail<T>(t, b, tok);
}
// ---- avg_pool2d(pool) + NCHW flatten of the NHWC projector output (chexpert_model.py:17-18) ----------------------------
template <typename T>
__global__ void avgpool_flatten_k(const T* __restrict__ in, T* __restrict__ out, int B, int G, int C, int pool) {
    const int Gp = G / pool;                       // floor, like F.avg_pool2d
    const size_t total = (size_t)B * C * Gp * Gp;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int w = (int)(i % Gp), h = (int)((i / Gp) % Gp), c = (int)((i / ((size_t)Gp * Gp)) % C), b = (int)(i / ((size_t)Gp * Gp * C));
        float acc = 0.f;
        for (int dy = 0; dy < pool; ++dy)
            for (int dx = 0; dx < pool; ++dx)
                acc += tof<T>(in[(((size_t)b * G + h * pool + dy) * G + w * pool + dx) * C + c]);
        out[i] = fromf<T>(acc / (float)(pool * pool));      // x.view(B, -1) of [B][C][Gp][Gp]
    }
}
void launch_avgpool_flatten(int dtype, const void* in, void* out, int B, int G, int C, int pool, hipStream_t s) {
    const size_t total = (size_t)B * C * (G / pool) * (G / pool);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((avgpool_flatten_k<T>), dim3(blocks), dim3(256), 0, s, (const T*)in, (T*)out, B, G, C, pool));
}

void launch_greedy_step(int dtype, const float* part_val, const int* part_idx, int n_tiles, int B, const StepTail& t, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((greedy_step_k<T>), dim3(B), dim3(256), 0, s, part_val, part_idx, n_tiles, t));
}

bool select_step_supported(int vocab) { return vocab > 0 && select_step_lds(vocab) <= 48 * 1024; }

void launch_select_step(int dtype, const SelectArgs& a, const StepTail& t, int B, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((select_step_k<T>), dim3(B), dim3(256), select_step_lds(t.vocab), s, a, t));
}

bool sample_step_supported(int vocab) { return vocab > 0 && sample_step_lds(vocab) <= 144 * 1024; }     // of the CU's 160 KB; step_tail's own words on top

void launch_sample_step(int dtype, const SelectArgs& a, const SampleArgs& sp, const StepTail& t, int B, hipStream_t s) {
    const size_t smem = sample_step_lds(t.vocab);
    if (dtype == DT_F16) {
        static DevOnce attr;
        if (attr.first()) (void)hipFuncSetAttribute((const void*)sample_step_k<f16>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
    } else {
        static DevOnce attr;
        if (attr.first()) (void)hipFuncSetAttribute((const void*)sample_step_k<bf16>, hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024);
    }
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((sample_step_k<T>), dim3(B), dim3(256), smem, s, a, sp, t));
}

// the caller's ids replace the token the previous step appended (rdx_decode_step_ids under logits rules)
__global__ void hist_set_last_k(const int* __restrict__ ids, int* __restrict__ hist, const int* __restrict__ hist_len, int ld, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int L = hist_len[b];
    if (L > 0 && L <= ld) hist[(size_t)b * ld + L - 1] = ids[b];
}
void launch_hist_set_last(const int* ids, int* hist, const int* hist_len, int ld, int B, hipStream_t s) {
    hipLaunchKernelGGL(hist_set_last_k, dim3((B + 63) / 64), dim3(64), 0, s, ids, hist, hist_len, ld, B);
}

// the prompt becomes the rows' history: hist[b][0 .. T) = ids[b], hist_len[b] = T
__global__ void hist_init_k(const int* __restrict__ ids, int T_, int* __restrict__ hist, int* __restrict__ hist_len, int ld) {
    const int b = blockIdx.x;
    for (int t = threadIdx.x; t < T_ && t < ld; t += blockDim.x) hist[(size_t)b * ld + t] = ids[(size_t)b * T_ + t];
    if (threadIdx.x == 0) hist_len[b] = min(T_, ld);
}
void launch_hist_init(const int* ids, int B, int T_, int* hist, int* hist_len, int ld, hipStream_t s) {
    hipLaunchKernelGGL(hist_init_k, dim3(B), dim3(256), 0, s, ids, T_, hist, hist_len, ld);
}

}  // namespace rdx
