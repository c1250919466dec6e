// Batch 3-16 decode projections (gfx950): ONE MFMA row tile of 16 rows -- five launches per layer instead of the seven of the 32-row
// family (xstat32.hip). The reference's own evaluation batch is 12 (test.py:279,:344); its decoder layer is
// modeling_llama_imgemb.py:266-318 (RMSNorm -> q/k/v -> attention -> o_proj + residual -> RMSNorm -> SwiGLU MLP + residual).
//
// What the 32-row family pays for at 3-16 rows: (1) half of every activation fragment, MFMA and start-up fetch is padding; (2) the two
// 256-tile projections (o_proj, down_proj) run K-split over fp32 slabs because [32][11008] activations do not fit a workgroup, and the
// slab combine + residual + RMSNorm is a 5-us launch of its own in front of QKV and of gate/up. At 16 rows neither is needed:
//
//   xstat16_k   QKV / gate-up / lm_head, K = 4096: activation-stationary like xstat32_k (256 persistent 8-wave workgroups, wave w owns
//               k in [512 w, 512 w + 512), 16 fragments = 64 VGPRs), two output tiles per trip (a 32-fragment weight ring: 256 KiB per CU in
//               flight), and the RMSNorm is its PROLOGUE: the workgroup reads the 16 residual-stream rows row-major (a wave's row segment is
//               one contiguous KiB), takes the row statistics (lanes -> waves through LDS, fixed order), scales and rounds exactly like
//               rmsnorm4096_k -- T(w * T(x * rstd)) -- and turns the rows into MFMA B fragments through a wave-private, conflict-free LDS
//               patch (ds_write_b128 / ds_read_b128; the direct gather from row-major memory is 16 rows x 64 B per load instruction). The
//               rows are requested first and the first weight ring right behind them, so the arithmetic runs under the weights' flight.
//   xrow16_k    o_proj / down_proj (+ residual): one 16-wave workgroup per output tile, K split over its waves, weight fragments (HBM,
//               non-temporal) AND activation fragments (fragment-packed by the producer's epilogue, L2) streamed through one register ring,
//               fixed-order LDS reduction, residual epilogue writing the final rows -- no slabs, nothing left for a later launch.
//   xstat16_w4_k / xrow16_w4_k   the same two kernels for QKV, gate/up and down_proj of a context with int4 group-quantised weights (RDX_W_GEMM_W4): the
//               nibbles are streamed (4.125 bits per weight) and decoded in registers to the bits of the dequantised bf16 weight, fragment by fragment
//               in front of the same MFMAs in the same order -- the outputs are those of the bf16 kernels on the packed dequantised copy, bit for bit.
// Same rounding points as the GEMV / 32-row families (skinny_body.h): only the fp32 accumulation order differs.
#include <type_traits>
#include <algorithm>
#include "rdx_common.h"
#include "rdx_kernels.h"
#include "skinny_body.h"   // swiglu()

namespace rdx {

constexpr int X16_WAVES = 8, X16_THREADS = 512, X16_K = 4096, X16_CPW = X16_K / 32 / X16_WAVES;   // 16 chunks of 32 per wave
constexpr int X16_TPI = 2, X16_RING = X16_TPI * X16_CPW;                                             // 32 fragments = 32 KiB per wave in flight
constexpr int X16_QPW = X16_CPW * 32 / W4_CHUNK_K;                                                    // int4 weights: 4 chunks of 128 per wave and tile
constexpr int X16_TR_ROW = 1024 + 16;      // bytes per row of a wave's transpose patch: 16 rows land 4 banks apart (b128 accesses, 16 lanes per pass)
constexpr int X16_TR_WAVE = 16 * X16_TR_ROW;
constexpr size_t X16_SMEM = (size_t)X16_WAVES * X16_TR_WAVE + 1024;                                   // patches (the partial buffers alias them) + statistics

// W4 (bf16): the weights come as the int4 stream a.W4 (rdx_common.h W4Chunk) -- wave w's k range of a tile is exactly its chunks 4 w .. 4 w + 3 -- and
// fragment j of a chunk is decoded in registers (w4_frag<j>: the bits of the packed copy of W') right in front of its MFMA: the same MFMAs in the same
// order, so the same output bits. A tile whose header word has bit 8 set (the LoRA-A tile of the fused QKV weight) streams its packed bytes from a.W.
// An int4 chunk as it sits in a ring: the scale keeps its 16 loaded bits until the chunk is consumed. (Widened at the load -- rdx_common.h w4_load -- the
// widening instructions of a whole ring stand at the end of the block that issued the loads, each behind a wait for its load: the first fragment would be
// decoded only after the last chunk of the first ring has landed.)
struct W4Ring { u4 nib; unsigned short sc; };
__device__ __forceinline__ W4Ring w4_ring_load(const unsigned char* p16, const unsigned char* p2) {
    W4Ring c;
    c.nib = ldg16_nt(p16);
    c.sc = __builtin_nontemporal_load((const __attribute__((address_space(1))) unsigned short*)p2);
    return c;
}
__device__ __forceinline__ W4Chunk w4_ring_open(const W4Ring& c) {
    unsigned short s = c.sc;
    asm volatile("" : "+v"(s));       // nothing computed from the scale is scheduled above this point
    return W4Chunk{c.nib, s};
}

template <typename T, int EPI, bool W4>
__device__ __forceinline__ void xstat16_body(const GemmArgs& a) {
    typedef typename Vec8<T>::type V8;
    extern __shared__ __attribute__((aligned(16))) unsigned char smx[];
    float* red = reinterpret_cast<float*>(smx);                                   // aliases the transpose patches: a barrier separates the two uses
    float* ssq = reinterpret_cast<float*>(smx + (size_t)X16_WAVES * X16_TR_WAVE);  // [8 waves][16 rows]
    float* rstd_s = ssq + X16_WAVES * 16;                                          // [16]

    const int lane = threadIdx.x & 63, wa = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int ntiles = (a.N + 15) >> 4;
    const int G = gridDim.x;
    const int ngroups = (ntiles + X16_TPI - 1) / X16_TPI;
    const int nit = (ngroups - (int)blockIdx.x + G - 1) / G;
    if (nit <= 0) return;

    const u4* wbase = reinterpret_cast<const u4*>(a.W) + (size_t)(wa * X16_CPW) * 64;   // wave-uniform
    auto tile_ptr = [&](int t) { return wbase + (size_t)min(t, ntiles - 1) * (X16_K / 32) * 64; };

    // W4: the wave's four chunks of a tile; every address is clamped like tile_ptr's (a raw tile has a chunk too: quant_w4_k writes every tile's)
    const unsigned char* cbase = W4 ? reinterpret_cast<const unsigned char*>(a.W4) + (size_t)(wa * X16_QPW) * W4_CHUNK_BYTES : nullptr;
    auto chunk_ptr = [&](int t) { return cbase + (size_t)min(t, ntiles - 1) * (X16_K / W4_CHUNK_K * W4_CHUNK_BYTES); };
    const int off16 = lane * 16, off2 = 1024 + r * 2;
    // wave-uniform, through the constant address space: a scalar load (as a vector load it would be the newest in the queue, and waiting for it drains the ring)
    auto tile_hdr = [&](int t) { return *(reinterpret_cast<const __attribute__((address_space(4))) unsigned*>((uintptr_t)a.w4hdr) + min(t, ntiles - 1)); };

    typename std::conditional<W4, W4Ring, u4>::type ring[W4 ? X16_TPI * X16_QPW : X16_RING];
    auto first_ring = [&](int q) {
        if constexpr (W4) {
            const unsigned char* cp = chunk_ptr((int)blockIdx.x * X16_TPI + q);
#pragma unroll
            for (int j = 0; j < X16_QPW; ++j) {
                ring[q * X16_QPW + j] = w4_ring_load(cp + j * W4_CHUNK_BYTES + off16, cp + j * W4_CHUNK_BYTES + off2);
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            const u4* wp = tile_ptr((int)blockIdx.x * X16_TPI + q);
#pragma unroll
            for (int j = 0; j < X16_CPW; ++j) {
                ring[q * X16_CPW + j] = ldg16_nt(wp + (unsigned)(j * 64 + lane));
                __builtin_amdgcn_sched_barrier(0);               // issue order = consume order (the loop's counted waits rely on it)
            }
        }
    };
    // ---- activations -> B fragments xf[c]: column = row r of X, k = 512 wa + 32 c + 8 g .. + 8 ------------------------------------------
    const T* X = reinterpret_cast<const T*>(a.X);
    u4 xf[X16_CPW];
    u4 nw4;
    {
        // row-major rows, this wave's k range: lane holds k = 512 wa + 8 lane .. + 8 of every row. These 17 KiB per wave are
        // requested FIRST (whole-KiB row segments, L2 hits after the first workgroup of an XCD) and the weight ring right behind them, so the
        // prologue's arithmetic runs under the flight of the first weights and its wait (vmcnt = ring) does not drain them
        const T* xw = X + wa * 512 + lane * 8;
        nw4 = ldg16(reinterpret_cast<const T*>(a.norm_w) + wa * 512 + lane * 8);
#pragma unroll
        for (int i = 0; i < 16; ++i) xf[i] = ldg16(xw + (size_t)min(i, a.M - 1) * a.ldx);      // unconditional (a select would serialise the loads behind
                                                                                                // vmcnt(0)); rows >= M repeat the last row: never stored
        __builtin_amdgcn_sched_barrier(0);
    }
    // the first tile's weights; the second tile's follow BEHIND the prologue (its scaling temporaries and a 32-fragment ring do not fit the register
    // file together: 56 bytes of scratch when both were issued up front)
    // (W4: a tile's ring is 20 registers, not 64 -- both tiles go out up front)
    first_ring(0);
    if constexpr (W4) first_ring(1);
    {
        // LlamaRMSNorm (:85-93): fp32 mean of squares per row -- lanes (DPP), then waves through LDS in wave order
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const V8 xv = as_vec8<T>(xf[i]);
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) { const float f = tof<T>(xv[j]); ss += f * f; }
            ss = wave_sum(ss);
            if (lane == 0) ssq[wa * 16 + i] = ss;
        }
        __syncthreads();
        if (threadIdx.x < 16) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < X16_WAVES; ++i) t += ssq[i * 16 + threadIdx.x];
            rstd_s[threadIdx.x] = rsqrtf(t / (float)X16_K + a.eps);
        }
        __syncthreads();
        unsigned char* patch = smx + (size_t)wa * X16_TR_WAVE;
        const V8 nw = as_vec8<T>(nw4);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float rs = rstd_s[i];
            // opaque to the optimiser: it would otherwise keep the 128 fp32 conversions of the statistics pass alive for this one
            asm volatile("" : "+v"(xf[i].x), "+v"(xf[i].y), "+v"(xf[i].z), "+v"(xf[i].w));
            V8 xv = as_vec8<T>(xf[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) xv[j] = fromf<T>(tof<T>(nw[j]) * rnd<T>(tof<T>(xv[j]) * rs));     // weight * (x * rsqrt(var + eps)).to(dtype)
            *reinterpret_cast<u4*>(patch + i * X16_TR_ROW + lane * 16) = as_u4<T>(xv);
        }
        __builtin_amdgcn_wave_barrier();        // the patch is wave-private: LDS serves a wave's operations in order
#pragma unroll
        for (int c = 0; c < X16_CPW; ++c) xf[c] = *reinterpret_cast<const u4*>(patch + r * X16_TR_ROW + (4 * c + g) * 16);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!W4) first_ring(1);
        __syncthreads();                     // every wave has its fragments: the partial buffers may overwrite the patches
    }
    __builtin_amdgcn_sched_barrier(0);

    T* out = reinterpret_cast<T*>(a.out);
    if (a.out_step && out) out += (size_t)(*a.out_step) * a.out_step_stride;

    // epilogue coordinates: thread -> (tile of the trip, row, column)
    const int e_q = threadIdx.x >> 8, e_idx = threadIdx.x & 255, e_m = e_idx >> 4, e_nl = e_idx & 15;

    // The end of a trip: the waves' partial tiles through LDS buffer vit & 1 in wave order, then the epilogue. W4: hq = the header words of the trip's
    // tiles, and the trip stores the tiles whose raw bit equals raw_want (an int4 trip those that are not raw, a cold trip the raw ones).
    auto finish = [&](const v4f (&acc)[X16_TPI], int t0, int vit, float e_bias, const unsigned (&hq)[X16_TPI], unsigned raw_want) {
        const int t_o = t0 + e_q, n = t_o * 16 + e_nl;
        // D[n_local = 4 g + reg][m_local = r] -> red[buf][q][wave][m_local * 16 + n_local]
        float* rb = red + (size_t)(vit & 1) * (X16_TPI * X16_WAVES * 256);
#pragma unroll
        for (int q = 0; q < X16_TPI; ++q)
            *reinterpret_cast<float4*>(&rb[(q * X16_WAVES + wa) * 256 + r * 16 + g * 4]) = make_float4(acc[q][0], acc[q][1], acc[q][2], acc[q][3]);
        __syncthreads();
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < X16_WAVES; ++i) v += rb[(e_q * X16_WAVES + i) * 256 + e_idx];
        v += e_bias;
        const bool mine = t_o < ntiles && (!W4 || (((e_q ? hq[1] : hq[0]) >> 8) & 1u) == raw_want);
        const bool ok = (e_m < a.M) && mine && (n < a.N);
        if (EPI == EPI_NONE) {
            if (ok) out[(size_t)e_m * a.ldo + n] = fromf<T>(v);
        } else if (EPI == EPI_SILU_MUL) {
            // rows 0-7 of a tile are gate, 8-15 the matching up rows: the partner sits 8 lanes away in the same DPP row
            const float u = dpp_mov<DPP_ROR8>(v);
            if (a.out_packed != ACT_ROWS) {
                // the 32-row fragment-packed block xrow16_k reads (row tile 0 of [f = k / 32][mt][lane (g = (k % 32) / 8, r = m)][8]): this
                // tile's 8 outputs k = 8 t_o .. + 8 of row m are one lane's 16-byte piece; rows >= M are zero-filled
                if (e_nl < 8 && mine)
                    out[((size_t)(((t_o >> 2) * 2) * 64 + (t_o & 3) * 16 + e_m) << 3) + e_nl] = e_m < a.M ? fromf<T>(swiglu<T>(v, u)) : fromf<T>(0.f);
            } else if (e_nl < 8 && ok) out[(size_t)e_m * a.ldo + t_o * 8 + e_nl] = fromf<T>(swiglu<T>(v, u));
        } else if (EPI == EPI_LOGITS) {
            float lv = rnd<T>(v);
            int li = n;
            const bool valid = n < a.n_valid && t_o < ntiles;
            if (valid && e_m < a.M && out) out[(size_t)e_m * a.ldo + n] = fromf<T>(lv);
            if (!valid) { lv = -INFINITY; li = 0x7fffffff; }
            // argmax over the tile's 16 columns (16 consecutive lanes share m); ties -> lowest index (torch.argmax)
#pragma unroll
            for (int sh = 8; sh > 0; sh >>= 1) {
                const float ov = __shfl_xor(lv, sh, 64);
                const int oi = __shfl_xor(li, sh, 64);
                if (ov > lv || (ov == lv && oi < li)) { lv = ov; li = oi; }
            }
            if (e_nl == 0 && e_m < a.M && t_o < ntiles) {
                a.part_val[(size_t)e_m * ntiles + t_o] = lv;
                a.part_idx[(size_t)e_m * ntiles + t_o] = li;
            }
        }
    };
    auto bias_of = [&](int t0) {
        const int n = (t0 + e_q) * 16 + e_nl;
        return a.bias ? a.bias[min(n, a.N - 1)] : 0.f;
    };

    // One trip: the ring's two tiles multiplied, the ring refilled (PF) with the tiles of the next trip, finish(). W4: BOTH tiles are decoded and
    // multiplied whatever their header words say (a raw tile's chunk holds zeros) and only the tiles that are not raw are stored; the raw tiles -- one
    // tile of the fused QKV weight -- get cold_trip behind the last trip. Inside this trip, as an arm of a wave-uniform branch or as a block stepped over
    // on an opaque flag, the raw loads sat on a path into the int4 form and its waits were counted along it: vmcnt(6) and (3) where (14) stand now.
    auto trip = [&](int it, auto pf_tag) {
        constexpr bool PF = decltype(pf_tag)::value;
        const int t0 = ((int)blockIdx.x + it * G) * X16_TPI;
        unsigned hq[X16_TPI] = {};
        if constexpr (W4) {
#pragma unroll
            for (int q = 0; q < X16_TPI; ++q) hq[q] = tile_hdr(t0 + q);
        }
        const float e_bias = bias_of(t0);
        v4f acc[X16_TPI];
#pragma unroll
        for (int q = 0; q < X16_TPI; ++q) {
            acc[q] = (v4f){0.f, 0.f, 0.f, 0.f};
            if constexpr (W4) {
                const unsigned char* cn = chunk_ptr(t0 + G * X16_TPI + q);
#pragma unroll
                for (int j = 0; j < X16_QPW; ++j) {
                    const W4Chunk ch = w4_ring_open(ring[q * X16_QPW + j]);
                    acc[q] = mfma16(as_vec8<T>(w4_frag<0>(ch)), as_vec8<T>(xf[4 * j]), acc[q]);
                    acc[q] = mfma16(as_vec8<T>(w4_frag<1>(ch)), as_vec8<T>(xf[4 * j + 1]), acc[q]);
                    acc[q] = mfma16(as_vec8<T>(w4_frag<2>(ch)), as_vec8<T>(xf[4 * j + 2]), acc[q]);
                    acc[q] = mfma16(as_vec8<T>(w4_frag<3>(ch)), as_vec8<T>(xf[4 * j + 3]), acc[q]);
                    if (PF) ring[q * X16_QPW + j] = w4_ring_load(cn + j * W4_CHUNK_BYTES + off16, cn + j * W4_CHUNK_BYTES + off2);
                    __builtin_amdgcn_sched_barrier(0);       // consume-j / refill-j order, two loads per chunk: the waits stay vmcnt(2 RING - 2)
                }
            } else {
                const u4* wn = tile_ptr(t0 + G * X16_TPI + q);
#pragma unroll
                for (int j = 0; j < X16_CPW; ++j) {
                    acc[q] = mfma16(as_vec8<T>(ring[q * X16_CPW + j]), as_vec8<T>(xf[j]), acc[q]);
                    if (PF) ring[q * X16_CPW + j] = ldg16_nt(wn + (unsigned)(j * 64 + lane));
                    __builtin_amdgcn_sched_barrier(0);           // consume-j / refill-j order: the waits stay vmcnt(RING - 1)
                }
            }
        }
        finish(acc, t0, it, e_bias, hq, 0u);
    };
    // W4: the raw tiles of trip `it` (wave-uniform): a tile's 16 packed fragments loaded from a.W and waited for, multiplied, stored
    auto cold_trip = [&](int it, int vit) {
        const int t0 = ((int)blockIdx.x + it * G) * X16_TPI;
        const unsigned hq[X16_TPI] = {tile_hdr(t0), tile_hdr(t0 + 1)};
        v4f acc[X16_TPI];
#pragma unroll
        for (int q = 0; q < X16_TPI; ++q) {
            acc[q] = (v4f){0.f, 0.f, 0.f, 0.f};
            if (hq[q] & 0x100u) {
                const u4* wr = tile_ptr(t0 + q);
                u4 rw[X16_CPW];
#pragma unroll
                for (int j = 0; j < X16_CPW; ++j) rw[j] = ldg16_nt(wr + (unsigned)(j * 64 + lane));
#pragma unroll
                for (int j = 0; j < X16_CPW; ++j) acc[q] = mfma16(as_vec8<T>(rw[j]), as_vec8<T>(xf[j]), acc[q]);
            }
        }
        finish(acc, t0, vit, bias_of(t0), hq, 1u);
    };

    // the first trip is peeled: its waits cover the activation loads (newest in the queue), the loop's stay counted
    if (nit > 1) {
        trip(0, std::true_type{});
        for (int it = 1; it + 1 < nit; ++it) trip(it, std::true_type{});
    }
    trip(nit - 1, std::false_type{});
    if constexpr (W4) {
        int vit = nit;          // the cold trips go on alternating the LDS buffers
        for (int it = 0; it < nit; ++it) {
            const int t0 = ((int)blockIdx.x + it * G) * X16_TPI;
            if ((tile_hdr(t0) | (t0 + 1 < ntiles ? tile_hdr(t0 + 1) : 0u)) & 0x100u) cold_trip(it, vit++);
        }
    }
}

template <typename T, int EPI>
__global__ __launch_bounds__(X16_THREADS) void xstat16_k(GemmArgs a) { xstat16_body<T, EPI, false>(a); }

// QKV (EPI_NONE) and gate/up (EPI_SILU_MUL) on the int4 stream: 4.125 bits per weight from HBM instead of 16
template <int EPI>
__global__ __launch_bounds__(X16_THREADS) void xstat16_w4_k(GemmArgs a) { xstat16_body<bf16, EPI, true>(a); }

// ---- un-split o_proj / down_proj with the residual epilogue ---------------------------------------------------------------------------
// One workgroup per 16-column output tile, XR_WAVES waves split K evenly in whole 32-deep chunks. Per chunk a wave needs one KiB of weights
// (fragment-packed, HBM, read once: non-temporal) and one KiB of activations (row tile 0 of the producer's fragment-packed 32-row block: every
// workgroup reads the same block, L2-resident); both go through one register ring of XR_U chunk pairs refilled pair by pair as the MFMAs consume
// them. At 16 rows there is one tile per workgroup, so nothing would be gained by parking the activations anywhere.
constexpr int XR_WAVES = 16, XR_THREADS = XR_WAVES * 64, XR_U = 8;

template <typename T>
__global__ __launch_bounds__(XR_THREADS) void xrow16_k(GemmArgs a) {
    __shared__ __attribute__((aligned(16))) float red[XR_WAVES][256];
    const int lane = threadIdx.x & 63, wa = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x;
    const int KC = a.K >> 5;
    const int c0 = (KC * wa) / XR_WAVES, c1 = (KC * (wa + 1)) / XR_WAVES;       // wave-uniform; c1 - c0 >= 1 (K >= 512)
    const int clast = c1 - 1;
    const u4* wp = reinterpret_cast<const u4*>(a.W) + (size_t)tile * KC * 64 + lane;
    const T* X = reinterpret_cast<const T*>(a.X);
    // fragment (c, mt = 0) of the packed block. At <= 8 (<= 4) rows the lanes of the padding rows re-read row r - 8 (r & 3): their MFMA columns are never stored, and
    // the fragment's second 128-byte line per lane group (half of each line) is not fetched at all -- at K = 11008 the activations are as many L2 -> CU bytes as the weights
    const int xlane = a.M <= 4 ? (lane & ~12) : a.M <= 8 ? (lane & ~8) : (a.M <= 12 && (lane & 12) == 12) ? lane - 4 : lane;      // (9-12 rows: rows 12-15 re-read 8-11 -- half a line)
    auto xaddr = [&](int c) { return X + (size_t)(((c * 2) * 64 + xlane) * 8); };

    u4 wr[XR_U], xr[XR_U];
#pragma unroll
    for (int u = 0; u < XR_U; ++u) {
        const int c = min(c0 + u, clast);
        wr[u] = ldg16_nt(wp + (size_t)c * 64);
        xr[u] = ldg16(xaddr(c));
        __builtin_amdgcn_sched_barrier(0);
    }
    // the residual of this thread's output: requested behind the first ring, consumed in the epilogue
    const int e_m = (threadIdx.x & 255) >> 4, e_nl = threadIdx.x & 15, n = tile * 16 + e_nl;
    unsigned short res_bits = 0;
    if (threadIdx.x < 256) res_bits = reinterpret_cast<const unsigned short*>(a.resid)[(size_t)min(e_m, a.M - 1) * a.ldr + min(n, a.N - 1)];

    v4f acc = (v4f){0.f, 0.f, 0.f, 0.f};
    int cb = c0;
    for (; cb + XR_U < c1; cb += XR_U) {
#pragma unroll
        for (int u = 0; u < XR_U; ++u) {
            acc = mfma16(as_vec8<T>(wr[u]), as_vec8<T>(xr[u]), acc);
            const int c = min(cb + XR_U + u, clast);            // past the slice: re-read its last chunk (never multiplied)
            wr[u] = ldg16_nt(wp + (size_t)c * 64);
            xr[u] = ldg16(xaddr(c));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#pragma unroll
    for (int u = 0; u < XR_U; ++u)
        if (cb + u < c1) acc = mfma16(as_vec8<T>(wr[u]), as_vec8<T>(xr[u]), acc);      // wave-uniform guard
    *reinterpret_cast<float4*>(&red[wa][r * 16 + g * 4]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    __syncthreads();
    if (threadIdx.x < 256) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < XR_WAVES; ++i) v += red[i][threadIdx.x];
        if (e_m < a.M && n < a.N)
            reinterpret_cast<T*>(a.out)[(size_t)e_m * a.ldo + n] = fromf<T>(tof<T>(from_bits16<T>(res_bits)) + rnd<T>(v));
    }
}

// down_proj on the int4 stream (bf16, K % 128 == 0). The waves' slices [c0, c1) of 32-deep chunks, the accumulation order inside a slice and the LDS
// reduction are xrow16_k's, so the output bits are. A slice is covered by the int4 chunks [q0, q1) (128 k = four packed chunks each); where a slice edge
// cuts an int4 chunk (K = 11008: every one) both neighbouring waves load it and each decodes only its own fragments -- a wave-uniform test, outside the
// loop: the first trip and the tail are guarded, the trips between them hold whole chunks only. Weights: XR4_RW int4 chunks in flight per wave (HBM,
// non-temporal); activations: the four fragments of XR4_RX chunks (L2), the depth of xrow16_k's ring. No tile of a weight this kernel is given is raw
// (only the fused QKV weight has raw tiles, rdx_set_weight): the header words are not read.
constexpr int XR4_RW = 4, XR4_RX = 2;

__global__ __launch_bounds__(XR_THREADS) void xrow16_w4_k(GemmArgs a) {
    typedef bf16 T;
    __shared__ __attribute__((aligned(16))) float red[XR_WAVES][256];
    const int lane = threadIdx.x & 63, wa = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int tile = blockIdx.x;
    const int KC = a.K >> 5, KQ = a.K >> 7;
    const int c0 = (KC * wa) / XR_WAVES, c1 = (KC * (wa + 1)) / XR_WAVES;       // wave-uniform; c1 - c0 >= 1 (K >= 512)
    const int clast = c1 - 1;
    const int q0 = c0 >> 2, q1 = (c1 + 3) >> 2, qlast = q1 - 1;                 // the int4 chunks the slice touches: q1 - q0 >= 1, qlast < KQ
    const unsigned char* wp16 = reinterpret_cast<const unsigned char*>(a.W4) + (size_t)tile * KQ * W4_CHUNK_BYTES + lane * 16;
    const unsigned char* wp2 = reinterpret_cast<const unsigned char*>(a.W4) + (size_t)tile * KQ * W4_CHUNK_BYTES + 1024 + r * 2;
    const T* X = reinterpret_cast<const T*>(a.X);
    const int xlane = a.M <= 4 ? (lane & ~12) : a.M <= 8 ? (lane & ~8) : (a.M <= 12 && (lane & 12) == 12) ? lane - 4 : lane;      // as xrow16_k
    auto xaddr = [&](int c) { return X + (size_t)(((c * 2) * 64 + xlane) * 8); };

    W4Ring wr[XR4_RW];
    u4 xr[XR4_RX][4];
    // past the slice: its last chunk again (never multiplied); a fragment of a neighbouring wave: the slice's nearest one
    auto wload = [&](int q) { const size_t o = (size_t)min(q, qlast) * W4_CHUNK_BYTES; return w4_ring_load(wp16 + o, wp2 + o); };
    auto xload = [&](u4 (&x)[4], int q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = ldg16(xaddr(min(max(4 * q + j, c0), clast)));
    };
#pragma unroll
    for (int u = 0; u < XR4_RW; ++u) {
        wr[u] = wload(q0 + u);
        if (u < XR4_RX) xload(xr[u], q0 + u);
        __builtin_amdgcn_sched_barrier(0);
    }
    const int e_m = (threadIdx.x & 255) >> 4, e_nl = threadIdx.x & 15, n = tile * 16 + e_nl;
    unsigned short res_bits = 0;
    if (threadIdx.x < 256) res_bits = reinterpret_cast<const unsigned short*>(a.resid)[(size_t)min(e_m, a.M - 1) * a.ldr + min(n, a.N - 1)];

    v4f acc = (v4f){0.f, 0.f, 0.f, 0.f};
    auto consume = [&](const W4Ring& wq, const u4 (&x)[4], int q, auto guard_tag) {
        constexpr bool GUARD = decltype(guard_tag)::value;
        const W4Chunk w = w4_ring_open(wq);
        const int c = 4 * q;
        if (!GUARD || (c >= c0 && c < c1)) acc = mfma16(as_vec8<T>(w4_frag<0>(w)), as_vec8<T>(x[0]), acc);
        if (!GUARD || (c + 1 >= c0 && c + 1 < c1)) acc = mfma16(as_vec8<T>(w4_frag<1>(w)), as_vec8<T>(x[1]), acc);
        if (!GUARD || (c + 2 >= c0 && c + 2 < c1)) acc = mfma16(as_vec8<T>(w4_frag<2>(w)), as_vec8<T>(x[2]), acc);
        if (!GUARD || (c + 3 >= c0 && c + 3 < c1)) acc = mfma16(as_vec8<T>(w4_frag<3>(w)), as_vec8<T>(x[3]), acc);
    };
    auto trip = [&](int q, auto guard_tag) {
#pragma unroll
        for (int u = 0; u < XR4_RW; ++u) {
            consume(wr[u], xr[u % XR4_RX], q + u, guard_tag);
            wr[u] = wload(q + XR4_RW + u);
            xload(xr[u % XR4_RX], q + XR4_RX + u);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    int q = q0;
    if (q + XR4_RW < q1) { trip(q, std::true_type{}); q += XR4_RW; }       // the trip that holds the slice's first chunk
    for (; q + XR4_RW < q1; q += XR4_RW) trip(q, std::false_type{});
#pragma unroll
    for (int u = 0; u < XR4_RW; ++u)
        if (q + u < q1) {                                                   // wave-uniform
            consume(wr[u], xr[u % XR4_RX], q + u, std::true_type{});
            if (q + u + XR4_RX < q1) xload(xr[u % XR4_RX], q + u + XR4_RX);
        }
    *reinterpret_cast<float4*>(&red[wa][r * 16 + g * 4]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    __syncthreads();
    if (threadIdx.x < 256) {
        float v = 0.f;
#pragma unroll
        for (int i = 0; i < XR_WAVES; ++i) v += red[i][threadIdx.x];
        asm volatile("" : "+v"(res_bits));      // its widening stays here (hoisted to the load, its wait drains the first ring in front of the first MFMA)
        if (e_m < a.M && n < a.N)
            reinterpret_cast<T*>(a.out)[(size_t)e_m * a.ldo + n] = fromf<T>(tof<T>(from_bits16<T>(res_bits)) + rnd<T>(v));
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
bool xs16_rows_ok(int M) { return M >= 3 && M <= 16; }

bool xstat16_supported(const GemmArgs& a, int epi) {
    return xs16_rows_ok(a.M) && a.K == X16_K && a.W && !a.W8 && (a.N + 15) / 16 >= 512 && a.norm_w && a.ldx % 8 == 0 && a.xpacked == ACT_ROWS &&
           (epi == EPI_NONE || epi == EPI_SILU_MUL || epi == EPI_LOGITS);
}

template <typename T, int EPI>
static void launch_xstat16_e(const GemmArgs& a, dim3 grid, hipStream_t s) {
    static DevOnce attr;
    if (attr.first()) (void)hipFuncSetAttribute((const void*)xstat16_k<T, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)X16_SMEM);
    hipLaunchKernelGGL((xstat16_k<T, EPI>), grid, dim3(X16_THREADS), X16_SMEM, s, a);          // always with the RMSNorm prologue (xstat16_supported)
}

static int xstat16_grid(const GemmArgs& a) {
    const int nt = (a.N + 15) / 16, groups = (nt + X16_TPI - 1) / X16_TPI;
    // 256 workgroups, unless the last round would be less than half full: then fewer workgroups with the same number of trips each (xstat32.hip)
    int g = groups < 256 ? groups : 256;
    const int rem = groups % 256;
    if (groups > 256 && rem && rem < 128) { const int trips = (groups + 255) / 256; g = (groups + trips - 1) / trips; }
    return g;
}

void launch_xstat16(int dtype, const GemmArgs& a, int epi, hipStream_t s) {
    const int g = xstat16_grid(a);
    RDX_DISPATCH_T(dtype, T, {
        if (epi == EPI_NONE) launch_xstat16_e<T, EPI_NONE>(a, dim3(g), s);
        else if (epi == EPI_SILU_MUL) launch_xstat16_e<T, EPI_SILU_MUL>(a, dim3(g), s);
        else if (epi == EPI_LOGITS) launch_xstat16_e<T, EPI_LOGITS>(a, dim3(g), s);
    });
}

// X: the fragment-packed 32-row block (row tile 0 is read); resid / out row-major
bool xrow16_supported(const GemmArgs& a) {
    return xs16_rows_ok(a.M) && a.W && !a.W8 && a.K % 32 == 0 && a.K >= 32 * XR_WAVES && a.N % 16 == 0 && a.xpacked == ACT_BLK32 && a.resid && !a.bias && !a.norm_w;
}

void launch_xrow16(int dtype, const GemmArgs& a, hipStream_t s) {
    RDX_DISPATCH_T(dtype, T, hipLaunchKernelGGL((xrow16_k<T>), dim3(a.N / 16), dim3(XR_THREADS), 0, s, a));
}

// ---- the int4 forms: the shapes of the bf16 kernels, an int4 stream with its header words, and the packed copy of W' for the raw tiles ----
bool xstat16_w4_supported(int dtype, const GemmArgs& a, int epi) {
    return dtype == DT_BF16 && a.W4 && a.w4hdr && xstat16_supported(a, epi) && (epi == EPI_NONE || epi == EPI_SILU_MUL);
}

template <int EPI>
static void launch_xstat16_w4_e(const GemmArgs& a, hipStream_t s) {
    static DevOnce attr;
    if (attr.first()) (void)hipFuncSetAttribute((const void*)xstat16_w4_k<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)X16_SMEM);
    hipLaunchKernelGGL((xstat16_w4_k<EPI>), dim3(xstat16_grid(a)), dim3(X16_THREADS), X16_SMEM, s, a);
}

void launch_xstat16_w4(const GemmArgs& a, int epi, hipStream_t s) {
    if (epi == EPI_NONE) launch_xstat16_w4_e<EPI_NONE>(a, s);
    else if (epi == EPI_SILU_MUL) launch_xstat16_w4_e<EPI_SILU_MUL>(a, s);
}

bool xrow16_w4_supported(int dtype, const GemmArgs& a) {
    return dtype == DT_BF16 && a.W4 && a.w4hdr && xrow16_supported(a) && a.K % W4_CHUNK_K == 0;
}

void launch_xrow16_w4(const GemmArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(xrow16_w4_k, dim3(a.N / 16), dim3(XR_THREADS), 0, s, a);
}

}  // namespace rdx
