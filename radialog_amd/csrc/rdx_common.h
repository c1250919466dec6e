// Shared device/host helpers for librdx (gfx950 / CDNA4 only: 64-wide wavefronts, MFMA 16x16x32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "rdx_kernels.h"

namespace rdx {

typedef _Float16 f16;
typedef __bf16 bf16;
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
typedef unsigned int u2 __attribute__((ext_vector_type(2)));
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef __bf16 v8b __attribute__((ext_vector_type(8)));

enum DType { DT_F16 = 0, DT_BF16 = 1 };

// ---- scalar conversions (round-to-nearest-even, the rounding torch's .to(half/bfloat16) applies) --------------
template <typename T> __device__ __forceinline__ float tof(T x) { return (float)x; }
template <typename T> __device__ __forceinline__ T fromf(float x) { return (T)x; }
// round a float through T and back: the "every torch op rounds its output to the model dtype" emulation
template <typename T> __device__ __forceinline__ float rnd(float x) { return (float)((T)x); }

template <typename T> struct Vec8;           // 8 x T in one 16-byte register quad
template <> struct Vec8<f16> { typedef v8h type; };
template <> struct Vec8<bf16> { typedef v8b type; };

template <typename T> __device__ __forceinline__ typename Vec8<T>::type as_vec8(u4 v) {
    return __builtin_bit_cast(typename Vec8<T>::type, v);
}
template <typename T> __device__ __forceinline__ unsigned short bits16(T v) { return __builtin_bit_cast(unsigned short, v); }
template <typename T> __device__ __forceinline__ T from_bits16(unsigned short b) { return __builtin_bit_cast(T, b); }
template <typename T> __device__ __forceinline__ u4 as_u4(typename Vec8<T>::type v) { return __builtin_bit_cast(u4, v); }

__device__ __forceinline__ v4f mfma16(v8h a, v8h b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v4f mfma16(v8b a, v8b b, v4f c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// 16-byte GLOBAL-memory loads/stores. `ldg_nt` = streamed-once data (decode weights): non-temporal policy.
// The explicit address_space(1) cast matters: a pointer that does not come straight from a kernel argument is generic, and
// generic accesses become FLAT instructions, whose completion order is not guaranteed -- the compiler then falls back
// to s_waitcnt vmcnt(0) everywhere and a software-pipelined weight stream collapses to one batch in flight.
typedef __attribute__((address_space(1))) u4 g_u4;
// Kernel arguments read LATE (the batch-1/2 step: gemm.hip skinny_gemm_k, chain.hip). What a launch's first loads are addressed from travels as leading
// scalar arguments, which kernarg preloading (build.py UNIT_FLAGS) has in SGPRs when the first wave starts; the rest is a struct by value behind them.
// The compiler would load that struct's fields where the kernel begins -- common fields of a kernel's roles end up in its entry block, with a wait for
// them in front of everything. late_kernarg<A>(offset) copies the struct found `offset` bytes into the kernarg segment through a pointer that an empty
// volatile asm has made opaque: its scalar loads are issued at the call, and no memory access of the program is moved across it. `offset` is the
// struct's offset in the kernel's argument list: kernarg_offset<I>(kernel) computes it from the kernel's OWN signature (argument I, counted from 0;
// the kernarg segment lays the arguments out in order, each at its natural alignment), so an argument added or moved moves the offset with it.
template <int I, typename... A> constexpr unsigned kernarg_offset_of() {
    static_assert(I >= 0 && I < (int)sizeof...(A), "no such kernel argument");
    unsigned off = 0, r = 0;
    int i = 0;
    ((off = (off + (unsigned)alignof(A) - 1u) / (unsigned)alignof(A) * (unsigned)alignof(A), r = (i == I ? off : r), off += (unsigned)sizeof(A), ++i), ...);
    return r;
}
template <int I, typename... A> constexpr unsigned kernarg_offset(void (*)(A...)) { return kernarg_offset_of<I, A...>(); }
template <typename A> __device__ __forceinline__ A late_kernarg(unsigned offset) {
    typedef __attribute__((address_space(4))) const unsigned char kbyte;
    typedef __attribute__((address_space(4))) const A kA;          // typed: the copy is made of aligned dword loads, which the scalar unit can do
    kA* p = (kA*)((kbyte*)__builtin_amdgcn_kernarg_segment_ptr() + offset);
    asm volatile("" : "+s"(p) :: "memory");
    A a;
    __builtin_memcpy(&a, p, sizeof(A));
    return a;
}
__device__ __forceinline__ u4 ldg16(const void* p) { return *(const g_u4*)p; }
__device__ __forceinline__ u4 ldg16_nt(const void* p) { return __builtin_nontemporal_load((const g_u4*)p); }
__device__ __forceinline__ void stg16(void* p, u4 v) { *(g_u4*)p = v; }

// ---- fp8 (OCP e4m3) -> model dtype, exact (every e4m3 value is representable in bf16 and f16) --------------------------------
// two dwords = 8 fp8 bytes -> 8 model-dtype values in one 16-byte register quad (an MFMA A-operand chunk)
template <typename T> __device__ __forceinline__ u4 dequant8(unsigned lo, unsigned hi);
template <> __device__ __forceinline__ u4 dequant8<bf16>(unsigned lo, unsigned hi) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    // bf16 = upper half of the f32 (exact here): (f0.hi16) | (f1.hi16 << 16). The elements are copied to scalars first:
    // __builtin_bit_cast on a vector ELEMENT (a[1]) reads element 0 with this compiler.
    const float a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1], c0 = c[0], c1 = c[1], d0 = d[0], d1 = d[1];
    return (u4){__builtin_amdgcn_perm(__builtin_bit_cast(unsigned, a1), __builtin_bit_cast(unsigned, a0), 0x07060302u),
                __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, b1), __builtin_bit_cast(unsigned, b0), 0x07060302u),
                __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, c1), __builtin_bit_cast(unsigned, c0), 0x07060302u),
                __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, d1), __builtin_bit_cast(unsigned, d0), 0x07060302u)};
}
template <> __device__ __forceinline__ u4 dequant8<f16>(unsigned lo, unsigned hi) {
    const auto a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
    const auto c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
    return (u4){__builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(a[0], a[1])), __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(b[0], b[1])),
                __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(c[0], c[1])), __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(d[0], d[1]))};
}

// ---- fp8 KV cache ("kv8": e4m3 codes with one power-of-two exponent per cache row of 128; the format's definition is radialog_amd/kv8.py) ----
// The stored row IS x' = code * 2^e, exactly a bf16 and an f16 value (e >= -15), so the expansion below is exact and the cache reads as a T cache
// holding x'. Two codes times the scale become a packed T pair in one VALU instruction (v_cvt_scalef32_pk_{bf16,f16}_fp8).
constexpr int KV8_EMIN = -15;
__device__ __forceinline__ float kv8_scale(int e) { return __builtin_bit_cast(float, (unsigned)(e + 127) << 23); }       // 2^e, e in [-126, 127]
template <typename T, bool HI> __device__ __forceinline__ unsigned kv8_pk(unsigned w, float s);       // codes 2 HI, 2 HI + 1 of w, times s
template <> __device__ __forceinline__ unsigned kv8_pk<bf16, false>(unsigned w, float s) { return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, false)); }
template <> __device__ __forceinline__ unsigned kv8_pk<bf16, true>(unsigned w, float s) { return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, s, true)); }
template <> __device__ __forceinline__ unsigned kv8_pk<f16, false>(unsigned w, float s) { return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, s, false)); }
template <> __device__ __forceinline__ unsigned kv8_pk<f16, true>(unsigned w, float s) { return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w, s, true)); }
// two dwords = 8 codes -> 8 T values x' in one 16-byte register quad (an MFMA A-operand chunk, or 8 dims of a V row)
template <typename T> __device__ __forceinline__ u4 kv8_expand(unsigned lo, unsigned hi, float s) {
    return (u4){kv8_pk<T, false>(lo, s), kv8_pk<T, true>(lo, s), kv8_pk<T, false>(hi, s), kv8_pk<T, true>(hi, s)};
}
// the row exponent of radialog_amd/kv8.py from the row's absmax (a T value held in fp32, finite): the smallest e >= -15 with amax 2^-e <= 448. With
// frexp(amax) = (m, ex), ex = E - 126 and m <= 0.875 <=> mantissa field <= 0x600000. Zero and fp32-subnormal rows (E = 0) clamp to -15.
__device__ __forceinline__ int kv8_exp(float amax) {
    const unsigned u = __builtin_bit_cast(unsigned, amax);
    const int E = (int)((u >> 23) & 0xffu);
    return max(E - 135 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0), KV8_EMIN);
}
// 8 values of a row (fp32 copies of T values) -> 8 codes RNE_e4m3(x 2^-e): the scaling is exact (or underflows below half the smallest code), one rounding
__device__ __forceinline__ u2 kv8_quant8(const float (&x)[8], int e) {
    const float inv = kv8_scale(-e);
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[0] * inv, x[1] * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(x[2] * inv, x[3] * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[4] * inv, x[5] * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(x[6] * inv, x[7] * inv, hi, true);
    return (u2){(unsigned)lo, (unsigned)hi};
}
// K codes inside one (row, head) slab [max_len][128] bytes: every group of 16 positions is stored [g = (dim % 32) / 8][r = pos % 16][dim / 32][8], so
// the 32 bytes of an MFMA A-fragment lane (g, r) -- its four 8-dim pieces -- are contiguous and a wave's group is ONE contiguous 2 KiB. V codes are row-major.
__host__ __device__ __forceinline__ size_t kperm8(int pos, int dim) {
    return (size_t)(pos >> 4) * 2048 + (size_t)((((dim & 31) >> 3) * 16 + (pos & 15)) * 32 + (dim >> 5) * 8 + (dim & 7));
}
typedef __attribute__((address_space(1))) u2 g_u2;
__device__ __forceinline__ u2 ldg8(const void* p) { return *(const g_u2*)p; }
__device__ __forceinline__ void stg8(void* p, u2 v) { *(g_u2*)p = v; }
__device__ __forceinline__ int ldg1s(const void* p) { return *(const __attribute__((address_space(1))) signed char*)p; }
__device__ __forceinline__ void stg1s(void* p, int v) { *(__attribute__((address_space(1))) signed char*)p = (signed char)v; }

// ---- coded bf16 weights ("WC", 13 bits per weight, exact; the format's definition is radialog_amd/wcode.py) ------------------------------
// A coded chunk is 128 k-values of one 16-row tile = four of the packed 32-k chunks, WC_CHUNK_BYTES bytes in three planes, each a run of whole-wave
// contiguous loads: [lo0: 64 lanes x 16 B][lo1: 64 x 16 B][idx: 64 x 16 B][sign: 64 x 4 B]. Lane (g, r) holds the 32 weights of ITS four MFMA A
// fragments j = 0..3 (fragment j = the lane's 16 bytes of packed chunk 4 q + j), weight e = 0..7 of fragment j:
//   low byte (e0 m6..m0), verbatim: byte 8 (j & 1) + e of lo0 (j < 2) or lo1;
//   4-bit index: dword j of the idx plane, nibble 2 e (e < 4) or 2 (e - 4) + 1 -- so the even nibbles are weights 0..3 and the odd ones 4..7;
//   sign: bit (2 j + e / 4) + 8 (e % 4) of the sign dword.
// The high byte is sign << 7 | h with h = (e7..e1) = 0 for index 0 and base + index otherwise; base comes from the tile's header word
// (bits 0..7; bit 8 = the tile is not expressible: the kernels read its raw packed copy instead).
struct WcChunk { u4 lo0, lo1, ix; unsigned sg; };
__device__ __forceinline__ unsigned ldg4_nt(const void* p) { return __builtin_nontemporal_load((const __attribute__((address_space(1))) unsigned*)p); }
// p16 = the tile's coded base + lane * 16, p4 = + 3 KiB + lane * 4 (both advanced by q * WC_CHUNK_BYTES by the caller)
__device__ __forceinline__ WcChunk wc_load(const unsigned char* p16, const unsigned char* p4) {
    WcChunk c;
    c.lo0 = ldg16_nt(p16); c.lo1 = ldg16_nt(p16 + 1024); c.ix = ldg16_nt(p16 + 2048); c.sg = ldg4_nt(p4);
    return c;
}
// four high bytes from four index bytes (0..15 each): GI = 2 j + (weights 4..7 ? 1 : 0) selects their sign bits
// DENSE: the tile holds no index 0 (its dense word says so, wcode.py dense()): every byte is base + index <= 126, no zero test, no carry between bytes
template <int GI, bool DENSE = false> __device__ __forceinline__ unsigned wc_hi4(unsigned x, unsigned base4, unsigned sg) {
    if constexpr (DENSE) return (x + base4) | ((sg << (7 - GI)) & 0x80808080u);
    const unsigned m = (x + 0x7f7f7f7fu) & 0x80808080u;       // bit 7 of a byte: its index is not 0
    const unsigned keep = m - (m >> 7);                        // 0x7f there, 0 where the index is 0
    return ((x + base4) & keep) | ((sg << (7 - GI)) & 0x80808080u);
}
// fragment J (constant) of a chunk: the 16 bytes pack_weight_k wrote for this lane in packed chunk 4 q + J
template <int J, bool DENSE = false> __device__ __forceinline__ u4 wc_frag(const WcChunk& c, unsigned base4) {
    const unsigned n = c.ix[J];
    const u4& lo = J < 2 ? c.lo0 : c.lo1;
    const unsigned l0 = lo[2 * (J & 1)], l1 = lo[2 * (J & 1) + 1];
    const unsigned h0 = wc_hi4<2 * J, DENSE>(n & 0x0f0f0f0fu, base4, c.sg), h1 = wc_hi4<2 * J + 1, DENSE>((n >> 4) & 0x0f0f0f0fu, base4, c.sg);
    return (u4){__builtin_amdgcn_perm(h0, l0, 0x05010400u), __builtin_amdgcn_perm(h0, l0, 0x07030602u),
                __builtin_amdgcn_perm(h1, l1, 0x05010400u), __builtin_amdgcn_perm(h1, l1, 0x07030602u)};
}

// ---- int4 group-quantised weights ("W4", 4.125 bits per weight; the format's definition is radialog_amd/w4.py) ------------------------------
// A W4 chunk is the same 128 k-values of one 16-row tile, W4_CHUNK_BYTES bytes: [nibbles: 64 lanes x 16 B][scales: 16 rows x 2 B]. Dword j of lane
// (g, r)'s 16 bytes holds the 8 weights of ITS MFMA A fragment j (packed chunk 4 q + j) as nibbles q + 8, weight e in nibble 2 e (e < 4) or 2 (e - 4) + 1;
// the group's bf16 scale s is the 2 bytes at 1024 + 2 r. The decode gives exactly W' = bf16(float(q) * float(s)): fma(float(nibble), s, -8 s) is
// (nibble - 8) * s, which fp32 holds exactly (4 x 8 significant bits), then ONE round-to-nearest-even to bf16 -- the packed bf16 copy's bits.
struct W4Chunk { u4 nib; unsigned sc; };
__device__ __forceinline__ unsigned ldg2_nt(const void* p) { return __builtin_nontemporal_load((const __attribute__((address_space(1))) unsigned short*)p); }
// p16 = the tile's stream base + lane * 16, p2 = + 1 KiB + 2 r (both advanced by q * W4_CHUNK_BYTES by the caller)
__device__ __forceinline__ W4Chunk w4_load(const unsigned char* p16, const unsigned char* p2) {
    W4Chunk c;
    c.nib = ldg16_nt(p16); c.sc = ldg2_nt(p2);
    return c;
}
__device__ __forceinline__ unsigned w4_pk(float a, float b) {
    typedef __bf16 v2b __attribute__((ext_vector_type(2)));
    const v2b p = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned, p);
}
// fragment J (constant) of a chunk: the 16 bytes the packed bf16 copy of W' holds for this lane in packed chunk 4 q + J
template <int J> __device__ __forceinline__ u4 w4_frag(const W4Chunk& c) {
    const float s = __builtin_bit_cast(float, c.sc << 16), m8 = -8.f * s;
    const unsigned n = c.nib[J];
    const unsigned lo = n & 0x0f0f0f0fu, hi = (n >> 4) & 0x0f0f0f0fu;     // weights 0..3, 4..7: one per byte (v_cvt_f32_ubyte0..3)
    // Two VALU instructions per weight, written out: left to itself the compiler extracts every nibble with a shift and a mask of its own and pairs
    // the multiplies into v_pk_fma_f32 on register PAIRS -- whose second register is the pending scale load of the next chunk, so every trip of the K
    // loop waited vmcnt(0) (tests/test_isa_w4.py).
#define RDX_W4F(x, k) ({ float t_, f_; asm("v_cvt_f32_ubyte" #k " %0, %1" : "=v"(t_) : "v"(x)); asm("v_fma_f32 %0, %1, %2, %3" : "=v"(f_) : "v"(t_), "v"(s), "v"(m8)); f_; })
    const u4 f = (u4){w4_pk(RDX_W4F(lo, 0), RDX_W4F(lo, 1)), w4_pk(RDX_W4F(lo, 2), RDX_W4F(lo, 3)),
                      w4_pk(RDX_W4F(hi, 0), RDX_W4F(hi, 1)), w4_pk(RDX_W4F(hi, 2), RDX_W4F(hi, 3))};
#undef RDX_W4F
    return f;
}

// What the two alternative weight streams of the batch <= 2 GEMV differ in (skinny_body.h / chain.hip, template switch WC: 1 = the 13-bit code,
// 2 = int4): the chunk in registers, its bytes, where the lane's second pointer starts, its loads (LOADS per chunk), the decode of fragment J (hp: the
// 13-bit code's window base from the tile's header; DENSE: the tile's dense word is set, the decode without the zero test; int4 carries its scale in
// the chunk) and which four 16-byte registers of a dropped ring a raw-flagged tile reuses.
template <int WC> struct Coded;
template <> struct Coded<1> {
    typedef WcChunk Chunk;
    static constexpr int BYTES = WC_CHUNK_BYTES, LOADS = 4;
    static __device__ __forceinline__ int off2(int lane) { return 3072 + lane * 4; }
    static __device__ __forceinline__ Chunk load(const unsigned char* p16, const unsigned char* p2) { return wc_load(p16, p2); }
    template <int J, bool DENSE = false> static __device__ __forceinline__ u4 frag(const Chunk& c, unsigned hp) { return wc_frag<J, DENSE>(c, hp); }
    static __device__ __forceinline__ u4& slot(Chunk* ring, int u) { return u == 0 ? ring[0].lo0 : u == 1 ? ring[0].lo1 : u == 2 ? ring[0].ix : ring[1].lo0; }
};
template <> struct Coded<2> {
    typedef W4Chunk Chunk;
    static constexpr int BYTES = W4_CHUNK_BYTES, LOADS = 2;
    static __device__ __forceinline__ int off2(int lane) { return 1024 + (lane & 15) * 2; }
    static __device__ __forceinline__ Chunk load(const unsigned char* p16, const unsigned char* p2) { return w4_load(p16, p2); }
    template <int J, bool = false> static __device__ __forceinline__ u4 frag(const Chunk& c, unsigned) { return w4_frag<J>(c); }
    static __device__ __forceinline__ u4& slot(Chunk* ring, int u) { return ring[u].nib; }       // (rings of at least four chunks)
};
template <> struct Coded<0> : Coded<1> {};      // the raw instantiations declare an unused ring of this type

// ---- model dtype -> fp8 (OCP e4m3) activation quantisation of the fp8 path: q = RNE_e4m3(x * (448 / absmax)), scale = absmax / 448 ----------
// (the arithmetic of pack_weight_fp8_k and of the oracle's fake quantisation; an all-zero range gets scale 1)
__device__ __forceinline__ void fp8_scale(float amax, float& sc, float& inv) {
    sc = amax > 0.f ? amax / 448.0f : 1.0f;
    inv = amax > 0.f ? 448.0f / amax : 1.0f;
}
template <typename T> __device__ __forceinline__ u2 quant8(const typename Vec8<T>::type& v, float inv) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(tof<T>(v[0]) * inv, tof<T>(v[1]) * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(tof<T>(v[2]) * inv, tof<T>(v[3]) * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(tof<T>(v[4]) * inv, tof<T>(v[5]) * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(tof<T>(v[6]) * inv, tof<T>(v[7]) * inv, hi, true);
    return (u2){(unsigned)lo, (unsigned)hi};
}
template <typename T> __device__ __forceinline__ float amax8(const typename Vec8<T>::type& v) {
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(tof<T>(v[j])));
    return m;
}
// ---- wave (64 lanes) reductions ----------------------------------------------------------------------------------
// Cross-lane traffic goes through DPP / v_readlane / v_permlane*_swap (VALU speed, ~8 cycles each) rather than
// __shfl_xor (ds_bpermute: an LDS-crossbar round trip of ~100 cycles per step) -- these reductions sit on the critical
// path of latency-bound kernels (decode attention, the RMSNorm prologue of every GEMV).
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140, DPP_ROR8 = 0x128;
// sum / max over each aligned group of 16 lanes (one DPP row); every lane of the group gets the result
__device__ __forceinline__ float row16_sum(float v) {
    v += dpp_mov<DPP_XOR1>(v);
    v += dpp_mov<DPP_XOR2>(v);
    v += dpp_mov<DPP_HALF_MIRROR>(v);
    v += dpp_mov<DPP_MIRROR>(v);
    return v;
}
__device__ __forceinline__ float row16_max(float v) {
    v = fmaxf(v, dpp_mov<DPP_XOR1>(v));
    v = fmaxf(v, dpp_mov<DPP_XOR2>(v));
    v = fmaxf(v, dpp_mov<DPP_HALF_MIRROR>(v));
    v = fmaxf(v, dpp_mov<DPP_MIRROR>(v));
    return v;
}
__device__ __forceinline__ float lane_bcast(float v, int lane_const) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane_const));
}
__device__ __forceinline__ float wave_sum(float v) {
    v = row16_sum(v);
    return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
}
__device__ __forceinline__ float wave_max(float v) {
    v = row16_max(v);
    return fmaxf(fmaxf(lane_bcast(v, 0), lane_bcast(v, 16)), fmaxf(lane_bcast(v, 32), lane_bcast(v, 48)));
}
// v[l] + v[l ^ 16] and v[l] + v[l ^ 32] (gfx950 v_permlane16_swap / v_permlane32_swap: odd rows of the first operand
// are exchanged with even rows of the second, so with both operands = v the pair holds {even rows, odd rows} twice)
__device__ __forceinline__ float xor16_sum(float v) {
    const int b = __builtin_bit_cast(int, v);
    const auto r = __builtin_amdgcn_permlane16_swap(b, b, false, false);
    return __builtin_bit_cast(float, (int)r[0]) + __builtin_bit_cast(float, (int)r[1]);
}
__device__ __forceinline__ float xor32_sum(float v) {
    const int b = __builtin_bit_cast(int, v);
    const auto r = __builtin_amdgcn_permlane32_swap(b, b, false, false);
    return __builtin_bit_cast(float, (int)r[0]) + __builtin_bit_cast(float, (int)r[1]);
}

// block reductions through a small LDS scratch (>= 32 floats); all threads get the result.
__device__ __forceinline__ float block_sum(float v, float* scratch) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) scratch[w] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < nw; ++i) r += scratch[i];
    return r;
}
__device__ __forceinline__ float block_max(float v, float* scratch) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) scratch[w] = v;
    __syncthreads();
    float r = -INFINITY;
    for (int i = 0; i < nw; ++i) r = fmaxf(r, scratch[i]);
    return r;
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float silu(float x) { return x / (1.0f + expf(-x)); }

// K-cache layout inside one (row, head) slab [max_len][128]: every group of 16 positions is stored in the MFMA A-fragment
// order [dim / 32][lane (g = (dim % 32) / 8, r = pos % 16)][8], so that a wave's fragment load for the scores (16 positions x
// 32 dims) is ONE contiguous KiB instead of 16 rows x 16 bytes per quarter wave (64 tag look-ups per load instruction).
// `dim` is a multiple of 8; max_len is a multiple of 16. V stays row-major (its reads are row-contiguous).
// The order is chosen per context (LlamaDims::k_perm): contexts of up to 8 rows (the 16-wave latency attention: batch-1 attention
// 8.7 -> 7.3 us) use it, larger ones keep K row-major (the 4-wave throughput attention measured 1.5 us per launch slower with it).
__host__ __device__ __forceinline__ size_t kperm(int pos, int dim, int perm = 1) {
    return perm ? (size_t)(pos >> 4) * 2048 + (size_t)((((dim >> 5) * 64) + ((dim & 31) >> 3) * 16 + (pos & 15)) << 3)
                : (size_t)pos * 128 + dim;
}

// Where the 8 elements (e4m3 layouts: bytes) k .. k + 8 of activation row `row` live in layout L, in elements (bytes) from the buffer's start: the
// orders of ActLayout (rdx_kernels.h). k is a multiple of 8. Used by the RMSNorm kernels (elem.hip); the GEMM and attention kernels carry their own copies.
__device__ __forceinline__ size_t act_offset(ActLayout L, size_t row, int k, int mtiles, int H) {
    const int rt = (int)(row >> 4), r = (int)(row & 15);
    switch (L) {
    case ACT_BLK32: return (size_t)(((k >> 5) * 2 + rt) * 64 + ((k & 31) >> 3) * 16 + r) << 3;
    case ACT_TILES32: return (size_t)(((k >> 5) * mtiles + rt) * 64 + ((k & 31) >> 3) * 16 + r) << 3;
    case ACT_BLK64: return (size_t)(((2 * (k >> 6) + ((k & 15) >> 3)) * 2 + rt) * 64 + ((k & 63) >> 4) * 16 + r) << 3;
    case ACT_BLK64_E4M3: return (row >> 5) * (size_t)(32 * H) + ((size_t)(((k >> 6) * 2 + (rt & 1)) * 64 + ((k & 63) >> 4) * 16 + r) << 4) + (k & 8);
    default: return row * H + k;
    }
}

// packed GEMM weight geometry: [n_tile16][k_chunk32][64 lanes][8 elems]; lane = (g<<4)|r holds
// W[n_tile*16 + r][k_chunk*32 + g*8 .. +8]  -- the MFMA 16x16x32 operand fragment, 1 KiB per block.
__host__ __device__ __forceinline__ size_t packed_elems(int n, int k) { return (size_t)((n + 15) / 16) * 16 * (size_t)k; }

}  // namespace rdx

// ---- host side ---------------------------------------------------------------------------------------------------
// hipFuncSetAttribute is per DEVICE: a process may own contexts on several GPUs (one per GPU is the rule, but nothing enforces it), so the
// "set once" guards of the launchers are keyed by the current device
namespace rdx {
struct DevOnce {
    bool done[64] = {};
    bool first() { int d = 0; (void)hipGetDevice(&d); d &= 63; if (done[d]) return false; done[d] = true; return true; }
};
}  // namespace rdx

#define RDX_DISPATCH_T(dt, T, ...)                         \
    do {                                                   \
        if ((dt) == rdx::DT_F16) { typedef rdx::f16 T; __VA_ARGS__; } \
        else { typedef rdx::bf16 T; __VA_ARGS__; }         \
    } while (0)
