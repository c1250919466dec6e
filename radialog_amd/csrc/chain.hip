// Chained decode launches of the batch-1/2 step (gfx950): units of consecutive decode layers run as ROLES of one launch, the dependency
// between them is a counter hand-off (handoff.h) instead of a kernel boundary -- a consumer workgroup first puts a ring of register
// fragments of ITS weight tile in flight, then waits until the producer role has published the activations. What is in flight is all
// that HBM moves during the hand-off, so the ring is sized to the hand-off, not to the main loop (profiles/r07_chain_seam.md).
//
//   decode_chain_k   down_proj(l) (+ residual)  ->  RMSNorm + QKV(l + 1): one launch per layer, one 1024-thread workgroup per CU
//                    (two resident 16-wave workgroups per CU run every unit ~25 % slower, so the launch reserves > half of the LDS).
//                    With one workgroup per CU a QKV workgroup becomes resident when a down_proj workgroup has retired; its dispatch and
//                    first byte (~1.8 us) hide behind the wait for the LAST arrival (~3 us: poll 2 us behind the slowest down_proj tile),
//                    then the row is loaded, normalised and staged (~2 us). A ring of 8 fragments per wave (25 MB over the chip, 4 us of
//                    HBM time) left ~2 us of that with nothing in flight; the QKV role now holds 16 (half of a wave's K slice). On coded
//                    weights (decode_chain_wc_k) the ring is 4 coded chunks; the first is decoded into LDS while the wave waits, and its slot
//                    is refilled only behind the row: loads return in order, and nothing but the ring stands in front of the row;
//   attn_oproj16_k   decode attention (attn_body.h) -> o_proj (+ residual): 32 attention workgroups + 128 two-tile o_proj workgroups
//                    whose whole K slice sits in registers while attention runs. Its hand-off is DATA-TAGGED (handoff.h: WaitTagged): the
//                    attention output travels as 8-byte {two elements, tag} granules in one buffer shared by all layers, the producer neither
//                    drains nor signals, the consumer re-reads its own granules until the tags match and stages them; a hint word per head,
//                    stored when the scores are finished, opens the sweep (profiles/r08_attn_oproj_handoff.md: 13.5 -> 12.6 us per launch).
// Payloads are written write-through (8-byte agent-scope stores) and read with agent-scope loads: no cache fences. Arithmetic,
// rounding points and the fixed-order LDS reduction are those of skinny_body.h (same oracle parity).
// Liveness: a workgroup only waits on counters fed by lower-indexed workgroups; spins are bounded (handoff.h).
// Arguments: every launch is a graph node of ONE layer, so the layer's pointers travel by value (there is no device table of layers). What a role's
// first loads are addressed from are LEADING scalar kernel arguments, which kernarg preloading (build.py UNIT_FLAGS) has in SGPRs when the first wave
// starts; everything else is read behind those loads (rdx_common.h late_kernarg). No scalar load, and no wait for one, stands in front of the first
// loads of any role (tests/test_isa_entry.py holds the assembly to that).
// (Round 3: the all-roles chained kernel RDX_MEGA, the gate/up -> down -> QKV chain RDX_CHAIN=1 and the 8-wave fused attention of
// fused.hip were measured slower in rounds 1-2 and have been removed; DESIGN.md 4 keeps the measurements.)
#include "rdx_common.h"
#include "rdx_kernels.h"
#include "attn_body.h"
#include "handoff.h"
#include "skinny_body.h"   // swiglu()

namespace rdx {

constexpr int CH_WAVES = 16;
constexpr int CH_THREADS = CH_WAVES * 64;
constexpr int CH_MAXM = 2;                       // batch rows supported (LDS staging of [M][inter] activations)
// coded chunks a wave decodes ahead of its role's seam in decode_chain_wc_k, 0 = none; at most the role's ring (4 and 2). Chosen by measurement.
// CH_PRE_*: into registers (chain_tile PRE; profiles/r13_chain_predecode.md: down_proj is fastest with 2). CH_PARK_QKV: into LDS, refilled behind
// the hand-off (chain_tile PARK; 64 KiB per chunk: 16 waves x 4 fragments x 1 KiB), in front of the CH_PRE_QKV register chunks. The QKV role is
// fastest with one parked chunk and none in registers; a second chunk, parked or in registers, is slower than the one (profiles/r17_chain_park.md)
constexpr int CH_PRE_QKV = 0, CH_PRE_DOWN = 2;
constexpr int CH_PARK_QKV = 1;
constexpr size_t CH_PARK_BYTES = (size_t)CH_WAVES * 4 * 64 * 16;

// One weight-streaming unit, WITHOUT what its ring needs: the weight base (model dtype, or the e4m3 bytes of a W8 instantiation) and K reach
// chain_tile as values of their own -- leading kernel arguments, which the command processor preloads into SGPRs (rdx_kernels.h), so the ring
// is issued before the first scalar load of the rest has come back
struct ChainGemm {
    const void* X; int ldx;
    const void* resid; int ldr;
    void* out; int ldo;
    int M, N;
    const void* norm_w; float eps;
    const float* wscale;                          // fp8 weights: per-row scale, see skinny_body.h
};

// what `late()` hands chain_tile behind the ring. wraw / wchdr: a WC instantiation's raw packed weight (what a flagged tile streams) and header words
template <typename WaitFn> struct ChainLate { ChainGemm a; WaitFn wait; long long* trace; const void* wraw = nullptr; const unsigned* wchdr = nullptr; };

// Wb, K, wg, ntiles: from preloaded kernel arguments. late(): the rest (ChainLate), built from kernel arguments that are loaded only now (late_kernarg)
// WC: Wb is the coded bf16 copy of the weight (rdx_common.h WcChunk): the ring holds U / 2 coded chunks (the 2 U packed chunks of the raw ring at 13/16 of
// the bytes), decoded in registers into the fragments the raw ring holds, in the same order: the sums do not change. As skinny_body.h.
// PRE (WC = 1 only): the first PRE coded chunks of the ring are decoded, and their slots refilled, BEFORE the role's dead time ends instead of behind
// it -- PRE_POLL: in front of wait_inputs(), by every wave but the polling one (wave 0); otherwise between the issue of the activation loads and
// their staging, by every wave. Same fragments into the same MFMAs in the same order (profiles/r13_chain_predecode.md).
// PARK (WC = 1 with PRE_POLL only): the first PARK chunks of the ring are decoded ahead of the seam into a wave-private LDS region behind the zero line,
// park[wave][4 PARK][64 lanes] x 16 bytes, and NO slot is refilled there: the refills of the PARK + PRE decoded slots stand behind the first barrier of
// the norm statistics, so no weight load stands between the ring and the row. The polling wave decodes behind the wait, in front of its row loads,
// through the same code. The first trip takes the parked fragments from LDS, then the PRE register fragments, then the rest of the ring. `red` lies over the park region (a wave's slice over
// its own slots, consumed by then): the role needs 208 B + the staged rows + PARK x 64 KiB (profiles/r17_chain_park.md).
template <typename T, int EPI, bool NORM, int SUB, int XL, typename WaitFn, int U = 4, bool RESID_EARLY = false, bool W8 = false, int WC = 0, int PRE = 0,
          bool PRE_POLL = false, int PARK = 0, typename Late>
__device__ __forceinline__ ChainLate<WaitFn> chain_tile(const void* Wb, const int K, const int wg, const int ntiles, unsigned char* smem, Late late) {
    typedef typename Vec8<T>::type V8;
    constexpr int WPS = CH_WAVES / SUB;           // waves per tile
    // U chunks per register batch, two batches in flight (a ring of 2 U fragments): 32 VGPRs at U = 4, 64 at U = 8; every role stays <= 128
    constexpr int RED_LD = PARK > 0 ? 4 * PARK * 256 : 256;             // floats from one wave's `red` slice to the next (PARK: a wave's park slots)
    float* red = reinterpret_cast<float*>(smem);                        // [CH_WAVES][256] (PARK: over the park region, set behind late())
    float* ssq = red + (PARK > 0 ? 0 : CH_WAVES * 256);                 // [CH_WAVES][CH_MAXM]
    float* rstd_s = ssq + CH_WAVES * CH_MAXM;                           // [CH_MAXM] (+pad)
    T* xs = reinterpret_cast<T*>(rstd_s + 16);                          // [M][K] x-hat

    const int lane = threadIdx.x & 63, wa = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sub = wa / WPS, w = wa - sub * WPS;
    const int tile = wg * SUB + sub;
    const int tile_c = min(tile, ntiles - 1);     // ragged last workgroup: duplicate loads, masked stores
    const int r = lane & 15, g = lane >> 4;
    const int KC = W8 ? (K >> 6) : (K >> 5);                            // W8: a chunk is 64 k-values (16 fp8 bytes per lane, two MFMAs)
    const int c0 = (KC * w) / WPS, c1 = (KC * (w + 1)) / WPS;
    const u4* wbase = reinterpret_cast<const u4*>(Wb) + (size_t)tile_c * KC * 64 + lane;
    const int clast = min(max(c1 - 1, c0), KC - 1);
    // WC: the slice stays [c0, c1) in PACKED chunks; the coded chunks [q0, q1) cover it, the first and the last may reach into the neighbours' (down_proj:
    // 344 chunks over 16 waves), whose fragments multiply the zero line behind the staged rows
    static_assert(!WC || (!W8 && U % 2 == 0), "coded weights: model dtype");
    typedef Coded<WC> CD;         // WC = 2: the int4 stream (rdx_common.h W4Chunk), rings of four chunks (8 loads) in both roles
    constexpr int RC = WC == 2 ? 4 : U / 2;
    const int KQ = K >> 7, q0 = c0 >> 2, q1 = c1 > c0 ? (c1 + 3) >> 2 : q0, qlast = min(max(q1 - 1, q0), KQ - 1);
    const unsigned char* cb16 = reinterpret_cast<const unsigned char*>(Wb) + (size_t)tile_c * KQ * CD::BYTES + lane * 16;
    const unsigned char* cb4 = reinterpret_cast<const unsigned char*>(Wb) + (size_t)tile_c * KQ * CD::BYTES + CD::off2(lane);
    // Everything up to here comes from preloaded kernel arguments, the workgroup id and the lane id: the ring below is issued with no scalar load
    // in front of it. The entry time is taken unconditionally (one scalar instruction, nothing waits for it before the ring is out) because the
    // trace pointer is one of the arguments that are only loaded behind the ring.
    const long long t_entry = (long long)__builtin_amdgcn_s_memrealtime();

    // two register batches (A, B) in flight before anything else; the main loop ping-pongs between them (no register
    // rotation: a rotated pair makes the compiler wait for the batch it has just issued)
    u4 wa_[U], wb_[U];
    typename CD::Chunk cring[RC];
    if constexpr (WC) {
#pragma unroll
        for (int u = 0; u < RC; ++u) { const size_t o = (size_t)min(q0 + u, qlast) * CD::BYTES; cring[u] = CD::load(cb16 + o, cb4 + o); }
    } else {
#pragma unroll
        for (int u = 0; u < U; ++u) wa_[u] = ldg16_nt(wbase + (size_t)min(c0 + u, clast) * 64);
#pragma unroll
        for (int u = 0; u < U; ++u) wb_[u] = ldg16_nt(wbase + (size_t)min(c0 + U + u, clast) * 64);
    }
    __builtin_amdgcn_sched_barrier(0);            // nothing of what follows is scheduled in front of the ring
    const ChainLate<WaitFn> lt = late();
    const ChainGemm& a = lt.a;
    const WaitFn& wait_inputs = lt.wait;
    long long* const trace = lt.trace;
    unsigned wc_hdr = 0;          // the tile's header word: a scalar load (constant address space) behind the ring, see skinny_body.h
    if constexpr (WC) wc_hdr = *(reinterpret_cast<const __attribute__((address_space(4))) unsigned*>((uintptr_t)lt.wchdr) + tile_c);
    // the 13-bit code's dense word, behind the header words (gemm.hip encode_wc_k): the tile holds no index 0 and is decoded without the zero test
    // (rdx_common.h wc_hi4 DENSE). Raw, general or dense: one scalar choice per tile, in the pre-decode and in front of the K loops.
    // The two coded forms stand one BEHIND the other, each stepped over by scalar branches where the tile takes the other (skinny_body.h: as the two
    // arms of one branch this kernel went from 96 VGPRs to 128 and 104 bytes of scratch). form_d / form_g: which one runs, opaque to the compiler --
    // what it can prove about them it uses to put the forms side by side again.
    unsigned wc_dense = 0;
    if constexpr (WC == 1) wc_dense = *(reinterpret_cast<const __attribute__((address_space(4))) unsigned*>((uintptr_t)lt.wchdr) + ntiles + tile_c);
    // (bit 0 of the word: exactly one of the two is set, whatever else the word may come to hold)
    auto form_d = [&]() -> bool { unsigned f = wc_dense & 1u; asm volatile("" : "+s"(f)); return f != 0; };
    auto form_g = [&]() -> bool { unsigned f = (wc_dense & 1u) ^ 1u; asm volatile("" : "+s"(f)); return f != 0; };
    // debug timeline of this workgroup (rdx_gemv_trace 7; null in every product launch), 100 MHz ticks, wave 0: [0] entry, [5] first weight KiB
    // back, [3] inputs ready, [6] first MFMA (row staged), [1] K loop done, [7] end; [2] = arrival, written by the down_proj role's caller
    const T* X = reinterpret_cast<const T*>(a.X);
    long long* trc = (trace && threadIdx.x == 0) ? trace : nullptr;
#define CH_T(i) do { if (trc) trc[i] = (long long)__builtin_amdgcn_s_memrealtime(); } while (0)
    if (trc) trc[0] = t_entry;
    if (trace) {        // traced launches only: wave 0 watches its first KiB come back (it stalls here, which a product launch never does)
        if (threadIdx.x < 64) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(WC ? CD::LOADS * RC - 1 : 2 * U - 1) : "memory");
        CH_T(5);
    }

    // RESID_EARLY: the residual predates the launch (fused attention + o_proj) -> fetch it now, off the critical tail
    constexpr int QPT_E = EPI == EPI_SILU_MUL ? 2 : 4;
    unsigned long long rs8_early = 0ull;
    if (RESID_EARLY && EPI == EPI_RESID && (int)threadIdx.x < SUB * a.M * QPT_E) {
        const int so = threadIdx.x / (a.M * QPT_E), rem = threadIdx.x - so * (a.M * QPT_E);
        const int m = rem / QPT_E, q = rem - m * QPT_E;
        const int n = (wg * SUB + so) * 16 + q * 4;
        if (wg * SUB + so < ntiles && n < a.N) rs8_early = ld8_agent(reinterpret_cast<const T*>(a.resid) + (size_t)m * a.ldr + n);
    }

    // Pre-decode (PRE): a wave of an unflagged tile turns the first PRE chunks of its ring into their 4 PRE MFMA fragments and refills those slots at
    // once with the chunks the first trip of the K loop would fetch into them (q0 + RC + u, clamped as every ring load is). Where it stands the wave
    // has nothing else to do: 15 of 16 waves sit at the barrier of the hand-off wait, and what they decode here they do not decode behind the seam, four
    // to a SIMD; the refills are in flight that much earlier. No barrier and no wait on another workgroup in here. Wave 0 polls (PRE_POLL): loads
    // return in order, so its first poll must not stand behind a refill -- it decodes nothing here and runs the same code once the row is staged, in
    // front of its first MFMA (one path behind the seam for all waves; a wave-0 path of its own cost 20 bytes of scratch).
    static_assert(PRE == 0 || (WC == 1 && PARK + PRE <= RC), "pre-decode: coded bf16 weights, at most the ring");
    static_assert(PARK == 0 || (WC == 1 && PRE_POLL && !WaitFn::TAGGED && NORM), "parked pre-decode: the polling role of the coded launch");
    static_assert(PRE == 0 || PRE_POLL || !WaitFn::TAGGED, "pre-decode without a poll stands behind the plain activation loads: a tagged sweep has no such site");
    u4 pre[PRE ? 4 * PRE : 1];
    const bool predec = PRE > 0 && !(wc_hdr & 0x100u);        // wave-uniform
    auto predecode_as = [&](auto dn) {         // dn: the tile is dense (std::true_type) or general
        if constexpr (PRE > 0) {
            constexpr bool DN = decltype(dn)::value;
            const unsigned base4 = (wc_hdr & 0xffu) * 0x01010101u;
#pragma unroll
            for (int u = 0; u < PRE; ++u) {
                pre[4 * u] = CD::template frag<0, DN>(cring[u], base4); pre[4 * u + 1] = CD::template frag<1, DN>(cring[u], base4);
                pre[4 * u + 2] = CD::template frag<2, DN>(cring[u], base4); pre[4 * u + 3] = CD::template frag<3, DN>(cring[u], base4);
                const size_t o = (size_t)min(q0 + RC + u, qlast) * CD::BYTES;
                cring[u] = CD::load(cb16 + o, cb4 + o);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    auto predecode = [&] {
        if (predec) {
            if (form_d()) predecode_as(std::true_type());
            if (form_g()) predecode_as(std::false_type());
        }
    };
    // PARK: decode only, chunks 0 .. PARK - 1 into the wave's park slots (one 16-byte LDS store per fragment, lane-contiguous), PARK .. PARK + PRE - 1
    // into `pre`; the chunks of the first trip go into all of these slots behind the row (below, in the norm statistics)
    u4* const parkw = reinterpret_cast<u4*>(xs + (size_t)a.M * K + 8) + wa * (4 * (PARK > 0 ? PARK : 1) * 64) + lane;
    if constexpr (PARK > 0) red = reinterpret_cast<float*>(xs + (size_t)a.M * K + 8);
    auto ahead_as = [&](auto dn) {
        if constexpr (PARK > 0) {
            constexpr bool DN = decltype(dn)::value;
            const unsigned base4 = (wc_hdr & 0xffu) * 0x01010101u;
#pragma unroll
            for (int u = 0; u < PARK + PRE; ++u)      // opaque: the decode below stands in the two-pass loop and is not hoisted out of it (for all waves, both forms)
                asm volatile("" : "+v"(cring[u].lo0), "+v"(cring[u].lo1), "+v"(cring[u].ix), "+v"(cring[u].sg));
#pragma unroll
            for (int u = 0; u < PARK; ++u) {
                parkw[(4 * u) * 64] = CD::template frag<0, DN>(cring[u], base4); parkw[(4 * u + 1) * 64] = CD::template frag<1, DN>(cring[u], base4);
                parkw[(4 * u + 2) * 64] = CD::template frag<2, DN>(cring[u], base4); parkw[(4 * u + 3) * 64] = CD::template frag<3, DN>(cring[u], base4);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int u = 0; u < PRE; ++u) {
                pre[4 * u] = CD::template frag<0, DN>(cring[PARK + u], base4); pre[4 * u + 1] = CD::template frag<1, DN>(cring[PARK + u], base4);
                pre[4 * u + 2] = CD::template frag<2, DN>(cring[PARK + u], base4); pre[4 * u + 3] = CD::template frag<3, DN>(cring[PARK + u], base4);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    auto ahead = [&] {
        if (!(wc_hdr & 0x100u)) {             // wave-uniform; a flagged raw tile parks nothing
            if (form_d()) ahead_as(std::true_type());
            if (form_g()) ahead_as(std::false_type());
        }
    };
    // activations: published write-through by other workgroups of this launch -> agent-scope 8-byte loads (L1 bypass),
    // each chunk loaded ONCE and kept in registers across the RMSNorm statistics
    // XL = chunks of 4 elements per thread: M*K/4 <= XL*1024 (checked by chain_supported)
    const int K4 = K >> 2, total4 = a.M * K4;
    unsigned long long xr[XL];
    unsigned long long nwr[PARK > 0 ? XL : 1];       // PARK: the norm weights, loaded next to the row
    if constexpr (PARK > 0) {
        // ahead() stands ONCE in the kernel's text, in a loop of two passes: fifteen waves run it in pass 0, in front of the hand-off wait, the polling
        // wave in pass 1, behind it and in front of its row loads: one path for all waves, no twin. (A second inlined copy for the polling wave,
        // under the flight of its row, is code that one wave runs once per workgroup with the other fifteen waiting at the barrier of the norm
        // statistics; measured 1.4 ms per report behind this form, profiles/r17_chain_park.md forms 3 and 4.) No load
        // stands in the loop: a loaded value carried round it is copied in the loop's header behind vmcnt(0), in front of the first poll. `pass`
        // is opaque so that the loop is neither unrolled nor peeled.
        unsigned pass = 0;
#pragma nounroll
        for (;;) {
            asm volatile("" : "+s"(pass));
            if ((pass == 0) == (wa != 0)) ahead();
            if (pass) break;
            wait_inputs();
            CH_T(3);
            pass = 1;
        }
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int c = threadIdx.x + i * CH_THREADS;
            xr[i] = 0ull; nwr[i] = 0ull;
            if (c < total4) {
                const int m = c / K4, k4 = c - m * K4;
                xr[i] = ld8_agent(X + (size_t)m * a.ldx + (size_t)k4 * 4);
                // the norm weights predate the launch: loaded here, behind the row, they are back with it; where the staging loads them without
                // PARK they would return behind the refills (loads return in order)
                nwr[i] = *reinterpret_cast<const unsigned long long*>(reinterpret_cast<const T*>(a.norm_w) + (size_t)k4 * 4);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    } else {
    if constexpr (PRE > 0 && PRE_POLL) {
        if (wa != 0) predecode();
    }

    wait_inputs();
    if (!WaitFn::TAGGED) CH_T(3);

    if constexpr (WaitFn::TAGGED) {              // tagged granules (handoff.h): the loads are the wait; same chunks in the same registers
        wait_inputs.template sweep<XL>(xr, a.X, a.ldx, K4, total4, CH_THREADS);
        if (trace) __syncthreads();              // traced launches only: "inputs ready" = EVERY wave has its granules (a product launch meets at the staging barrier below)
        CH_T(3);
    } else {
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int c = threadIdx.x + i * CH_THREADS;
            xr[i] = 0ull;
            if (c < total4) { const int m = c / K4, k4 = c - m * K4; xr[i] = ld8_agent(X + (size_t)m * a.ldx + (size_t)k4 * 4); }
        }
        if constexpr (PRE > 0 && !PRE_POLL) {     // a role whose input predates the launch: under the flight of the loads just issued (the ring is older)
            __builtin_amdgcn_sched_barrier(0);
            predecode();
        }
    }
    }
    if (NORM) {
        float ss[CH_MAXM];
#pragma unroll
        for (int m = 0; m < CH_MAXM; ++m) ss[m] = 0.f;
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int c = threadIdx.x + i * CH_THREADS;
            float t = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float f = tof<T>(from_bits16<T>((unsigned short)(xr[i] >> (16 * j)))); t += f * f; }
            const int m = c < total4 ? c / K4 : 0;                       // padding chunks are zero
#pragma unroll
            for (int mm = 0; mm < CH_MAXM; ++mm) ss[mm] += (m == mm) ? t : 0.f;
        }
#pragma unroll
        for (int m = 0; m < CH_MAXM; ++m) {
            const float t = wave_sum(ss[m]);
            if (lane == 0) ssq[wa * CH_MAXM + m] = t;
        }
        __syncthreads();
        if constexpr (PARK > 0) {
            // The refills of the decoded slots, behind the barrier that every wave reaches with its row in registers: right behind a wave's own row
            // loads they stand in front of the rows of the workgroup's later waves ("inputs ready -> first MFMA" 2.5 us there, 2.1 here at depth 1;
            // profiles/r17_chain_park.md forms 2 and 3). UNCONDITIONAL, a flagged raw tile included (it drops the ring, as it drops the ring
            // of the entry): behind a conditional load every later wait is vmcnt(0).
#pragma unroll
            for (int u = 0; u < PARK + PRE; ++u) { const size_t o = (size_t)min(q0 + RC + u, qlast) * CD::BYTES; cring[u] = CD::load(cb16 + o, cb4 + o); }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (threadIdx.x < CH_MAXM) {
            float t = 0.f;
#pragma unroll
            for (int i = 0; i < CH_WAVES; ++i) t += ssq[i * CH_MAXM + threadIdx.x];
            rstd_s[threadIdx.x] = rsqrtf(t / (float)K + a.eps);
        }
        __syncthreads();
    }
    {
        const T* NW = reinterpret_cast<const T*>(a.norm_w);
#pragma unroll
        for (int i = 0; i < XL; ++i) {
            const int c = threadIdx.x + i * CH_THREADS;
            if (c < total4) {
                const int m = c / K4, k4 = c - m * K4;
                unsigned long long v = xr[i];
                if (NORM) {
                    const float rs = rstd_s[m];
                    unsigned long long nw;
                    if constexpr (PARK > 0) nw = nwr[i];
                    else nw = *reinterpret_cast<const unsigned long long*>(NW + (size_t)k4 * 4);
                    v = 0ull;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float h = rnd<T>(tof<T>(from_bits16<T>((unsigned short)(xr[i] >> (16 * j)))) * rs);   // (x * rsqrt(var+eps)).to(dtype)
                        const float wv_ = tof<T>(from_bits16<T>((unsigned short)(nw >> (16 * j))));
                        v |= (unsigned long long)bits16<T>(fromf<T>(wv_ * h)) << (16 * j);                         // weight * hidden
                    }
                }
                *reinterpret_cast<unsigned long long*>(xs + (size_t)m * K + (size_t)k4 * 4) = v;
            }
        }
        if (WC && threadIdx.x == 0) *reinterpret_cast<u4*>(xs + (size_t)a.M * K) = (u4){0u, 0u, 0u, 0u};     // the zero line (launchers reserve it)
        __syncthreads();
    }

    // MFMA columns m >= M read row 0 again (an LDS broadcast) instead of zeros: their results are never stored, and a per-lane select around the
    // LDS read put an EXEC-masked branch inside the main loop -- the loop fell apart into basic blocks, the refill of a batch was issued before
    // the batch's last MFMA into a spare register, and the copy back waited vmcnt(0) on every trip
    const T* xrow = xs + (size_t)(r < a.M ? r : 0) * K + g * (W8 ? 16 : 8);
    v4f acc = (v4f){0.f, 0.f, 0.f, 0.f};
    CH_T(6);
    // Main loop: loads are UNCONDITIONAL (addresses clamped into the slice) and no MFMA is guarded, so the compiler can
    // wait with counted vmcnt (one batch stays in flight); a conditional load anywhere in the loop makes it fall back
    // to vmcnt(0). At most one batch per wave is fetched in vain (same 1 KiB line as the slice's last chunk).
    auto consume = [&](const u4 (&wreg)[U], int cb, bool guard) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!guard || cb + u < c1) {
                if (W8) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const u4 wd = dequant8<T>(h ? wreg[u].z : wreg[u].x, h ? wreg[u].w : wreg[u].y);
                        const u4 xv = *reinterpret_cast<const u4*>(xrow + (size_t)(cb + u) * 64 + h * 8);
                        acc = mfma16(as_vec8<T>(wd), as_vec8<T>(xv), acc);
                    }
                } else {
                    const u4 xv = *reinterpret_cast<const u4*>(xrow + (size_t)(cb + u) * 32);
                    acc = mfma16(as_vec8<T>(wreg[u]), as_vec8<T>(xv), acc);
                }
            }
        }
    };
    // Main loop: a ring of 2 U fragments, every fragment refilled right after the MFMA that consumed it, the pair pinned by a scheduling barrier
    // (the xstat32_k idiom): the waits are vmcnt(2 U - 1) and 2 U - 1 loads per wave stay in flight. As two batches ("consume U, refill U") the
    // compiler issued the refills early into spare registers and copied them back at the loop end behind vmcnt(1..7) / vmcnt(0): one load in
    // flight per wave at the end of every trip.
    auto consume1 = [&](const u4& wv, int c) {
        if (W8) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const u4 wd = dequant8<T>(h ? wv.z : wv.x, h ? wv.w : wv.y);
                const u4 xv = *reinterpret_cast<const u4*>(xrow + (size_t)c * 64 + h * 8);
                acc = mfma16(as_vec8<T>(wd), as_vec8<T>(xv), acc);
            }
        } else {
            const u4 xv = *reinterpret_cast<const u4*>(xrow + (size_t)c * 32);
            acc = mfma16(as_vec8<T>(wv), as_vec8<T>(xv), acc);
        }
    };
    if constexpr (WC) {
        if (wc_hdr & 0x100u) {
            // a tile the code cannot express (wave-uniform, once per tile): the coded ring is dropped and the raw loop runs on the packed copy, in four
            // of the ring's registers (a rare path; registers of its own would be carried through it)
            const u4* wraw = reinterpret_cast<const u4*>(lt.wraw) + (size_t)tile_c * KC * 64 + lane;
            auto slot = [&](int u) -> u4& { return CD::slot(cring, u); };
#pragma unroll
            for (int u = 0; u < 4; ++u) slot(u) = ldg16_nt(wraw + (size_t)min(c0 + u, clast) * 64);
            int cb = c0;
            for (; cb + 4 < c1; cb += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    consume1(slot(u), cb + u);
                    slot(u) = ldg16_nt(wraw + (size_t)min(cb + 4 + u, clast) * 64);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (cb + u < c1) consume1(slot(u), cb + u);
        } else {
            const unsigned base4 = (wc_hdr & 0xffu) * 0x01010101u;
            const T* zptr = xs + (size_t)a.M * K;
            // guard (first trip and tail only): fragments outside [c0, c1) read the zero line. Exact because (1) every weight of an unflagged tile is
            // finite, so the products are zeros; (2) the fp32 accumulator starts at +0 and a sum is -0 only if all its terms are, so it is never -0 and
            // x + (+-0) = x leaves its bits alone; (3) an MFMA whose 32 products are all zero returns its accumulator operand.
            auto xsel = [&](int c, bool guard) -> const u4* { return reinterpret_cast<const u4*>((!guard || (c >= c0 && c < c1)) ? xrow + (size_t)c * 32 : zptr); };
            // dn (a type: std::true_type / false_type): the dense form of the decode
            auto consumeC = [&](auto dn, const typename CD::Chunk& ch, int q, bool guard) {
                constexpr bool DN = decltype(dn)::value;
                if constexpr (WC == 1) {
                    // operand lookahead: the four activation fragments of the chunk do not depend on its decode, so they are read from LDS in front of
                    // it (16 VGPRs) and the LDS round trip passes under the decodes -- the waits are lgkmcnt(3..0) across the chunk instead of a
                    // drain in front of every MFMA. (Not the int4 stream: there the same lookahead makes the K loops wait vmcnt(0).)
                    const u4 x0 = *xsel(4 * q, guard), x1 = *xsel(4 * q + 1, guard), x2 = *xsel(4 * q + 2, guard), x3 = *xsel(4 * q + 3, guard);
                    auto one = [&](const u4 wd, const u4& xv) {
                        acc = mfma16(as_vec8<T>(wd), as_vec8<T>(xv), acc);
                        __builtin_amdgcn_sched_barrier(0);      // one fragment at a time (below)
                    };
                    one(CD::template frag<0, DN>(ch, base4), x0); one(CD::template frag<1, DN>(ch, base4), x1);
                    one(CD::template frag<2, DN>(ch, base4), x2); one(CD::template frag<3, DN>(ch, base4), x3);
                } else {
                    auto one = [&](const u4 wd, int c) {
                        acc = mfma16(as_vec8<T>(wd), as_vec8<T>(*xsel(c, guard)), acc);
                        // one fragment at a time. Without this barrier the compiler interleaves the four decodes of a chunk with the refill and waits
                        // vmcnt(0) once per trip: the ring drains (tests/test_isa_wcode.py)
                        __builtin_amdgcn_sched_barrier(0);
                    };
                    one(CD::template frag<0, DN>(ch, base4), 4 * q); one(CD::template frag<1, DN>(ch, base4), 4 * q + 1);
                    one(CD::template frag<2, DN>(ch, base4), 4 * q + 2); one(CD::template frag<3, DN>(ch, base4), 4 * q + 3);
                }
            };
            auto trip = [&](auto dn, int q, bool guard) {
#pragma unroll
                for (int u = 0; u < RC; ++u) {
                    consumeC(dn, cring[u], q + u, guard);
                    const size_t o = (size_t)min(q + RC + u, qlast) * CD::BYTES;
                    cring[u] = CD::load(cb16 + o, cb4 + o);
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            if constexpr (PARK > 0) {
                // The first trip, unconditional as below: chunks q0 .. q0 + PARK - 1 are in the wave's park slots and take an LDS read and an MFMA each
#pragma unroll
                for (int u = 0; u < PARK; ++u) {
                    const u4 x0 = *xsel(4 * (q0 + u), true), x1 = *xsel(4 * (q0 + u) + 1, true), x2 = *xsel(4 * (q0 + u) + 2, true), x3 = *xsel(4 * (q0 + u) + 3, true);
                    const u4 w0 = parkw[(4 * u) * 64], w1 = parkw[(4 * u + 1) * 64], w2 = parkw[(4 * u + 2) * 64], w3 = parkw[(4 * u + 3) * 64];
                    acc = mfma16(as_vec8<T>(w0), as_vec8<T>(x0), acc); acc = mfma16(as_vec8<T>(w1), as_vec8<T>(x1), acc);
                    acc = mfma16(as_vec8<T>(w2), as_vec8<T>(x2), acc); acc = mfma16(as_vec8<T>(w3), as_vec8<T>(x3), acc);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if constexpr (PRE > 0) {
                // The first trip, unconditional (a slice of at most RC chunks refills from its clamped last chunk, and the guard sends what lies past
                // c1 to the zero line): chunks q0 .. q0 + PRE - 1 are in `pre`, decoded and their slots refilled ahead of the seam -- by the polling
                // wave only now -- and take MFMAs only, same guard; the rest of the ring follows as in any trip, in the tile's form. The ring is then
                // that of a first trip taken: nothing is fetched twice that the loop without pre-decode fetches once. The MFMAs on `pre` stand in
                // front of both forms: its 16 PRE registers are dead where the forms' loops begin.
                if constexpr (PRE_POLL && PARK == 0) {
                    if (wa == 0) predecode();
                }
#pragma unroll
                for (int u = 0; u < 4 * PRE; ++u) {
                    acc = mfma16(as_vec8<T>(pre[u]), as_vec8<T>(*xsel(4 * (q0 + PARK) + u, true)), acc);
                    if (u % 4 == 3) __builtin_amdgcn_sched_barrier(0);      // a chunk's four operand reads at a time (16 VGPRs)
                }
            }
            if constexpr (WC == 1) {
                // First trip, K loop and tail exist once per form. The two forms stand one BEHIND the other, each stepped over as a whole where the
                // tile takes the other.
                auto coded_loop = [&](auto dn) {
                    int q = q0;
                    if constexpr (PARK + PRE > 0) {
                        // the rest of the first trip (above): the ring's chunks PARK + PRE .. RC - 1 as in any trip, guarded
#pragma unroll
                        for (int u = PARK + PRE; u < RC; ++u) {
                            consumeC(dn, cring[u], q0 + u, true);
                            const size_t o = (size_t)min(q0 + RC + u, qlast) * CD::BYTES;
                            cring[u] = CD::load(cb16 + o, cb4 + o);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                        q += RC;
                    } else if (q + RC < q1) { trip(dn, q, true); q += RC; }
                    for (; q + RC < q1; q += RC) trip(dn, q, false);
#pragma unroll
                    for (int u = 0; u < RC; ++u)
                        if (q + u < q1) consumeC(dn, cring[u], q + u, true);
                };
                if (form_d()) coded_loop(std::true_type());
                if (form_g()) coded_loop(std::false_type());
            } else {        // the int4 stream: one form, no pre-decode. The driver is written out, not a call of a lambda like coded_loop: only so does
                            // decode_chain_w4_k compile to the instructions it had (tests/test_isa_chain_predecode.py pins its loops)
                const std::false_type dn;
                int q = q0;
                if (q + RC < q1) { trip(dn, q, true); q += RC; }
                for (; q + RC < q1; q += RC) trip(dn, q, false);
#pragma unroll
                for (int u = 0; u < RC; ++u)
                    if (q + u < q1) consumeC(dn, cring[u], q + u, true);
            }
        }
    } else {
        int cb = c0;
        for (; cb + 2 * U < c1; cb += 2 * U) {
    #pragma unroll
            for (int u = 0; u < 2 * U; ++u) {
                u4& wr = u < U ? wa_[u] : wb_[u - U];
                consume1(wr, cb + u);
                wr = ldg16_nt(wbase + (size_t)min(cb + 2 * U + u, clast) * 64);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        consume(wa_, cb, true);
        consume(wb_, cb + U, true);
    }
    CH_T(1);
    // D[n_local = g*4+reg][m_local = r] -> red[wave][m_local*16 + n_local]
    *reinterpret_cast<float4*>(&red[wa * RED_LD + r * 16 + g * 4]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    __syncthreads();

    // epilogue: one thread per 4 consecutive output columns (one write-through 8-byte store each)
    T* out = reinterpret_cast<T*>(a.out);
    constexpr int QPT = EPI == EPI_SILU_MUL ? 2 : 4;                     // 4-column groups per tile row that are stored
    const int items = SUB * a.M * QPT;
    if ((int)threadIdx.x < items) {
        const int so = threadIdx.x / (a.M * QPT), rem = threadIdx.x - so * (a.M * QPT);
        const int m = rem / QPT, q = rem - m * QPT;
        const int t_o = wg * SUB + so;
        const int n = t_o * 16 + q * 4;
        const bool ok = (t_o < ntiles) && (n < a.N);                     // N % 4 == 0: a group is all-in or all-out
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = 0.f;
#pragma unroll
            for (int i = 0; i < WPS; ++i) v[j] += red[(so * WPS + i) * RED_LD + m * 16 + q * 4 + j];
            if (W8) v[j] *= a.wscale[t_o * 16 + q * 4 + j];
        }
        unsigned long long pk = 0ull;
        if (EPI == EPI_NONE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) pk |= (unsigned long long)bits16<T>(fromf<T>(v[j])) << (16 * j);
            if (ok) st8_agent(out + (size_t)m * a.ldo + n, pk);
        } else if (EPI == EPI_RESID) {
            if (ok) {
                const unsigned long long rs8 = RESID_EARLY ? rs8_early : ld8_agent(reinterpret_cast<const T*>(a.resid) + (size_t)m * a.ldr + n);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float rsd = tof<T>(from_bits16<T>((unsigned short)(rs8 >> (16 * j))));
                    pk |= (unsigned long long)bits16<T>(fromf<T>(rsd + rnd<T>(v[j]))) << (16 * j);
                }
                st8_agent(out + (size_t)m * a.ldo + n, pk);
            }
        } else if (EPI == EPI_SILU_MUL) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float u = 0.f;
#pragma unroll
                for (int i = 0; i < WPS; ++i) u += red[(so * WPS + i) * RED_LD + m * 16 + 8 + q * 4 + j];
                if (W8) u *= a.wscale[t_o * 16 + 8 + q * 4 + j];
                pk |= (unsigned long long)bits16<T>(fromf<T>(swiglu<T>(v[j], u))) << (16 * j);
            }
            if (ok) st8_agent(out + (size_t)m * a.ldo + t_o * 8 + q * 4, pk);
        }
    }
    CH_T(7);
#undef CH_T
    return lt;          // what the caller still needs of the late arguments (the down_proj role: its counters and its trace record)
}

// down_proj(l) then RMSNorm + QKV(l + 1): blocks [0, nwg_down) are down_proj tiles (one tile per workgroup, 16 waves split K; their
// input predates the launch), blocks [nwg_down, +nwg_qkv) are QKV workgroups of the NEXT layer (4 tiles each, 4 waves per tile, the
// normalised row staged once per workgroup) that wait for all down_proj tiles on the layer's sharded counter. The QKV role's ring is 16
// fragments deep (U = 8; fp8 weights keep 8: 16 measured slower there): it is issued at entry and is what HBM carries while the
// workgroup waits for the last arrival and stages the row. Same chunks in the same order per wave: the sums do not change by a bit.
// Leading arguments (preloaded into SGPRs, rdx_kernels.h): the two weight bases -- down_proj of `layer`, QKV of `layer + 1`; the e4m3 bytes in the W8
// instantiation -- and the four ints the roles' tile and K-slice arithmetic needs. The rest of the two layers travels by value in ChainArgs, read late.
template <typename T, bool W8>
__global__ __launch_bounds__(CH_THREADS, 4) void decode_chain_k(const void* wdown, const void* wqkv, int hidden, int inter, int qkv_n, int nwg_down, ChainArgs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char msm[];
    const int H = hidden;
    auto args = [] { return late_kernarg<ChainArgs>(kernarg_offset<6>(decltype(&decode_chain_k<T, W8>){})); };      // argument 6: the ChainArgs
    if ((int)blockIdx.x < nwg_down) {
        const ChainLate<WaitSharded> lt = chain_tile<T, EPI_RESID, false, 1, 6, WaitSharded, 4, false, W8>(wdown, inter, blockIdx.x, nwg_down, msm, [&] {
            const ChainArgs ca = args();
            int* ctr = ca.ctr + (size_t)ca.layer * HO_CTR_INTS;
            return ChainLate<WaitSharded>{ChainGemm{ca.dgu, inter, ca.dx, H, ca.dx, H, ca.B, H, nullptr, 0.f, ca.sdown},
                                          WaitSharded{ctr, 0, ca.err, ca.naps, nullptr}, ca.trace ? ca.trace + (size_t)blockIdx.x * 8 : nullptr};
        });
        publish_sc1(lt.wait.ctr, blockIdx.x);
        if (lt.trace && threadIdx.x == 0) lt.trace[2] = (long long)__builtin_amdgcn_s_memrealtime();      // arrival
        return;
    }
    chain_tile<T, EPI_NONE, true, 4, 2, WaitSharded, W8 ? 4 : 8, false, W8>(wqkv, H, blockIdx.x - nwg_down, (qkv_n + 15) / 16, msm, [&] {
        const ChainArgs ca = args();
        int* ctr = ca.ctr + (size_t)ca.layer * HO_CTR_INTS;
        return ChainLate<WaitSharded>{ChainGemm{ca.dx, H, nullptr, 0, ca.dqkv, ca.qkv_ld, ca.B, qkv_n, ca.attn_norm, ca.eps, ca.sqkv},
                                      WaitSharded{ctr, nwg_down, ca.err, ca.naps, nullptr}, ca.trace ? ca.trace + (size_t)blockIdx.x * 8 : nullptr};
    });
}

// The same launch on coded bf16 weights (chain_tile WC; a kernel name of its own): the leading weight arguments are the coded planes of down_proj(layer)
// and QKV(layer + 1); the raw packed copies (what a flagged tile streams) and the header words travel in ChainArgs and are read behind the rings. The
// QKV role's ring is four coded chunks (the raw role's sixteen fragments), down_proj's two. decode_chain_w4_k is the same launch on the int4 streams
// (WC = 2; ChainArgs::wdown / wqkv are then the packed bf16 copies of the dequantised weights, which the LoRA-A tiles of the QKV role stream).
typedef void (*ChainCodedFn)(const void*, const void*, int, int, int, int, ChainArgs);       // the signature of both kernels
template <int WC>
__device__ __forceinline__ void chain_coded(const void* cdown, const void* cqkv, int hidden, int inter, int qkv_n, int nwg_down, unsigned char* msm) {
    typedef bf16 T;
    const int H = hidden;
    auto args = [] { return late_kernarg<ChainArgs>(kernarg_offset<6>(ChainCodedFn{})); };      // argument 6: the ChainArgs
    if ((int)blockIdx.x < nwg_down) {
        const ChainLate<WaitSharded> lt = chain_tile<T, EPI_RESID, false, 1, 6, WaitSharded, 4, false, false, WC, WC == 1 ? CH_PRE_DOWN : 0, false>(cdown, inter, blockIdx.x, nwg_down, msm, [&] {
            const ChainArgs ca = args();
            int* ctr = ca.ctr + (size_t)ca.layer * HO_CTR_INTS;
            return ChainLate<WaitSharded>{ChainGemm{ca.dgu, inter, ca.dx, H, ca.dx, H, ca.B, H, nullptr, 0.f, nullptr},
                                          WaitSharded{ctr, 0, ca.err, ca.naps, nullptr}, ca.trace ? ca.trace + (size_t)blockIdx.x * 8 : nullptr, ca.wdown, ca.hdown};
        });
        publish_sc1(lt.wait.ctr, blockIdx.x);
        if (lt.trace && threadIdx.x == 0) lt.trace[2] = (long long)__builtin_amdgcn_s_memrealtime();      // arrival
        return;
    }
    chain_tile<T, EPI_NONE, true, 4, 2, WaitSharded, 8, false, false, WC, WC == 1 ? CH_PRE_QKV : 0, true, WC == 1 ? CH_PARK_QKV : 0>(cqkv, H, blockIdx.x - nwg_down, (qkv_n + 15) / 16, msm, [&] {
        const ChainArgs ca = args();
        int* ctr = ca.ctr + (size_t)ca.layer * HO_CTR_INTS;
        return ChainLate<WaitSharded>{ChainGemm{ca.dx, H, nullptr, 0, ca.dqkv, ca.qkv_ld, ca.B, qkv_n, ca.attn_norm, ca.eps, nullptr},
                                      WaitSharded{ctr, nwg_down, ca.err, ca.naps, nullptr}, ca.trace ? ca.trace + (size_t)blockIdx.x * 8 : nullptr, ca.wqkv, ca.hqkv};
    });
}
__global__ __launch_bounds__(CH_THREADS, 4) void decode_chain_wc_k(const void* cdown, const void* cqkv, int hidden, int inter, int qkv_n, int nwg_down, ChainArgs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char msm[];
    chain_coded<1>(cdown, cqkv, hidden, inter, qkv_n, nwg_down, msm);
}
__global__ __launch_bounds__(CH_THREADS, 4) void decode_chain_w4_k(const void* cdown, const void* cqkv, int hidden, int inter, int qkv_n, int nwg_down, ChainArgs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char msm[];
    chain_coded<2>(cdown, cqkv, hidden, inter, qkv_n, nwg_down, msm);
}

// ---- decode attention + o_proj(+residual) in ONE launch, 16-wave workgroups -------------------------------------------------
// Workgroups [0, heads*B): attention exactly as the stand-alone latency kernel (wave 0 = new token, 15 cache waves),
// output stored write-through as tagged granules. Workgroups [heads*B, +ntiles/2): two o_proj tiles each (8 waves per tile), whose WHOLE
// K slice (16 chunks per wave) goes in flight at entry and sits in registers while attention runs; then the data-tagged
// hand-off (handoff.h: hint poll, granule sweep straight into the LDS staging) and ~2 us of work. heads*B + ntiles/2 <= 256 workgroups
// of <= 128 VGPRs: all resident, one per CU.
// Leading arguments (preloaded into SGPRs, rdx_kernels.h; 14 dwords, all there are): what the first loads of either role are addressed from -- o_proj:
// its weight base (the e4m3 bytes in the W8 instantiation), K, the tile count and where its workgroups start; attention: the qkv row(s), the layer's
// K / V cache and their geometry. K is also the hidden size and 128 heads' worth of it (attn_oproj16_supported), so neither travels twice.
// *at.epoch changes every step and stays a load: it is read behind the first loads of both roles (the tag is first needed by the hand-off).
template <typename Kernel> struct AttnOprojLate {       // the attention role's late arguments (attn_body.h); Kernel = attn_oproj16_k's own type
    // arguments 10 .. 13 of the kernel: DecAttnArgs, ChainGemm, hint, err
    static constexpr unsigned AT = kernarg_offset<10>(Kernel{}), G = kernarg_offset<11>(Kernel{}), HINT = kernarg_offset<12>(Kernel{}), ERR = kernarg_offset<13>(Kernel{});
    __device__ __forceinline__ DecAttnArgs operator()() const { return late_kernarg<DecAttnArgs>(AT); }
    __device__ __forceinline__ int* hint() const { return late_kernarg<int*>(HINT) + blockIdx.x; }
};
template <typename T, bool W8>
__global__ __launch_bounds__(CH_THREADS, 4) void attn_oproj16_k(const void* wo, const void* qkv, void* kcache, void* vcache, int K, int ntiles, int n_attn,
                                                                 int max_len, int qkv_ld, int k_perm, DecAttnArgs, ChainGemm, int*, int*) {
    extern __shared__ __attribute__((aligned(16))) unsigned char msm[];
    // debug timeline (rdx_gemv_trace 8; null in every product launch): one 8-slot record per workgroup, attention's slots in attn_body.h
    // ([6] = its stores acknowledged, written here: only a traced launch drains them), o_proj's those of chain_tile
    if ((int)blockIdx.x < n_attn) {
        const int heads = K >> 7;
        const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
        const AttnEarly e = {qkv, kcache, vcache, LlamaDims{K, heads, 128, qkv_ld, 0, 0.f, max_len, 0, k_perm}};
        const AttnOprojLate<decltype(&attn_oproj16_k<T, W8>)> late;
        decode_attention_core<T, CH_WAVES, true, NoWait, true, 0, true, false>(e, late, h, b, reinterpret_cast<float*>(msm), NoWait());
        const DecAttnArgs at = late();
        if (at.trace && threadIdx.x == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            at.trace[(size_t)blockIdx.x * 8 + 6] = (long long)__builtin_amdgcn_s_memrealtime();
        }
    } else {
        chain_tile<T, EPI_RESID, false, 2, 2, WaitTagged, W8 ? 4 : 8, true, W8>(wo, K, blockIdx.x - n_attn, ntiles, msm, [&] {
            typedef AttnOprojLate<decltype(&attn_oproj16_k<T, W8>)> L;
            const DecAttnArgs at = late_kernarg<DecAttnArgs>(L::AT);
            const ChainGemm g = late_kernarg<ChainGemm>(L::G);
            int* hint = late_kernarg<int*>(L::HINT);
            int* err = late_kernarg<int*>(L::ERR);
            return ChainLate<WaitTagged>{g, WaitTagged{hint, n_attn, at.epoch, at.layers, at.layer, err}, at.trace ? at.trace + (size_t)blockIdx.x * 8 : nullptr};
        });
    }
}

bool attn_oproj16_supported(const LlamaDims& d, int N, int K, int B) {
    const int ntiles = (N + 15) / 16;
    if (d.kv_fp8) return false;      // the fp8 KV cache is read by the stand-alone attention builds only
    return B <= CH_MAXM && d.head_dim == 128 && K == d.heads * 128 && K == d.hidden && K % 32 == 0 && N % 4 == 0 && (size_t)B * K <= 8192 &&
           d.heads * B + (ntiles + 1) / 2 <= 256;
}

void launch_attn_oproj16(int dtype, const DecAttnArgs& a, const GemmArgs& ga, int B, int* hint, int* err, hipStream_t s) {
    const int n_attn = a.d.heads * B, ntiles = (ga.N + 15) / 16;
    const bool w8 = ga.W8 && ga.wscale && ga.K % 64 == 0;
    // a.out = ga.X = the granule buffer: [B][K] elements as 8-byte {pair, tag} granules
    ChainGemm g = {ga.X, ga.ldx, ga.resid, ga.ldr, ga.out, ga.ldo, ga.M, ga.N, nullptr, 0.f, ga.wscale};
    const size_t sm_gemm = (size_t)(CH_WAVES * 256 + CH_WAVES * CH_MAXM + 16) * 4 + (size_t)B * ga.K * 2;
    const size_t sm_att = decode_attention_smem_floats(CH_WAVES, a.d.max_len) * sizeof(float);
    const size_t smem = sm_gemm > sm_att ? sm_gemm : sm_att;
    dim3 grid(n_attn + (ntiles + 1) / 2), block(CH_THREADS);
    RDX_DISPATCH_T(dtype, T, {
        if (w8) hipLaunchKernelGGL((attn_oproj16_k<T, true>), grid, block, smem, s, ga.W8, a.qkv, a.kcache, a.vcache, ga.K, ntiles, n_attn, a.d.max_len, a.d.qkv_ld,
                                   a.d.k_perm, a, g, hint, err);
        else hipLaunchKernelGGL((attn_oproj16_k<T, false>), grid, block, smem, s, ga.W, a.qkv, a.kcache, a.vcache, ga.K, ntiles, n_attn, a.d.max_len, a.d.qkv_ld,
                                a.d.k_perm, a, g, hint, err);
    });
}

bool chain_supported(const LlamaDims& d, int inter, int B) {
    if (B > CH_MAXM || d.head_dim != 128 || d.hidden % 32 || inter % 32 || d.hidden % 16) return false;
    const size_t stage = (size_t)B * (inter > d.hidden ? inter : d.hidden) * 2;
    // staged activations: <= 2 x 1024 chunks of 4 elements for the K = hidden unit, <= 6 x 1024 for down_proj (K = inter)
    return stage <= 48 * 1024 && inter % 4 == 0 && (size_t)B * d.hidden <= 8192 && (size_t)B * inter <= 24576;
}

size_t chain_ctr_ints(int layers) { return (size_t)layers * HO_CTR_INTS; }

void launch_decode_chain(int dtype, ChainArgs ca, bool with_next_qkv, hipStream_t s) {
    const int nwg_down = ca.hidden / 16;
    const int nwg_qkv = with_next_qkv ? ((ca.qkv_n + 15) / 16 + 3) / 4 : 0;
    const int kmax = ca.inter > ca.hidden ? ca.inter : ca.hidden;
    const size_t sm_gemm = (size_t)(CH_WAVES * 256 + CH_WAVES * CH_MAXM + 16) * 4 + (size_t)ca.B * kmax * 2 + 16;      // + the coded kernel's zero line
    // ONE workgroup per CU: the register budget alone (<= 128 VGPRs) would admit two, so reserve more than half of the LDS
    const size_t smem = sm_gemm > (size_t)84 * 1024 ? sm_gemm : (size_t)84 * 1024;
    dim3 grid(nwg_down + nwg_qkv), block(CH_THREADS);
    RDX_DISPATCH_T(dtype, T, {
        static DevOnce attr_set;
        if (attr_set.first()) {
            hipFuncSetAttribute((const void*)decode_chain_k<T, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024);
            hipFuncSetAttribute((const void*)decode_chain_k<T, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024);
        }
        if (ca.wc == 2 && dtype == DT_BF16 && !ca.w8) {       // int4 streams (api_llama.hip: every weight of the launch has one)
            static DevOnce w4_attr_set;
            if (w4_attr_set.first()) hipFuncSetAttribute((const void*)decode_chain_w4_k, hipFuncAttributeMaxDynamicSharedMemorySize, 100 * 1024);
            hipLaunchKernelGGL(decode_chain_w4_k, grid, block, smem, s, ca.cdown, with_next_qkv ? ca.cqkv : ca.cdown, ca.hidden, ca.inter, ca.qkv_n, nwg_down, ca);
        } else if (ca.wc && dtype == DT_BF16 && !ca.w8) {        // coded bf16 weights (api_llama.hip sets wc only where every copy of the launch exists)
            // the larger of the two roles' needs: the QKV role's `red` lies over its park region (chain_tile PARK), down_proj's carve-up is sm_gemm.
            // B * hidden <= 8192 (chain_supported): 208 B + at most 16 KiB of rows + 64 KiB per parked chunk, 147,664 B at depth 2 of the CU's 160 KiB
            const size_t sm_qkv = (size_t)(CH_WAVES * CH_MAXM + 16) * 4 + (size_t)ca.B * ca.hidden * 2 + 16 + CH_PARK_QKV * CH_PARK_BYTES;
            const size_t smem_wc = smem > sm_qkv ? smem : sm_qkv;
            static DevOnce wc_attr_set;
            if (wc_attr_set.first()) hipFuncSetAttribute((const void*)decode_chain_wc_k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            hipLaunchKernelGGL(decode_chain_wc_k, grid, block, smem_wc, s, ca.cdown, with_next_qkv ? ca.cqkv : ca.cdown, ca.hidden, ca.inter, ca.qkv_n, nwg_down, ca);
        } else if (ca.w8) hipLaunchKernelGGL((decode_chain_k<T, true>), grid, block, smem, s, ca.wdown8, ca.wqkv8, ca.hidden, ca.inter, ca.qkv_n, nwg_down, ca);
        else hipLaunchKernelGGL((decode_chain_k<T, false>), grid, block, smem, s, ca.wdown, ca.wqkv, ca.hidden, ca.inter, ca.qkv_n, nwg_down, ca);
    });
}

}  // namespace rdx
