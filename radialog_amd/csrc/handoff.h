// Workgroup-to-workgroup hand-off inside ONE launch (cdna_hip_programming.md G16). Three forms (the first is the recipe the other two shorten; no launch uses it today):
//   counter + fences (WaitCounter / publish)       plain payload, release fence, counter; acquire fence on the consumer;
//   counter, fence-free (WaitSharded / publish_sc1) write-through payload, drain, sharded counter; agent-scope loads: the chained down -> QKV launch (chain.hip);
//   data-tagged (WaitTagged / store_granule)        the payload carries its own tag, nothing else is signalled: the fused attention + o_proj launch (chain.hip).
//
// Counter form. Producer workgroup: plain stores -> every wave drains vmcnt -> __syncthreads -> ONE lane does an agent-scope release
// fence (L2 write-back: the 8 XCD L2s are not coherent with each other), drains again, then a relaxed agent-scope
// atomic add on the counter. Consumer workgroup: ONE lane polls the counter (relaxed, s_sleep between polls), then an
// agent-scope acquire fence (L1/L2 invalidate), __syncthreads, plain loads.
//
// Liveness: a workgroup only ever waits on workgroups with a SMALLER blockIdx (dispatched no later than itself), and a
// producer never waits on a consumer, so the lowest-indexed unfinished workgroup can always run to completion. Every
// spin is nevertheless bounded: on timeout the consumer sets *err and carries on (wrong numbers, reported by the host
// after the step -- never a hang).
#pragma once
#include "rdx_common.h"

namespace rdx {

typedef __attribute__((address_space(1))) int gint;   // GLOBAL (not flat) address space for the agent-scope accesses

// every wait policy says how the inputs arrive: TAGGED = false: wait, then load them (ld8_agent); true: the loads ARE the wait (WaitTagged)
struct NoWait { static constexpr bool TAGGED = false; __device__ __forceinline__ void operator()() const {} };

struct WaitCounter {
    static constexpr bool TAGGED = false;
    int* counter; int target; int* err;
    __device__ __forceinline__ void operator()() const {
        if (threadIdx.x == 0) {
            bool ok = false;
            gint* gc = (gint*)counter;
            for (int it = 0; it < (1 << 16); ++it) {         // bounded: tens of ms worst case, then give up loudly
                if (__hip_atomic_load(gc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) { ok = true; break; }
                __builtin_amdgcn_s_sleep(4);
            }
            if (!ok) *err = 1;
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        }
        __syncthreads();
    }
};

// all threads of the workgroup call this after their last store of the published data
__device__ __forceinline__ void publish(int* counter) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add((gint*)counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- fence-free form (write-through payload): used by chain.hip ---------------------------------------------------------
// Payload words are written with relaxed agent-scope 8-byte stores (sc1: write-through, the line leaves the writer's
// L2) and read with relaxed agent-scope 8-byte loads (sc1: bypass the reader's L1), so neither side needs a cache
// fence (a release fence costs 1.7-6.5 us per workgroup, an acquire 1.7 us and more with several workgroups per CU).
// The arrival counter is sharded 8 ways (one 64-byte line each): a single word serialises arrivals at ~13 ns apiece.
typedef __attribute__((address_space(1))) unsigned long long gu64;
__device__ __forceinline__ unsigned long long ld8_agent(const void* p) {
    return __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st8_agent(void* p, unsigned long long v) {
    __hip_atomic_store((gu64*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int HO_SHARDS = 8, HO_SHARD_STRIDE = 16;          // ints
constexpr int HO_CTR_INTS = HO_SHARDS * HO_SHARD_STRIDE;

// all threads call this after their last st8_agent of the published data; `idx` = this producer's index in its role
__device__ __forceinline__ void publish_sc1(int* ctr, int idx) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // EVERY storing wave drains its write-through stores
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_fetch_add((gint*)(ctr + (idx & (HO_SHARDS - 1)) * HO_SHARD_STRIDE), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct WaitSharded {     // wait until all `n` producers (indices 0..n-1) of a role have arrived; then read with ld8_agent
    static constexpr bool TAGGED = false;
    int* ctr; int n; int* err; int naps; long long* tr;   // tr: optional trace slot ([1] = inputs ready); naps: s_sleep(8) repeats between polls (pollers share 8 lines with the arrivals)
    __device__ __forceinline__ void operator()() const {
        if (n <= 0) {
            if (tr && threadIdx.x == 0) tr[1] = (long long)__builtin_amdgcn_s_memrealtime();
            return;
        }
        if (threadIdx.x < HO_SHARDS) {            // 8 lanes, one shard each: ONE 8-request load per poll
            const int k = threadIdx.x;
            const int need = (n - k + HO_SHARDS - 1) / HO_SHARDS;
            gint* gc = (gint*)(ctr + k * HO_SHARD_STRIDE);
            bool ok = false;
            for (int it = 0; it < (1 << 16); ++it) {
                ok = __hip_atomic_load(gc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= need;
                if (__all(ok)) break;
                for (int z = 0; z < naps; ++z) __builtin_amdgcn_s_sleep(8);
            }
            if (!__all(ok) && threadIdx.x == 0) *err = 1;
            if (tr && threadIdx.x == 0) tr[1] = (long long)__builtin_amdgcn_s_memrealtime();
        }
        __syncthreads();
    }
};

// ---- data-tagged form (G16 recipe R2: the data is the flag): used by the fused attention + o_proj launch -----------------------
// The payload travels as 8-byte granules {value: two model-dtype elements, tag}, each written by ONE aligned 8-byte write-through store and read by
// ONE 8-byte agent-scope load, so a granule is never torn and a matching tag proves its value: the producer neither drains its stores nor signals,
// the consumer re-reads its own granules until every tag matches and goes straight on into its LDS staging -- one fabric round trip instead of a
// drain, a counter add, a poll and a dependent load.
// Tag = epoch * layers + layer + 1 (mod 2^32, never 0): `epoch` is a device word that the tail of every step (and of the prefill) increments, read at
// kernel entry (it predates the launch), `layer` a kernel argument (per graph node, so replay keeps it). ONE granule buffer serves every layer, and
// that is what makes tags safe without zeroing: what a consumer can find stale is the tag of the fused launch just before, which differs.
// Sweeping from entry would put every consumer's granule loads beside the producers' own loads for as long as they run, so a hint word per producer
// (the tag, stored un-drained once the producer is about one round trip from its output) opens the sweep. Correctness does not rest on the hint.
__device__ __forceinline__ unsigned handoff_tag(int epoch, int layers, int layer) {
    const unsigned t = (unsigned)epoch * (unsigned)layers + (unsigned)layer + 1u;
    return t ? t : 0x80000000u;
}
__device__ __forceinline__ void store_hint(int* hint, int idx, unsigned tag) {
    __hip_atomic_store((gint*)(hint + idx), (int)tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one granule: elements (2 i, 2 i + 1) of the row-major payload live in granule i
__device__ __forceinline__ void store_granule(void* gran, size_t i, unsigned pair, unsigned tag) {
    st8_agent(reinterpret_cast<unsigned long long*>(gran) + i, ((unsigned long long)tag << 32) | pair);
}

struct WaitTagged {      // inputs arrive as tagged granules from `n` producers (hint words 0..n-1)
    static constexpr bool TAGGED = true;
    // the tag is derived HERE, from the step epoch (a device word that predates the launch): the consumer's weight ring is issued before this
    // load, not behind it
    const int* hint; int n; const int* epoch; int layers, layer; int* err;
    __device__ __forceinline__ unsigned the_tag() const { return handoff_tag(*epoch, layers, layer); }
    __device__ __forceinline__ void operator()() const {      // the opener: wave 0 polls the hints; a timeout here only starts the sweep early
        const unsigned tag = the_tag();
        if (threadIdx.x < 64) {
            for (int it = 0; it < (1 << 16); ++it) {
                bool ok = true;
                for (int i = threadIdx.x; i < n; i += 64)
                    ok = ok && (unsigned)__hip_atomic_load((gint*)(hint + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag;
                if (__all(ok)) break;
                __builtin_amdgcn_s_sleep(8);
            }
        }
        __syncthreads();
    }
    // every thread loads the two granules of each 4-element chunk c = threadIdx.x + i * nthreads it owns (row m = c / K4, `ld` elements apart) and
    // re-reads them until all tags of its wave match; xr[i] = the chunk as the wait-then-load form returns it. Bounded: on timeout *err = 1, go on.
    template <int XL>
    __device__ __forceinline__ void sweep(unsigned long long (&xr)[XL], const void* gran, int ld, int K4, int total4, int nthreads) const {
        const unsigned long long* g = reinterpret_cast<const unsigned long long*>(gran);
        const unsigned tag = the_tag();
        bool ok = false;
        for (int it = 0; it < (1 << 14); ++it) {
            ok = true;
#pragma unroll
            for (int i = 0; i < XL; ++i) {
                const int c = threadIdx.x + i * nthreads;
                xr[i] = 0ull;
                if (c < total4) {
                    const int m = c / K4, k4 = c - m * K4;
                    const unsigned long long* p = g + (((size_t)m * ld) >> 1) + (size_t)k4 * 2;
                    const unsigned long long lo = ld8_agent(p), hi = ld8_agent(p + 1);
                    ok = ok && (unsigned)(lo >> 32) == tag && (unsigned)(hi >> 32) == tag;
                    xr[i] = (lo & 0xffffffffull) | (hi << 32);
                }
            }
            if (__all(ok)) break;
            __builtin_amdgcn_s_sleep(2);
        }
        if (!__all(ok) && (threadIdx.x & 63) == 0) *err = 1;
    }
};

}  // namespace rdx
