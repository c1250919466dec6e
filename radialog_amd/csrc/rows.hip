// Row sessions (api_rows.hip): moving a freshly prefilled STAGING row of the decoder into a live row, and parking a row nobody uses.
// A staging row is an ordinary row of every per-row array (KV cache, decode state) above the rows the step runs on; the prompt path filled it exactly as
// rdx_prefill fills row b. Both kernels are plain copies: nothing here touches the hand-off counters or the step epoch (handoff.h).
#include "rdx_common.h"
#include "rdx_kernels.h"

namespace rdx {

// KV cache [layer][K|V is a separate base][row][head][max_len][128] (2-byte elements: 256 bytes per position). Positions [0, npos) of every head of row
// src[i] -> row dst[i], all layers, K and V. npos is a multiple of 16 (or max_len), so a K slab's 16-position fragment groups (k_perm) move whole, as in
// kv_beam_copy_k. Source rows (staging) and target rows (live) never overlap: no scratch copy. grid: (n * heads, layers, 2). 16 bytes per thread per trip.
__global__ __launch_bounds__(256) void kv_rows_move_k(char* __restrict__ kcache, char* __restrict__ vcache, RowList rl, int heads, int max_len,
                                                      size_t layer_bytes, int npos) {
    const int ih = blockIdx.x, i = ih / heads, h = ih % heads, layer = blockIdx.y, kv = blockIdx.z;
    char* base = (kv ? vcache : kcache) + (size_t)layer * layer_bytes;
    const char* from = base + ((size_t)rl.src[i] * heads + h) * max_len * 256;
    char* to = base + ((size_t)rl.dst[i] * heads + h) * max_len * 256;
    const size_t span = (size_t)npos * 256;
    for (size_t o = (size_t)threadIdx.x * 16; o < span; o += (size_t)blockDim.x * 16) stg16(to + o, ldg16(from + o));
}

void launch_kv_rows_move(void* kcache, void* vcache, const RowList& rl, int heads, int layers, int max_len, size_t layer_bytes, int npos, hipStream_t s) {
    if (rl.n <= 0 || npos <= 0) return;
    hipLaunchKernelGGL(kv_rows_move_k, dim3(rl.n * heads, layers, 2), dim3(256), 0, s, (char*)kcache, (char*)vcache, rl, heads, max_len, layer_bytes, npos);
}

// The per-row decode state of staged row src[i] -> live row dst[i]: next position, cache slot, step count, the unfinished flag, the key-mask row, the next
// input embedding (dx) and the cos | sin row of the next position. The target's out_tokens row is cleared to pad_id and takes token 0 (what the prompt
// pass selected into the staging token row) in column 0.
// park != 0 (dst only): the row becomes a PARKED one -- slot 0, position 0, finished, step count = cap -- which still runs a one-position step but writes
// no token (step_tail: step < max_new) and, re-parked before every rdx_rows_step call, cannot walk out of its cache row. Its key-mask row is all ones and
// its dx / cos | sin rows are zero: finite inputs whatever the row held before. park & 2 (rdx_rows_begin): its out_tokens row is cleared as well.
// One workgroup per listed row.
__global__ __launch_bounds__(256) void row_state_move_k(RowState st, RowList rl, int park) {
    const int i = blockIdx.x, d = rl.dst[i], tid = threadIdx.x;
    uint8_t* km_d = st.key_mask + (size_t)d * st.max_len;
    char* dx_d = (char*)st.dx + (size_t)d * st.H * 2;
    char* rope_d = (char*)st.cur_rope + (size_t)d * 512;
    int32_t* tok_d = st.out_tokens + (size_t)d * st.cap;
    if (park) {
        if (tid == 0) { st.slot[d] = 0; st.pos[d] = 0; st.unf[d] = 0; st.step[d] = st.cap; }
        for (int t = tid; t < st.max_len; t += blockDim.x) km_d[t] = 1;
        const u4 z = {0u, 0u, 0u, 0u};
        for (int o = tid * 16; o < st.H * 2; o += blockDim.x * 16) stg16(dx_d + o, z);
        if (tid < 32) stg16(rope_d + tid * 16, z);
        if (park & 2) for (int t = tid; t < st.cap; t += blockDim.x) tok_d[t] = st.pad_id;
        return;
    }
    const int sr = rl.src[i];
    if (tid == 0) { st.slot[d] = st.slot[sr]; st.pos[d] = st.pos[sr]; st.unf[d] = st.unf[sr]; st.step[d] = st.step[sr]; }
    const uint8_t* km_s = st.key_mask + (size_t)sr * st.max_len;
    for (int t = tid; t < st.max_len; t += blockDim.x) km_d[t] = km_s[t];
    const char* dx_s = (const char*)st.dx + (size_t)sr * st.H * 2;
    for (int o = tid * 16; o < st.H * 2; o += blockDim.x * 16) stg16(dx_d + o, ldg16(dx_s + o));
    if (tid < 32) stg16(rope_d + tid * 16, ldg16((const char*)st.cur_rope + (size_t)sr * 512 + tid * 16));
    const int tok0 = st.stage_tokens[(size_t)(sr - st.row0) * st.cap];
    for (int t = tid; t < st.cap; t += blockDim.x) tok_d[t] = t == 0 ? tok0 : st.pad_id;
}

void launch_row_state_move(const RowState& st, const RowList& rl, int park, hipStream_t s) {
    if (rl.n <= 0) return;
    hipLaunchKernelGGL(row_state_move_k, dim3(rl.n), dim3(256), 0, s, st, rl, park);
}

}  // namespace rdx
