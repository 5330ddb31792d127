// needle_csr_rows.h -- what the kernels that take a CSR list over the rows of a packed batch share (needle_replace.hip: the match list
// that is spliced; needle_set_spans.h: the span list that is tagged; needle_utf8.hip: the position list that is mapped): a wave owns a
// 64-row group, keeps the group's 65 list offsets and 65 row offsets in its LDS, and a lane finds the row of its list entry there and
// clamps the entry into that row.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace needle {

// A wave's own LDS traffic is in order; this keeps the compiler from moving accesses across the hand-over between lanes.
__device__ __forceinline__ void csr_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The group's 65 list offsets and 65 row offsets (rows beyond the batch: empty, with no entries) into the wave's LDS.
__device__ __forceinline__ void csr_group_offsets(const uint64_t *list_off, const uint64_t *row_off, uint64_t n_rows, uint64_t g0, int lane,
                                                  uint64_t *mo, uint64_t *ino) {
    const uint64_t r = g0 + (uint64_t)lane < n_rows ? g0 + (uint64_t)lane : n_rows;
    mo[lane] = list_off[r];
    ino[lane] = row_off[r];
    if (lane == 0) {
        const uint64_t r2 = g0 + 64u < n_rows ? g0 + 64u : n_rows;
        mo[64] = list_off[r2];
        ino[64] = row_off[r2];
    }
}

// ... the 65 row offsets alone (needle_utf8.hip: kernels without a list).
__device__ __forceinline__ void csr_group_row_offsets(const uint64_t *row_off, uint64_t n_rows, uint64_t g0, int lane, uint64_t *ino) {
    const uint64_t r = g0 + (uint64_t)lane < n_rows ? g0 + (uint64_t)lane : n_rows;
    ino[lane] = row_off[r];
    if (lane == 0) ino[64] = row_off[g0 + 64u < n_rows ? g0 + 64u : n_rows];
}

// The row (0 .. 63 within the group) of list entry m: the last r with mo[r] <= m.
__device__ __forceinline__ uint32_t csr_row_of(const uint64_t *mo, uint64_t m) {
    uint32_t r = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1)
        if (mo[r + step] <= m) r += step;
    return r;
}

// The entry (s32, e32) clamped into a row of `len` code units: *s = clamp(s32, 0, len), *e = clamp(e32, *s, len).
__device__ __forceinline__ void csr_clamp(int32_t s32, int32_t e32, uint64_t len, uint64_t *s, uint64_t *e) {
    const uint64_t sc = s32 < 0 ? 0ull : ((uint64_t)s32 > len ? len : (uint64_t)s32);
    const uint64_t ec = e32 < 0 ? 0ull : ((uint64_t)e32 > len ? len : (uint64_t)e32);
    *s = sc;
    *e = ec < sc ? sc : ec;
}

} // namespace needle
