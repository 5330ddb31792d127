// needle_packed_find_all_lane.h -- every non-overlapping match of every row of a PACKED batch (needle_packed_view) for patterns WITHOUT a
// find-all transducer: nullable patterns (`[a-c]*`), unbounded ones whose starts need indexBackwards (`http://.+`), nested dictionaries
// (`international|inter|nation`), `abc+d|ab`.  The reference's repeated Matcher.find() (DFAClassBuilder.java:616-659, nextStart = end) on
// each row, hand-written for gfx950 (CDNA4).  Included by needle_packed_find_all_lane{1,2}.hip (one per char width).
//
//   Staging: packed_kernel's (needle_packed.h packed_stream, unchanged): a wave owns 64 consecutive rows and streams their one contiguous
//   span through its LDS window; no 16-byte block without a byte of the group's span is loaded.
//   Walk: needle_find_all_walk.h's.  Every lane keeps its own BLOCK index (16-byte block counted from its row's origin) and cursor, and
//   walk_window iterates "every live lane walks its current block" (find_all_lane_step) until every live lane stands at or past the
//   window's end, or is done with its row.  Positions are origin-relative as in packed_kernel: the origin is the row's start rounded
//   down to its 16-byte block, the lane's first cursor the `skip` chars of the origin block in front of the row -- hidden by the guard
//   that hides the chars before any restart cursor (the lengths form with skip states: the search enters the block in skip state
//   fa_skip_lo + skip - 1).  The row's end is a ragged end: flags masked beyond `len`, the CUT re-walk for the lengths form.
//   Restarts: the block holding a lane's new cursor is read from the window while it is still there, else from memory, 16-byte blocks of
//   the lane's own row, until the lane is back in the window: the stream never moves backwards.  unresolved() = the row is not done;
//   wanted_from() = the address of the lane's current block.
//   Starts: the lengths programs (lmode / LM), the immediate form (backward_walk per match, the window as its text), or the deferred
//   find_all_starts_phase with the lane's slot of the by then free window for its text.
//   Results (FindAllArgs): counting only, or CSR filing at caller offsets (match k of row r at offsets[r] + k).  Result indices are
//   64-bit, positions row-relative int32 (rows of at most 2^31 - 1 chars); counts[r] = min(matches, room), *more = a row had more.
//
// Memory safety: the window loads are packed_stream's.  A restart block is block `pi` of the lane's row with pi * CPP < len: it holds a
// char of the row.  The deferred starts read the block of char end - 1 and blocks between it and the origin block: each holds a char of the
// row.  backward_walk reads single chars of [bound, end) -- inside the row.  Nothing else is loaded.
#pragma once
#include "needle_packed.h"
#include "needle_find_all_walk.h"

namespace needle {

// The packed rows of packed_find_all_lane_kernel as needle_find_all_walk.h's Rows policy: a row starts `skip` chars into its origin block
// at `org`; results go to two arrays at the caller's offsets; text: the wave's window.
template <int CW>
struct PackedLaneRows {
    const FindAllArgs &fa;
    const uint32_t win_base, slot; // the wave's window in LDS; this lane's CHB bytes of it
    const uint64_t org;            // the row's origin: its start rounded down to its 16-byte block
    const uint32_t skip;           // chars of the origin block before the row
    const uint32_t win_b0, bw_bytes; // the window's first byte, origin-relative (mod 2^32: negative when the row starts inside it), and
                                   // its size -- 0 where origin-relative BYTE offsets do not fit an int32: every char from memory
    __device__ __forceinline__ void file_match(uint64_t out0, uint32_t k, int32_t s, int32_t en) const { fa.starts[out0 + k] = s, fa.ends[out0 + k] = en; }
    __device__ __forceinline__ void file_end(uint64_t out0, uint32_t k, int32_t en) const { fa.ends[out0 + k] = en; }
    __device__ __forceinline__ int32_t read_end(uint64_t out0, uint32_t k) const { return __hip_atomic_load(&fa.ends[out0 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void file_start(uint64_t out0, uint32_t k, int32_t s, int32_t) const { fa.starts[out0 + k] = s; }
    __device__ __forceinline__ int32_t backward(bool act, int32_t en, int32_t bound) const {
        return backward_walk<CW>(fa.s, act, en, bound, win_base, win_b0, bw_bytes, 0u, (const uint8_t *)(uintptr_t)org);
    }
    __device__ __forceinline__ FindAllOwner owner(uint64_t, uint32_t l) const {
        auto of = [&](uint32_t x) __attribute__((always_inline)) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(l << 2), (int)x); };
        const uint64_t o_org = (uint64_t)of((uint32_t)org) | ((uint64_t)of((uint32_t)(org >> 32)) << 32);
        return {(const uint8_t *)(uintptr_t)o_org, of(skip)};
    }
    static __device__ __forceinline__ bool no_text(int32_t en) { return (uint32_t)en >= (1u << 30); }
    __device__ __forceinline__ uint32_t slot_addr() const { return slot; }
};

// LM: the "lengths" form (fa.lmode) of a program with skip states
template <int CW, int MODE, int CHB, bool LM>
__global__ __launch_bounds__(kWavesPerBlock * 64) void packed_find_all_lane_kernel(const PackedFindAllArgs pf) {
    const FindAllArgs &fa = pf.f;
    const ScanArgs &a = fa.s;
    constexpr uint32_t kWin = 64u * CHB;
    constexpr int CPP = 16 / CW; // chars per 16-byte block
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_waves = blockDim.x >> 6;

    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();
    for (uint32_t i = tid * 16u; i < a.hdr.lds_bytes; i += blockDim.x * 16u)
        *(u32x4 *)(smem + i) = *(const u32x4 *)(a.prog + i);
    __syncthreads();

    FindAllWalk fw;
    find_all_walk_setup<CW, MODE>(a, lane, fw);

    const PackedWindow<CHB> win(a.hdr.lds_bytes, 0u, wave);
    const uint64_t n_rows = a.n_rows;

    // ---- per-group (per-row) state
    uint64_t rs, re;     // this lane's row as absolute byte addresses [rs, re) (packed_stream)
    uint64_t org = 0;    // the row's origin: rs rounded down to its 16-byte block
    uint32_t skip = 0;   // chars of the origin block before the row
    bool row_ok = false;
    FindAllRow row = {}; // (row.len: skip + the row's chars)
    row.done = true, row.last = -1;
    auto rows_at = [&](uint32_t win_b0, uint32_t bw_bytes) __attribute__((always_inline)) {
        return PackedLaneRows<CW>{fa, win.base, win.at((uint32_t)lane * CHB), org, skip, win_b0, bw_bytes};
    };

    auto begin_group = [&](uint64_t grp) __attribute__((always_inline)) {
        const uint64_t my_row = (grp << 6) + (uint64_t)lane;
        row_ok = my_row < n_rows;
        org = rs & ~(uint64_t)15;
        skip = (uint32_t)(rs & 15u) / CW;
        row.len = skip + (uint32_t)((re - rs) / CW);
        row.cursor = (int32_t)skip;
        row.pi = 0;
        row.count = 0;
        row.st = fw.start_state;
        if (LM) row.st = skip ? a.hdr.fa_skip_lo + skip - 1u : fw.start_state; // S_k swallows the skip chars in front of the row
        row.last = a.hdr.root_accepting ? (int32_t)skip : -1; // :356 literal 0 (row-relative)
        row.out0 = 0;
        row.cap = fa.count_only ? 0xFFFFFFFFu : 0u;
        if (fa.offsets) {
            row.out0 = row_ok ? fa.offsets[my_row] : 0ull;
            row.cap = row_ok ? (uint32_t)(fa.offsets[my_row + 1] - row.out0) : 0u;
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(row.cap)); // (no vmcnt wait inside the walk)
        }
        row.done = !row_ok;
        // An EMPTY row has no block of its own (a group of empty rows has no window at all): its find() is decided here -- the one empty
        // match of a pattern that accepts the empty string (what the fixed-stride kernel's walk over PAD arrives at), else nothing.
        if (row_ok && row.len == skip) {
            row.done = true;
            if (a.hdr.root_accepting) {
                const bool file = row.count < row.cap;
                if (!file) *fa.more = 1;
                if (file && !fa.count_only) rows_at(0u, 0u).file_match(row.out0, 0u, 0, 0);
                row.count = file ? 1u : 0u;
            }
        }
    };

    // Walk the window at w (its bytes are in LDS) until every live lane is past it or done.
    auto walk_window = [&](uint64_t w) __attribute__((always_inline)) {
        const uint64_t wend = w + kWin;
        const auto rows = rows_at((uint32_t)(w - org), row.len < (1u << 30) ? kWin : 0u);
        for (;;) {
            const uint32_t p0 = row.pi * CPP;
            const uint64_t ba = org + ((uint64_t)row.pi << 4); // the lane's current block
            const bool beyond = p0 >= row.len; // nothing of the row there (a walk over PAD: the search ends)
            const bool active = !row.done && (ba < wend || beyond);
            if (__ballot(active) == 0ull) break;
            // (straight-line code for all 64 lanes, idle ones included: find_all_lane_step)
            const bool in_lds = active && !beyond && ba >= w;
            u32x4 v = *(const lds_u32x4 *)(uintptr_t)win.at(in_lds ? (uint32_t)(ba - w) : 0u);
            const bool in_mem = active && !beyond && ba < w;
            if (__ballot(in_mem) != 0ull) { // a restart behind the window (rare): waited for HERE, so that the common path carries no
                                            // vmcnt wait (the window prefetch and match stores are in flight)
                if (in_mem) {
                    v = *(const u32x4 *)(uintptr_t)ba; // (block pi of the row, pi * CPP < len: it holds a char of the row)
                    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v));
                }
            }
            const uint32_t w4[4] = {v[0], v[1], v[2], v[3]}; // (a block beyond the row: whatever is there -- its flags are masked)
            find_all_lane_step<CW, MODE, LM>(fa, fw, rows, w4, active, p0, row);
        }
    };

    auto finish_rows = [&](uint64_t grp) __attribute__((always_inline)) {
        if (row_ok && fa.counts) fa.counts[(grp << 6) + (uint64_t)lane] = row.count;
        if (fa.defer && !fa.count_only) find_all_starts_phase<CW>(fa, rows_at(0u, 0u), lane, grp, row);
    };

    packed_stream<CW, CHB>(lane, wave, n_waves, a.rows, pf.row_offsets, n_rows, win, rs, re, begin_group, walk_window,
                           [&]() __attribute__((always_inline)) { return !row.done; },
                           [&]() __attribute__((always_inline)) { return org + ((uint64_t)row.pi << 4); }, finish_rows);
}

template <int CW, int MODE, int CHB, bool LM>
static hipError_t launch_packed_find_all_lane_one(const PackedFindAllArgs &a, int grid, int waves, size_t lds, hipStream_t stream) {
    auto k = packed_find_all_lane_kernel<CW, MODE, CHB, LM>;
    static thread_local uint64_t configured = 0;
    if (hipError_t e = allow_full_lds((const void *)k, configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(waves * 64), lds, stream, a);
    return hipGetLastError();
}

template <int CW, int MODE>
static hipError_t launch_packed_find_all_lane_h(const PackedFindAllArgs &a, int chb, int grid, int waves, size_t lds, hipStream_t s) {
    if constexpr (MODE == MODE_TABLE8 || MODE == MODE_TABLE16) {
        if (a.f.lmode && a.f.s.hdr.fa_skip_lo)
            return chb == 128 ? launch_packed_find_all_lane_one<CW, MODE, 128, true>(a, grid, waves, lds, s)
                              : launch_packed_find_all_lane_one<CW, MODE, 64, true>(a, grid, waves, lds, s);
    }
    return chb == 128 ? launch_packed_find_all_lane_one<CW, MODE, 128, false>(a, grid, waves, lds, s)
                      : launch_packed_find_all_lane_one<CW, MODE, 64, false>(a, grid, waves, lds, s);
}

template <int CW>
static hipError_t launch_packed_find_all_lane_m(const PackedFindAllArgs &a, int chb, int grid, int waves, size_t lds, hipStream_t s) {
    switch (a.f.s.hdr.mode) {
    case MODE_PACK: return launch_packed_find_all_lane_h<CW, MODE_PACK>(a, chb, grid, waves, lds, s);
    case MODE_TABLE8: return launch_packed_find_all_lane_h<CW, MODE_TABLE8>(a, chb, grid, waves, lds, s);
    case MODE_TABLE16: return launch_packed_find_all_lane_h<CW, MODE_TABLE16>(a, chb, grid, waves, lds, s);
    default: return hipErrorInvalidValue; // (hot-rows, HBM-table and compressed programs: the caller converts the batch)
    }
}

} // namespace needle
