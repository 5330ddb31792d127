// needle_utf8.hip -- UTF-8 packed rows transcoded where they lie into the UTF-16 packed batch every kernel takes, and the code-unit
// positions those kernels file mapped back to byte offsets of the UTF-8, hand-written for gfx950 (CDNA4): the kernels of
// needle_utf16_lengths_from_utf8_packed_dev / needle_utf16_from_utf8_packed_dev / needle_utf8_positions_packed_dev
// (include/needle_hip.h).  The rule is needle_utf8.h's utf8_classify16, called by all three.
//
//   A wave owns a 64-row group: ONE contiguous span of text; its 65 row offsets sit in the wave's LDS (needle_csr_rows.h).
//   Lengths and fill are POSITION-parallel.  The wave walks the span in steps of 64 lanes x one aligned 16-byte block (kUtf8WindowBytes):
//     coalesced 16-byte global_* loads, the next step's blocks in flight while this step's are classified.  A block is loaded only when it
//     holds a byte of the span (the packed kernels' rule) and its bytes outside the span are zeroed -- first and last block are the
//     guarded ones.  The three bytes before and behind a block are the neighbour lanes' (cross-lane moves); lane 0 gets them from the
//     step before (a wave-uniform carry), lane 63 from the next step's lane 0, which is loaded already.  The rows a block touches are
//     found by a binary search in the LDS offsets: every row start within [block - 4, block + 20) becomes a bit of first24.
//     A step without a byte >= 0x80 skips all of that: every byte is a start that files itself.
//   Lengths: the step's four masks go to LDS (8 bytes per 16 of text), then lane = row counts the bits of its own byte range: 64 at a
//     time, so a row longer than a step adds up in its lane's register over the steps.  The two bitmaps are ballots: one plain store per
//     word.  LDS: 65 * 8 + 4 * 128 = 1032 bytes per wave.
//   Fill: rows are back to back in the input AND in the output (out_off is the prefix sum of the lengths), so the group's units are one
//     contiguous run from out_off[g0]: a unit's place is that, plus the units of the steps before (wave-uniform), plus the wave's
//     exclusive prefix sum of the blocks' popcounts.  A lane stores its <= 17 units with 2-byte stores; neighbouring lanes write
//     neighbouring addresses.  Nothing is stored outside [out_off[g0], out_off[g1]) clamped into [out_off[0], out_off[n_rows]).
//     LDS: 2 * 65 * 8 = 1040 bytes per wave.
//   Positions: lane = row, as set_spans_kernel's lanes are spans.  A lane sweeps the aligned 16-byte blocks of its own row straight from
//     global memory (other rows' bytes zeroed, so the one-row form of the rule serves), keeping the units before the current block; an
//     entry inside the block is resolved by popcounts of the masks below a byte, found by bisection.  Entries that do not decrease go
//     on from where the sweep stands; a decreasing one restarts it.  Limit: a long row with entries runs at one lane's pace.
//     LDS: 2 * 65 * 8 = 1040 bytes per wave.
#include <hip/hip_runtime.h>

#include "needle_csr_rows.h"
#include "needle_launch.h"
#include "needle_utf8.h"

namespace needle {

typedef uint32_t u8_u32x4 __attribute__((ext_vector_type(4)));
// (global_* loads and stores: flat ones would count on the LDS counter too -- needle_replace.hip)
#define U8_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ uint64_t utf8_clamp(uint64_t x, uint64_t lo, uint64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Bit j: byte X + j lies in [lo, hi).
__device__ __forceinline__ uint32_t utf8_valid16(uint64_t X, uint64_t lo, uint64_t hi) {
    const uint32_t a = lo > X ? (lo - X < 16u ? (uint32_t)(lo - X) : 16u) : 0u;
    const uint32_t b = hi > X ? (hi - X < 16u ? (uint32_t)(hi - X) : 16u) : 0u;
    return ((1u << b) - 1u) & ~((1u << a) - 1u);
}

// The aligned block at X, zeros for every byte outside [lo, hi); not loaded when it holds none of them.
__device__ __forceinline__ u8_u32x4 utf8_load_block(uint64_t X, uint64_t lo, uint64_t hi) {
    u8_u32x4 v = {0u, 0u, 0u, 0u};
    if (X < hi && X + 16u > lo) {
        v = *(const U8_GLOBAL u8_u32x4 *)(uintptr_t)X;
        if (X < lo || X + 16u > hi) { // an edge of the range
            const uint32_t ok = utf8_valid16(X, lo, hi);
#pragma unroll
            for (int d = 0; d < 4; ++d) v[d] &= (utf8_detail::spread4(ok >> (4 * d)) >> 7) * 0xFFu;
        }
    }
    return v;
}

// The row starts (and the group's end) within the window [X - 4, X + 20) of the block at X, as bits: the rows' absolute addresses are
// dbase + ino[0 .. 64], non-decreasing.
__device__ __forceinline__ uint32_t utf8_first24(const uint64_t *ino, uint64_t dbase, uint64_t X) {
    const uint64_t lo = X - 4u;
    uint32_t at = 0; // the offsets below the window
#pragma unroll
    for (uint32_t step = 64; step; step >>= 1)
        if (at + step <= 65u && dbase + ino[at + step - 1u] < lo) at += step;
    uint32_t first = 0;
    for (; at <= 64u; ++at) {
        const uint64_t A = dbase + ino[at];
        if (A >= lo + 24u) break;
        if (A >= lo) first |= 1u << (uint32_t)(A - lo);
    }
    return first;
}

// One step of the position-parallel kernels: the lane's block `cur` at X (its bytes outside the span [inB, inE) zeroed), the blocks of the
// next step loaded already (`nxt0`: their first dwords), `carry` the last dword of the block before this step's first.
__device__ __forceinline__ Utf8Masks utf8_step(const u8_u32x4 cur, uint32_t nxt0, uint32_t carry, uint64_t X, uint64_t inB, uint64_t inE,
                                               const uint64_t *ino, uint64_t dbase, int lane, uint32_t *behind) {
    uint32_t before = (uint32_t)__shfl_up((int)cur[3], 1, 64), after = (uint32_t)__shfl_down((int)cur[0], 1, 64);
    const uint32_t next_first = (uint32_t)__builtin_amdgcn_readlane((int)nxt0, 0);
    if (lane == 0) before = carry;
    if (lane == 63) after = next_first;
    *behind = after;
    const uint32_t valid = utf8_valid16(X, inB, inE);
    Utf8Masks m = {valid, 0u, 0u, 0u};
    if (__ballot(((cur[0] | cur[1] | cur[2] | cur[3]) & 0x80808080u) != 0u) != 0ull) { // (wave-uniform)
        m = utf8_classify16<false>(cur[0], cur[1], cur[2], cur[3], before, after, utf8_first24(ino, dbase, X));
        m.starts &= valid; // (a zero byte outside the span reads as a start; pairs, bad and high are not set for one)
    }
    return m;
}

__global__ __launch_bounds__(kUtf8Waves * 64) void utf8_lengths_kernel(const Utf8Args a) {
    __shared__ uint64_t s_ino[kUtf8Waves][65];
    __shared__ __attribute__((aligned(8))) uint16_t s_mask[kUtf8Waves][4][64]; // a step's starts | pairs | bad | high, 16 bits per block
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *ino = s_ino[wave];
    uint16_t(*mask)[64] = s_mask[wave];
    const uint64_t n = a.n_rows, n_groups = (n + 63u) >> 6;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.data;
    const uint64_t in_first = a.in_off[0], in_last = a.in_off[n];
    for (uint64_t grp = (uint64_t)blockIdx.x * kUtf8Waves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kUtf8Waves) {
        const uint64_t g0 = grp << 6;
        csr_group_row_offsets(a.in_off, n, g0, lane, ino);
        csr_wave_sync();
        const uint64_t in_b = utf8_clamp(ino[0], in_first, in_last);
        const uint64_t inB = dbase + in_b, inE = dbase + utf8_clamp(ino[64], in_b, in_last);
        // lane = row: its own byte range, inside the group's
        const uint64_t rowB = utf8_clamp(dbase + ino[lane], inB, inE), rowE = utf8_clamp(dbase + ino[lane + 1], rowB, inE);
        uint64_t units = 0;
        bool non_ascii = false, malformed = false;
        const uint64_t X0 = inB & ~(uint64_t)15;
        u8_u32x4 cur = utf8_load_block(X0 + (uint64_t)lane * 16u, inB, inE);
        uint32_t carry = 0;
        for (uint64_t Xw = X0; Xw < inE; Xw += kUtf8WindowBytes) {
            const uint64_t X = Xw + (uint64_t)lane * 16u;
            const u8_u32x4 nxt = utf8_load_block(X + kUtf8WindowBytes, inB, inE);
            uint32_t behind;
            const Utf8Masks m = utf8_step(cur, nxt[0], carry, X, inB, inE, ino, dbase, lane, &behind);
            carry = (uint32_t)__builtin_amdgcn_readlane((int)cur[3], 63);
            mask[0][lane] = (uint16_t)m.starts, mask[1][lane] = (uint16_t)m.pairs, mask[2][lane] = (uint16_t)m.bad, mask[3][lane] = (uint16_t)m.high;
            csr_wave_sync();
            const uint64_t lo = rowB > Xw ? rowB : Xw, hi = rowE < Xw + kUtf8WindowBytes ? rowE : Xw + kUtf8WindowBytes;
            if (lo < hi) { // the row's bytes of this step: bits [b0, b1] of the step's masks
                const uint32_t b0 = (uint32_t)(lo - Xw), b1 = (uint32_t)(hi - Xw) - 1u;
                for (uint32_t wd = b0 >> 6; wd <= (b1 >> 6); ++wd) {
                    uint64_t own = ~0ull;
                    if (wd == (b0 >> 6)) own &= ~0ull << (b0 & 63u);
                    if (wd == (b1 >> 6)) own &= ~0ull >> (63u - (b1 & 63u));
                    units += (uint64_t)(__popcll(((const uint64_t *)mask[0])[wd] & own) + __popcll(((const uint64_t *)mask[1])[wd] & own));
                    malformed |= (((const uint64_t *)mask[2])[wd] & own) != 0ull;
                    non_ascii |= (((const uint64_t *)mask[3])[wd] & own) != 0ull;
                }
            }
            csr_wave_sync(); // (the next step overwrites the masks)
            cur = nxt;
        }
        if (g0 + (uint64_t)lane < n) a.out_len[g0 + (uint64_t)lane] = units;
        const uint64_t na = __ballot(non_ascii), mal = __ballot(malformed); // (rows beyond the batch are empty: their bits are 0)
        if (lane == 0) {
            if (a.non_ascii) a.non_ascii[grp] = na;
            if (a.malformed) a.malformed[grp] = mal;
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

__global__ __launch_bounds__(kUtf8Waves * 64) void utf8_fill_kernel(const Utf8Args a) {
    __shared__ uint64_t s_oo[kUtf8Waves][65], s_ino[kUtf8Waves][65];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *oo = s_oo[wave], *ino = s_ino[wave];
    const uint64_t n = a.n_rows, n_groups = (n + 63u) >> 6;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.data;
    const uint64_t in_first = a.in_off[0], in_last = a.in_off[n], out_first = a.out_off[0], out_last = a.out_off[n];
    U8_GLOBAL uint16_t *out = (U8_GLOBAL uint16_t *)(uintptr_t)a.out;
    for (uint64_t grp = (uint64_t)blockIdx.x * kUtf8Waves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kUtf8Waves) {
        csr_group_offsets(a.out_off, a.in_off, n, grp << 6, lane, oo, ino);
        csr_wave_sync();
        const uint64_t in_b = utf8_clamp(ino[0], in_first, in_last);
        const uint64_t inB = dbase + in_b, inE = dbase + utf8_clamp(ino[64], in_b, in_last);
        uint64_t at = utf8_clamp(oo[0], out_first, out_last); // the unit the step's first start files (wave-uniform)
        const uint64_t out_e = utf8_clamp(oo[64], at, out_last);
        const uint64_t X0 = inB & ~(uint64_t)15;
        u8_u32x4 cur = utf8_load_block(X0 + (uint64_t)lane * 16u, inB, inE);
        uint32_t carry = 0;
        for (uint64_t Xw = X0; Xw < inE; Xw += kUtf8WindowBytes) {
            const uint64_t X = Xw + (uint64_t)lane * 16u;
            const u8_u32x4 nxt = utf8_load_block(X + kUtf8WindowBytes, inB, inE);
            uint32_t behind;
            const Utf8Masks m = utf8_step(cur, nxt[0], carry, X, inB, inE, ino, dbase, lane, &behind);
            carry = (uint32_t)__builtin_amdgcn_readlane((int)cur[3], 63);
            const uint32_t mine = (uint32_t)(__popc(m.starts) + __popc(m.pairs));
            uint32_t incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
                if (lane >= d) incl += up;
            }
            uint64_t pos = at + (uint64_t)(incl - mine);
            at += (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (m.starts != 0u) {
                const uint32_t v[5] = {cur[0], cur[1], cur[2], cur[3], behind};
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    if ((m.starts >> j) & 1u) {
                        const int d = j >> 2, sh = 8 * (j & 3);
                        const uint32_t q = sh ? (v[d] >> sh) | (v[d + 1] << (32 - sh)) : v[d];
                        uint32_t low;
                        const uint32_t unit = utf8_unit(q, ((m.bad >> j) & 1u) != 0u, &low);
                        if (pos < out_e) out[pos] = (uint16_t)unit;
                        ++pos;
                        if ((m.pairs >> j) & 1u) {
                            if (pos < out_e) out[pos] = (uint16_t)low;
                            ++pos;
                        }
                    }
                }
            }
            cur = nxt;
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

__global__ __launch_bounds__(kUtf8Waves * 64) void utf8_positions_kernel(const Utf8Args a) {
    __shared__ uint64_t s_mo[kUtf8Waves][65], s_ino[kUtf8Waves][65];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave];
    const uint64_t n = a.n_rows, n_groups = (n + 63u) >> 6;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.data;
    const uint64_t in_first = a.in_off[0], in_last = a.in_off[n];
    for (uint64_t grp = (uint64_t)blockIdx.x * kUtf8Waves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kUtf8Waves) {
        csr_group_offsets(a.list_off, a.in_off, n, grp << 6, lane, mo, ino);
        csr_wave_sync();
        uint64_t m = mo[lane];
        const uint64_t m_end = mo[lane + 1];
        // lane = row: its bytes [rowB, rowE) inside the batch's, the aligned blocks that hold them
        const uint64_t r_b = utf8_clamp(ino[lane], in_first, in_last);
        const uint64_t rowB = dbase + r_b, rowE = dbase + utf8_clamp(ino[lane + 1], r_b, in_last);
        const uint64_t len = rowE - rowB < 0x7FFFFFFFull ? rowE - rowB : 0x7FFFFFFFull;
        const uint64_t b0 = rowB & ~(uint64_t)15;
        const uint32_t n_blk = rowE > rowB ? (uint32_t)((rowE - b0 + 15u) >> 4) : 0u;
        auto load = [&](uint32_t k) __attribute__((always_inline)) {
            const u8_u32x4 zero = {0u, 0u, 0u, 0u};
            return k < n_blk ? utf8_load_block(b0 + (uint64_t)k * 16u, rowB, rowE) : zero;
        };
        // the sweep: block k, `u_base` units before it, `u` units in it
        bool swept = false, have_p = false;
        uint32_t k = 0, u_base = 0, u = 0, before = 0;
        int32_t p = 0;
        u8_u32x4 cur = {0u, 0u, 0u, 0u}, nxt = {0u, 0u, 0u, 0u};
        Utf8Masks mk = {0u, 0u, 0u, 0u};
        while (__ballot(m < m_end) != 0ull) {
            if (m < m_end) {
                if (!have_p) {
                    p = a.unit_pos[m];
                    have_p = true;
                }
                if (p < 0 || n_blk == 0u) { // passed through; an empty row: B(0) = len = 0
                    a.byte_pos[m] = p < 0 ? -1 : 0;
                    ++m;
                    have_p = false;
                } else {
                    bool fresh = false;
                    if (!swept || (uint32_t)p < u_base) { // the first entry, or one that decreases: from the row's start
                        swept = true;
                        k = 0, u_base = 0, before = 0;
                        cur = load(0u), nxt = load(1u);
                        fresh = true;
                    } else if ((uint32_t)p >= u_base + u && k + 1u < n_blk) { // behind this block
                        u_base += u;
                        before = cur[3];
                        cur = nxt;
                        ++k;
                        nxt = load(k + 1u);
                        fresh = true;
                    }
                    if (fresh) {
                        mk = utf8_classify16<true>(cur[0], cur[1], cur[2], cur[3], before, nxt[0], 0u);
                        mk.starts &= utf8_valid16(b0 + (uint64_t)k * 16u, rowB, rowE);
                        u = (uint32_t)(__popc(mk.starts) + __popc(mk.pairs));
                    } else { // in this block, or behind the row's last unit
                        const uint32_t q = (uint32_t)p - u_base;
                        int32_t B = (int32_t)len;
                        if (q < u) {
                            uint32_t j = 0; // the bytes whose units, their own included, do not reach q: the start that files unit q
#pragma unroll
                            for (uint32_t step = 8; step; step >>= 1) {
                                const uint32_t below = (2u << (j + step - 1u)) - 1u;
                                if ((uint32_t)(__popc(mk.starts & below) + __popc(mk.pairs & below)) <= q) j += step;
                            }
                            B = (int32_t)(b0 + (uint64_t)k * 16u + j - rowB);
                        }
                        a.byte_pos[m] = B;
                        ++m;
                        have_p = false;
                    }
                }
            }
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

static int utf8_grid(uint64_t n_rows, int n_cus) {
    const uint64_t blocks = ((n_rows + 63u) / 64u + kUtf8Waves - 1u) / kUtf8Waves;
    const uint64_t cap = (uint64_t)(n_cus > 0 ? n_cus : 1) * 16u;
    return (int)(blocks < cap ? blocks : cap);
}

uint32_t utf8_window_bytes() { return kUtf8WindowBytes; }

hipError_t launch_utf8_lengths(const Utf8Args &a, int n_cus, hipStream_t stream) {
    hipLaunchKernelGGL(utf8_lengths_kernel, dim3(utf8_grid(a.n_rows, n_cus)), dim3(kUtf8Waves * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_utf8_fill(const Utf8Args &a, int n_cus, hipStream_t stream) {
    hipLaunchKernelGGL(utf8_fill_kernel, dim3(utf8_grid(a.n_rows, n_cus)), dim3(kUtf8Waves * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_utf8_positions(const Utf8Args &a, int n_cus, hipStream_t stream) {
    hipLaunchKernelGGL(utf8_positions_kernel, dim3(utf8_grid(a.n_rows, n_cus)), dim3(kUtf8Waves * 64), 0, stream, a);
    return hipGetLastError();
}

} // namespace needle
