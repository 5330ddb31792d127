// needle_lines.hip -- a packed batch of documents cut at its line terminators into a packed batch of lines, hand-written for gfx950 (CDNA4):
// the kernels of needle_lines_count_packed_dev / needle_lines_fill_packed_dev (include/needle_hip.h).  Pure functions of the
// text: no pattern.  The rule is bytes.splitlines() / String.lines(): '\n', '\r' and "\r\n" end a line, an unterminated tail is a line.
//
//   A workgroup of 256 lanes owns a TILE: kLinesTileBytes of `data` at a fixed place (grid-stride over the tiles), whatever documents lie
//   there.  A tile's units inside the batch's span [offsets[0], offsets[n_rows]) are [lo, hi); the aligned 16-byte blocks that hold them
//   (512, or 513 when `data` is not 16-byte aligned) are the lanes' -- block b is lane b mod 256's: coalesced 16-byte global_* loads, all of
//   a lane's blocks in flight at once.  A block is loaded only when it holds a unit of the span: the one block more that is loaded at
//   times is the one with the lookahead unit `hi` (the first unit of the next tile), and only when hi < offsets[n_rows].
//   Classification is per block on whole units: a mask of '\n' units and one of '\r' units (SWAR compares of the four dwords).  A lane
//   needs the '\n' bit of the unit behind its block: the masks go to LDS, the neighbour's bit 0 comes back from there -- block and tile
//   edges are the same case.  Document boundaries inside (lo, hi] are CUTS behind a unit: the first one comes from a binary search over
//   `offsets` (one lane's, handed over through LDS), then the lanes walk the offsets from there, 256 at a time, and set the bit of the
//   unit in front of each in an LDS bit mask (ds_or).  A unit in front of a cut is its document's last: an event whatever it is.
//       event = '\n'  |  cut behind it  |  ('\r' and no '\n' behind it)           keep = neither '\n' nor '\r'
//   Limit: a run of EMPTY documents is that many offsets at one position, all walked by the one tile that holds the position.
//   The blocks' event and keep counts (16 + 16 bits) get an exclusive prefix sum over the tile in LDS; rank of a unit = the block's prefix
//   plus a popcount below it.  The same table answers the rank queries of d_doc_line_offsets (an offsets walk like the cuts').
//   Count: the two totals, one plain store each.
//   Fill: line_base[t] + rank of an event is its line; the line's end goes to out_off[line + 1]: the unit behind the event (KEEP: a
//   position of the caller's data) or unit_base[t] + the kept units up to it (STRIP).  STRIP: the tile's kept units are ONE contiguous output
//   range, so they are put together in LDS -- at the byte offset the range has in its first aligned 16-byte block -- and written as
//   aligned 16-byte blocks; the first and the last partial block go unit by unit: tiles meet at unit granularity and the batch's ends border
//   the caller's memory.
//   Stores stay inside what the bases name even when the bases are no prefix sums: lines [line_base[t], line_base[t + 1]) within
//   [line_base[0], line_base[tiles]), units [unit_base[t], unit_base[t + 1]) within [unit_base[0], unit_base[tiles]).
//   No workgroup waits on another.  LDS per workgroup: 7200 bytes of tables, and 8208 more of text in the STRIP fill kernel.
#include <hip/hip_runtime.h>
#include <type_traits>

#include "needle_launch.h"
#include "needle_lines.h"

namespace needle {

typedef uint32_t ln_u32x4 __attribute__((ext_vector_type(4)));
// (global_* loads and stores: flat ones would count on the LDS counter too -- needle_replace.hip)
#define LN_GLOBAL __attribute__((address_space(1)))

constexpr uint32_t kLinesBlocks = kLinesLanes * kLinesBlocksPerLane; // 512 blocks of an aligned tile
constexpr uint32_t kLinesSlots = kLinesBlocksPerLane + 1u;           // a lane's blocks: one more for a misaligned tile and the lookahead
constexpr uint32_t kLinesTable = kLinesLanes * kLinesSlots;          // 768 entries of the prefix table (514 used at most)

struct LinesLds {
    uint64_t d0;                            // the tile's first document boundary, from the one lane that searches
    uint32_t pre[kLinesTable];              // block b: events (low 16 bits) and kept units (high 16) of the tile's blocks before it
    uint16_t lf[kLinesTable];               // block b: its '\n' units
    uint16_t ev[kLinesTable];               // block b: its events
    uint32_t cut[(kLinesBlocks + 2u) / 2u]; // 16 bits a block: a document ends behind the unit
    uint32_t wave[kLinesLanes / 64];        // the waves' totals
};

__device__ __forceinline__ uint64_t lines_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t lines_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Bit j: unit j of the aligned block at byte address X lies in the byte range [lo, hi).
template <int CW>
__device__ __forceinline__ uint32_t lines_valid(uint64_t X, uint64_t lo, uint64_t hi) {
    constexpr uint32_t U = 16u / CW;
    const uint32_t a = lo > X ? (lo - X < 16u ? (uint32_t)(lo - X) / CW : U) : 0u;
    const uint32_t b = hi > X ? (hi - X < 16u ? (uint32_t)(hi - X) / CW : U) : 0u;
    return ((1u << b) - 1u) & ~((1u << a) - 1u);
}

// Bit j: unit j of the block is the code unit c (c < 0x80), compared as a whole unit.
template <int CW>
__device__ __forceinline__ uint32_t lines_eq(const ln_u32x4 v, uint32_t c) {
    uint32_t m = 0;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if (CW == 1) {
            const uint32_t x = v[d] ^ (c * 0x01010101u);
            const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u; // 0x80 in every byte that is zero, exactly
            m |= ((((z >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * d);
        } else {
            const uint32_t x = v[d] ^ (c * 0x00010001u);
            const uint32_t z = ~(((x & 0x7FFF7FFFu) + 0x7FFF7FFFu) | x) & 0x80008000u;
            m |= (((z >> 15) & 1u) | ((z >> 30) & 2u)) << (2 * d);
        }
    }
    return m;
}

// The first d in [0, n] with off[d] > x; n + 1 when there is none.
__device__ __forceinline__ uint64_t lines_first_above(const uint64_t *off, uint64_t n, uint64_t x) {
    uint64_t a = 0, b = n + 1u;
    while (a < b) {
        const uint64_t m = a + ((b - a) >> 1);
        if (off[m] > x) b = m;
        else a = m + 1u;
    }
    return a;
}

// What a workgroup knows of its tile.
struct LinesTile {
    uint64_t loB, hiB; // the tile's units inside the span, as absolute byte addresses
    uint64_t A0;       // the aligned block that holds loB
    uint32_t nblk;     // blocks that hold a unit of [loB, hiB)
    uint64_t d0;       // the first document boundary above lo (lines_classify fills it in)
    uint64_t lo, hi;   // loB and hiB as units of data
};

// Classify the tile: this lane's blocks' events and kept units (and the blocks themselves), the tile's table in LDS, t.d0, the totals
// (events low, kept units high) returned.  Called by all 256 lanes.
template <int CW>
__device__ __forceinline__ uint32_t lines_classify(const LinesArgs &a, LinesLds &s, LinesTile &t, uint64_t S1B, ln_u32x4 (&blk)[kLinesSlots],
                                                   uint32_t (&ev)[kLinesSlots], uint32_t (&keep)[kLinesSlots]) {
    constexpr uint32_t U = 16u / CW;
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.data;
    const uint64_t hi2B = lines_min(t.hiB + CW, S1B);                  // ... and the lookahead unit, if the span has one
    const uint32_t nblk2 = (uint32_t)((hi2B - t.A0 + 15u) >> 4);       // nblk or nblk + 1
    uint32_t lf[kLinesSlots], cr[kLinesSlots];
#pragma unroll
    for (uint32_t k = 0; k < kLinesSlots; ++k) {
        const uint32_t b = tid + k * kLinesLanes;
        const ln_u32x4 zero = {0u, 0u, 0u, 0u};
        blk[k] = zero;
        if (b < nblk2) blk[k] = *(const LN_GLOBAL ln_u32x4 *)(uintptr_t)(t.A0 + (uint64_t)b * 16u);
    }
    for (uint32_t w = tid; w < (kLinesBlocks + 2u) / 2u; w += kLinesLanes) s.cut[w] = 0u;
    if (tid == 0) s.d0 = lines_first_above(a.in_off, a.n_rows, t.lo); // (one lane's dependent loads, behind the blocks' loads)
    __syncthreads();
    t.d0 = s.d0;
    // the cuts: document boundaries in (lo, hi], the bit of the unit in front
    for (uint64_t d = t.d0 + tid; d <= a.n_rows; d += kLinesLanes) {
        const uint64_t o = a.in_off[d];
        if (o > t.hi) break;
        const uint64_t at = dbase + o * CW - CW;
        if (at >= t.loB && at < t.hiB) {
            const uint32_t q = (uint32_t)(at - t.A0) / CW; // the unit's place among the tile's blocks' units
            atomicOr(&s.cut[q >> 5], 1u << (q & 31u));
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < kLinesSlots; ++k) {
        const uint32_t b = tid + k * kLinesLanes;
        const uint32_t ok = b < nblk2 ? lines_valid<CW>(t.A0 + (uint64_t)b * 16u, t.loB, hi2B) : 0u;
        lf[k] = lines_eq<CW>(blk[k], 0x0Au) & ok;
        cr[k] = lines_eq<CW>(blk[k], 0x0Du) & ok;
        s.lf[b] = (uint16_t)lf[k];
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLinesSlots; ++k) {
        const uint32_t b = tid + k * kLinesLanes;
        ev[k] = 0u, keep[k] = 0u;
        if (b < t.nblk) {
            const uint32_t own = lines_valid<CW>(t.A0 + (uint64_t)b * 16u, t.loB, t.hiB);
            const uint32_t behind = b + 1u < nblk2 ? (uint32_t)s.lf[b + 1u] & 1u : 0u;
            const uint32_t lf_next = (lf[k] >> 1) | (behind << (U - 1u));
            const uint32_t cut = CW == 1 ? (s.cut[b >> 1] >> ((b & 1u) * 16u)) & 0xFFFFu : (s.cut[b >> 2] >> ((b & 3u) * 8u)) & 0xFFu;
            ev[k] = (lf[k] | cut | (cr[k] & ~lf_next)) & own;
            keep[k] = own & ~(lf[k] | cr[k]);
        }
        s.ev[b] = (uint16_t)ev[k];
        s.pre[b] = (uint32_t)__popc(ev[k]) | ((uint32_t)__popc(keep[k]) << 16);
    }
    __syncthreads();
    // the exclusive prefix sum of the table: a lane takes kLinesSlots consecutive entries, the waves meet in LDS
    uint32_t c[kLinesSlots], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLinesSlots; ++k) {
        c[k] = s.pre[tid * kLinesSlots + k];
        mine += c[k];
    }
    uint32_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s.wave[tid >> 6] = incl;
    __syncthreads();
    uint32_t excl = incl - mine, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kLinesLanes / 64; ++w) {
        if (w < (tid >> 6)) excl += s.wave[w];
        total += s.wave[w];
    }
#pragma unroll
    for (uint32_t k = 0; k < kLinesSlots; ++k) {
        s.pre[tid * kLinesSlots + k] = excl;
        excl += c[k];
    }
    __syncthreads();
    return total;
}

// The tile's place: false when it holds no unit of the span [S0, S1) (units of data).
template <int CW>
__device__ __forceinline__ bool lines_tile(const LinesArgs &a, uint64_t tile, uint64_t S0, uint64_t S1, LinesTile *t) {
    constexpr uint64_t T = kLinesTileBytes / CW;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.data;
    const uint64_t lo = lines_max(tile * T, S0), hi = lines_min(tile * T + T, S1);
    if (lo >= hi) return false;
    t->loB = dbase + lo * CW, t->hiB = dbase + hi * CW;
    t->A0 = t->loB & ~(uint64_t)15;
    t->nblk = (uint32_t)((t->hiB - t->A0 + 15u) >> 4);
    t->lo = lo, t->hi = hi;
    t->d0 = 0;
    return true;
}

template <int CW>
__global__ __launch_bounds__(kLinesLanes) void lines_count_kernel(const LinesArgs a) {
    __shared__ LinesLds s;
    const uint64_t S0 = lines_min(a.in_off[0], a.data_units), S1 = lines_min(lines_max(a.in_off[a.n_rows], S0), a.data_units);
    const uint64_t S1B = (uint64_t)(uintptr_t)a.data + S1 * CW;
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        LinesTile t;
        uint32_t total = 0;
        if (lines_tile<CW>(a, tile, S0, S1, &t)) { // (workgroup-uniform)
            ln_u32x4 blk[kLinesSlots];
            uint32_t ev[kLinesSlots], keep[kLinesSlots];
            total = lines_classify<CW>(a, s, t, S1B, blk, ev, keep);
        }
        if (threadIdx.x == 0) {
            a.tile_lines[tile] = total & 0xFFFFu;
            if (a.tile_units) a.tile_units[tile] = total >> 16;
        }
    }
}

template <int CW, bool KEEP>
__global__ __launch_bounds__(kLinesLanes) void lines_fill_kernel(const LinesArgs a) {
    using Unit = std::conditional_t<CW == 1, uint8_t, uint16_t>;
    constexpr uint64_t T = kLinesTileBytes / CW;
    constexpr uint32_t U = 16u / CW;
    __shared__ LinesLds s;
    __shared__ __attribute__((aligned(16))) uint8_t s_text[KEEP ? 16 : kLinesTileBytes + 16u]; // STRIP: the tile's kept units
    const uint32_t tid = threadIdx.x;
    const uint64_t n = a.n_rows, dbase = (uint64_t)(uintptr_t)a.data, obase = (uint64_t)(uintptr_t)a.out;
    const uint64_t S0 = lines_min(a.in_off[0], a.data_units), S1 = lines_min(lines_max(a.in_off[n], S0), a.data_units);
    const uint64_t S1B = dbase + S1 * CW;
    const uint64_t L0 = a.line_base[0], L1 = lines_max(a.line_base[a.tiles], L0);
    uint64_t U0 = 0, U1 = 0;
    if (!KEEP) U0 = a.unit_base[0], U1 = lines_max(a.unit_base[a.tiles], U0);
    const uint64_t home = lines_min(S0 / T, a.tiles - 1u); // the tile that answers for what lies at the span's start
    for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
        if (tile == 0 && tid == 0) a.out_off[L0] = KEEP ? a.in_off[0] : U0;
        if (tile == home && a.doc_lines) // document 0 and the empty documents behind it: no line in front of them
            for (uint64_t d = tid; d <= n && a.in_off[d] <= S0; d += kLinesLanes) a.doc_lines[d] = L0;
        LinesTile t;
        if (!lines_tile<CW>(a, tile, S0, S1, &t)) continue; // (workgroup-uniform)
        ln_u32x4 blk[kLinesSlots];
        uint32_t ev[kLinesSlots], keep[kLinesSlots];
        const uint32_t total = lines_classify<CW>(a, s, t, S1B, blk, ev, keep);
        // this tile's lines and units, inside the batch's
        const uint64_t lb = a.line_base[tile], line_lo = lines_max(lb, L0), line_hi = lines_min(a.line_base[tile + 1u], L1);
        uint64_t ub = 0, unit_lo = 0, unit_hi = 0;
        uint32_t shift = 0;
        if (!KEEP) {
            ub = a.unit_base[tile];
            const uint64_t own_end = ub + (uint64_t)(total >> 16);
            unit_lo = lines_max(ub, U0), unit_hi = lines_min(lines_min(a.unit_base[tile + 1u], U1), own_end >= ub ? own_end : 0u);
            shift = (uint32_t)(obase + ub * CW) & 15u;
        }
#pragma unroll
        for (uint32_t k = 0; k < kLinesSlots; ++k) {
            const uint32_t b = tid + k * kLinesLanes;
            if (b >= t.nblk) continue;
            const uint32_t pre = s.pre[b], pe = pre & 0xFFFFu, pk = pre >> 16;
            for (uint32_t m = ev[k]; m; m &= m - 1u) { // the block's events: usually none, rarely more than one
                const uint32_t j = (uint32_t)__builtin_ctz(m);
                const uint64_t line = lb + (uint64_t)(pe + (uint32_t)__popc(ev[k] & ((1u << j) - 1u)));
                // (the event's own address, not its block's: the first block may begin in front of `data`)
                const uint64_t end = KEEP ? (t.A0 + (uint64_t)b * 16u + j * CW - dbase) / CW + 1u : ub + (uint64_t)(pk + (uint32_t)__popc(keep[k] & ((2u << j) - 1u)));
                if (line >= line_lo && line < line_hi) a.out_off[line + 1u] = end;
            }
            if (!KEEP) {
                uint32_t at = shift + pk * CW; // the byte of s_text the block's first kept unit goes to
#pragma unroll
                for (uint32_t d = 0; d < 4; ++d) {
                    constexpr uint32_t per = U / 4u, all = (1u << per) - 1u;
                    const uint32_t kd = (keep[k] >> (d * per)) & all;
                    if (kd == all && (at & 3u) == 0u) { // a whole dword to an aligned place
                        *(uint32_t *)(s_text + at) = blk[k][d];
                        at += 4u;
                    } else {
#pragma unroll
                        for (uint32_t j = 0; j < per; ++j)
                            if ((kd >> j) & 1u) {
                                *(Unit *)(s_text + at) = (Unit)(blk[k][d] >> (j * 8u * CW));
                                at += CW;
                            }
                    }
                }
            }
        }
        if (a.doc_lines) // the documents that begin in (lo, hi]: the lines up to the unit in front of them
            for (uint64_t d = t.d0 + tid; d <= n; d += kLinesLanes) {
                const uint64_t o = a.in_off[d];
                if (o > t.hi) break;
                const uint64_t at = dbase + o * CW - CW;
                if (at >= t.loB && at < t.hiB) {
                    const uint32_t b = (uint32_t)(at - t.A0) >> 4, j = ((uint32_t)(at - t.A0) & 15u) / CW;
                    a.doc_lines[d] = lb + (uint64_t)((s.pre[b] & 0xFFFFu) + (uint32_t)__popc((uint32_t)s.ev[b] & ((2u << j) - 1u)));
                }
            }
        if (!KEEP) {
            __syncthreads();
            if (unit_lo < unit_hi) {
                const uint64_t oB = obase + unit_lo * CW, oE = obase + unit_hi * CW;
                const uint64_t base16 = (obase + ub * CW) & ~(uint64_t)15; // s_text[0] is this address
                for (uint64_t X = (oB & ~(uint64_t)15) + (uint64_t)tid * 16u; X < oE; X += (uint64_t)kLinesLanes * 16u) {
                    const uint32_t off = (uint32_t)(X - base16);
                    if (X >= oB && X + 16u <= oE) { // the tile's own 16 bytes: one store
                        *(LN_GLOBAL ln_u32x4 *)(uintptr_t)X = *(const ln_u32x4 *)(s_text + off);
                    } else { // an edge of the tile's range, shared with another tile or with the caller's memory: the own units only
#pragma unroll
                        for (uint32_t x = 0; x < 16u; x += CW)
                            if (X + x >= oB && X + x < oE) *(LN_GLOBAL Unit *)(uintptr_t)(X + x) = *(const Unit *)(s_text + off + x);
                    }
                }
            }
        }
        __syncthreads(); // (the next tile overwrites the tables and the text)
    }
}

static int lines_grid(uint64_t tiles, int n_cus) {
    const uint64_t cap = (uint64_t)(n_cus > 0 ? n_cus : 1) * 8u;
    return (int)(tiles < cap ? tiles : cap);
}

uint32_t lines_tile_units(uint32_t char_width) { return char_width == 1 || char_width == 2 ? kLinesTileBytes / char_width : 0u; }

hipError_t launch_lines_count(const LinesArgs &a, int n_cus, hipStream_t stream) {
    const dim3 grid(lines_grid(a.tiles, n_cus)), block(kLinesLanes);
    if (a.cw == 1) hipLaunchKernelGGL(lines_count_kernel<1>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(lines_count_kernel<2>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_lines_fill(const LinesArgs &a, bool keep_ends, int n_cus, hipStream_t stream) {
    const dim3 grid(lines_grid(a.tiles, n_cus)), block(kLinesLanes);
    if (a.cw == 1 && keep_ends) hipLaunchKernelGGL((lines_fill_kernel<1, true>), grid, block, 0, stream, a);
    else if (a.cw == 1) hipLaunchKernelGGL((lines_fill_kernel<1, false>), grid, block, 0, stream, a);
    else if (keep_ends) hipLaunchKernelGGL((lines_fill_kernel<2, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((lines_fill_kernel<2, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace needle
