// needle_set_spans.h -- which members of a pattern set match each span of a CSR match list of PACKED rows
// (needle_set_matches_spans_packed_dev), hand-written for gfx950 (CDNA4).  Included by one translation unit per char
// width (needle_set_spans1.hip / needle_set_spans2.hip).
//
// A pure function of (text, span list, set): it never sees how the list was made.  Bit i of masks[m] is Matcher.matches() of member i
// on row[start[m]:end[m]] -- what needle_set_matches_packed_dev stores for a row holding that text.
//
//   Program: the OP_MATCHES program of the set's group (lower_pattern_set, plain LDS table), staged once per workgroup as
//            packed_set_kernel stages it; the same Walk constants, the same walk_piece<OP_MATCHES> per 16-byte block, mask[st] read
//            from LDS ONCE at the span's end.
//   Lanes are SPANS, not rows.  A wave owns a 64-row group at a time (grid-stride, as replace_lengths_kernel): the group's 65 span
//            offsets and 65 row offsets go into the wave's LDS behind the program, the wave takes the group's spans m0 + lane,
//            m0 + lane + 64, ..; a lane finds its span's row by a 6-step binary search, clamps the span into the row
//            (s' = clamp(s, 0, len), e' = clamp(e, s', len): the result of a malformed span is DEFINED) and turns it into absolute byte
//            addresses [as, ae).  Spans need not be monotone or disjoint.  A group without spans costs its offsets and nothing else.
//   Text comes straight from global memory, not through the packed_stream window: a match list covers a small, scattered share of the
//            text (4 of 256 bytes per row in the sparse keyword workload) and streaming every line of every row would read the whole
//            batch again.  A lane loads the aligned 16-byte blocks of its own span -- an aligned block is loaded only when it holds a
//            byte of the span (the packed kernels' rule; the other bytes of the first and last block are masked out by skip / rem) --
//            with global_* loads (a flat load would count on the LDS counter too), the next block before the current one is walked.
//            First and last block are guarded, the ones in between are not.  Neighbouring lanes hold neighbouring spans, so a wave's
//            loads fall into few lines.  A lane stops in the sink (st == 0) or at its span's end; the wave goes on to its next 64
//            spans when all lanes have stopped.
//   Limit:   a span is walked by ONE lane: a long span runs at one lane's pace (16 bytes per round trip to memory in flight).
//   Result:  masks[m] = bits (the set's first group) or masks[m] |= bits (later groups: launches are stream-ordered): one lane per
//            span, no atomics.  Only m in [span_off[0], span_off[n_rows]) is written.
//
// The wave's hand-over, the group's offsets in LDS, the row search and the clamp are needle_csr_rows.h's, shared with needle_replace.hip.
#pragma once
#include "needle_csr_rows.h"
#include "needle_walk.h"

namespace needle {

#define NEEDLE_SS_GLOBAL __attribute__((address_space(1)))

template <int CW, int MODE>
__global__ __launch_bounds__(kWavesPerBlock * 64) void set_spans_kernel(const SetSpansArgs a) {
    static_assert(MODE == MODE_TABLE8 || MODE == MODE_TABLE16, "plain table programs only");
    constexpr uint32_t CPP = 16 / CW;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_waves = blockDim.x >> 6;

    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();
    // ---- stage the automaton (column maps, table, masks) in LDS (once per workgroup)
    for (uint32_t i = tid * 16u; i < a.hdr.lds_bytes; i += blockDim.x * 16u)
        *(u32x4 *)(smem + i) = *(const u32x4 *)(a.prog + i);
    __syncthreads();

    // ---- walk constants of a plain table program (no window addressing, compact page map): packed_set_kernel's
    Walk wk;
    constexpr uint32_t ELEM = MODE == MODE_TABLE16 ? 2u : 1u;
    wk.ncols_e = a.hdr.n_cols * ELEM;
    wk.pad_e = a.hdr.pad_col * ELEM;
    wk.pre_e = (a.hdr.pad_col + 1u) * ELEM;
    wk.pad_b = wk.pre_b = 0;
    wk.win_on = 0;
    wk.win_lo = wk.win_hi = 0;
    wk.dead_hi = 0;
    wk.sp_chains = wk.sp_pad_ident = 0;
    wk.flat = 0;
    wk.table_off = a.hdr.off_table;
    wk.lane4 = (uint32_t)(lane & 31) * 4u;
    wk.gtable = nullptr;
    wk.hot_last = 0;
    const uint32_t accept_lo = a.hdr.accept_lo, start_state = a.hdr.start, mask_off = a.hdr.ft_codes_off;

    // the wave's offsets, behind the program
    uint64_t *mo = (uint64_t *)(smem + ((a.hdr.lds_bytes + 15u) & ~15u) + (uint32_t)wave * kSetSpansWaveLds), *ino = mo + 65;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.rows;
    const uint64_t n_groups = (a.n_rows + 63u) >> 6;

    auto load16 = [](uint64_t at) __attribute__((always_inline)) { return *(const NEEDLE_SS_GLOBAL u32x4 *)(uintptr_t)at; };
    auto walk_block = [&](const u32x4 c, uint32_t p0, uint32_t rem, uint32_t skip, uint32_t &st, auto guard) __attribute__((always_inline)) {
        constexpr bool G = decltype(guard)::value;
        const uint32_t wv[4] = {c[0], c[1], c[2], c[3]};
        int32_t unused = -1;
        walk_piece<OP_MATCHES, CW, MODE, G>(wk, wv, p0, G ? rem : 0u, G ? skip : 0u, accept_lo, st, unused);
    };

    for (uint64_t grp = (uint64_t)blockIdx.x * (uint64_t)n_waves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * (uint64_t)n_waves) {
        csr_group_offsets(a.span_off, a.offsets, a.n_rows, grp << 6, lane, mo, ino);
        csr_wave_sync();
        const uint64_t m0 = mo[0], m1 = mo[64];
        for (uint64_t mb = m0; mb < m1; mb += 64u) { // (wave-uniform)
            const uint64_t m = mb + (uint64_t)lane;
            const bool own = m < m1;
            uint64_t b0 = 0;      // the span's first aligned 16-byte block
            uint32_t nblk = 0;    // blocks that hold a byte of the span
            uint32_t skip = 0, rem = 0; // chars of block 0 before the span; chars from block 0's first to the span's end
            if (own) {
                const uint32_t r = csr_row_of(mo, m);
                const uint64_t row = ino[r];
                uint64_t sc, ec;
                csr_clamp(a.start[m], a.end[m], ino[r + 1] - row, &sc, &ec);
                const uint64_t as = dbase + (row + sc) * CW, ae = dbase + (row + ec) * CW;
                b0 = as & ~(uint64_t)15;
                skip = (uint32_t)(as & 15u) / CW;
                rem = skip + (uint32_t)(ec - sc); // (positions are int32: no overflow)
                nblk = ae > as ? (uint32_t)((ae - b0 + 15u) >> 4) : 0u;
            }
            uint32_t st = start_state;
            u32x4 cur = {0u, 0u, 0u, 0u}, nxt = {0u, 0u, 0u, 0u};
            if (nblk > 0u) { // the first block: guarded
                cur = load16(b0);
                if (nblk > 1u) nxt = load16(b0 + 16u);
                walk_block(cur, 0u, rem, skip, st, std::true_type());
                cur = nxt;
            }
            uint32_t k = 1; // cur = block k
            while (__ballot(k + 1u < nblk && st != 0u) != 0ull) { // the blocks in between: whole blocks of the span
                if (k + 1u < nblk && st != 0u) {
                    nxt = load16(b0 + (uint64_t)(k + 1u) * 16u); // next block: its latency hides below
                    walk_block(cur, k * CPP, 0u, 0u, st, std::false_type());
                    cur = nxt;
                    ++k;
                }
            }
            if (nblk > 1u && st != 0u) walk_block(cur, (nblk - 1u) * CPP, rem, skip, st, std::true_type()); // the last block: guarded
            if (own) {
                uint32_t bits = lds_u32(mask_off + st * 4u); // (the sink's mask is 0)
                if (!a.store) bits |= a.masks[m];
                a.masks[m] = bits;
            }
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

template <int CW>
static hipError_t launch_set_spans_cw(const SetSpansArgs &a, int grid, int waves, size_t lds, hipStream_t stream) {
    const uint32_t mode = a.hdr.mode;
    if (mode == MODE_TABLE8) {
        auto k = set_spans_kernel<CW, MODE_TABLE8>;
        static thread_local uint64_t configured = 0;
        if (hipError_t e = allow_full_lds((const void *)k, configured); e != hipSuccess) return e;
        hipLaunchKernelGGL(k, dim3(grid), dim3(waves * 64), lds, stream, a);
        return hipGetLastError();
    }
    if (mode == MODE_TABLE16) {
        auto k = set_spans_kernel<CW, MODE_TABLE16>;
        static thread_local uint64_t configured = 0;
        if (hipError_t e = allow_full_lds((const void *)k, configured); e != hipSuccess) return e;
        hipLaunchKernelGGL(k, dim3(grid), dim3(waves * 64), lds, stream, a);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

} // namespace needle
