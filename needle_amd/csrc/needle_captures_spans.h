// needle_captures_spans.h -- the capturing groups of each span of a CSR match list of PACKED rows
// (needle_captures_spans_packed_dev), hand-written for gfx950 (CDNA4).  Included by one translation unit per char
// width (needle_captures_spans1.hip / needle_captures_spans2.hip).
//
// A pure function of (text, span list, pattern): it never sees how the list was made.  For span m, clamped into its row as csr_clamp
// clamps, plane g of the result holds group g of a full match of row[s':e'] (needle_captures.h), or -1 where the pattern does not
// match that text whole.
//
//   Program: the tagged DFA of the pattern (lower_captures, plain LDS program: column maps, table of next state | op list, op lists,
//            fin), staged once per workgroup.
//   Lanes are SPANS, as in set_spans_kernel (needle_set_spans.h), whose skeleton this is: a wave owns a 64-row group at a time
//            (grid-stride), the group's 65 span offsets and 65 row offsets go into the wave's LDS behind the program
//            (needle_csr_rows.h), the wave takes the group's spans 64 at a time, a lane finds its span's row by binary search and
//            clamps the span into it.  Text comes straight from global memory: aligned 16-byte global_* loads of the lane's own span,
//            the next block in flight while the current one is walked, first and last block guarded.
//   Per char: one column lookup, one table lookup; the lane's op list runs only when its id is not 0.  An op is
//            dst slot <- src slot | the position behind the char | -1: an index word, and per op three dependent LDS accesses of the
//            lane.  That, not the text, bounds the kernel (profiles/captures.md).
//   Slots:   the lane's slot file lives in the wave's LDS behind the offsets, lane-interleaved -- slot r of lane l is word r * 64 + l,
//            so the 64 lanes of one access fall into 64 consecutive words: no bank conflict whatever the ops, and no private memory.
//            Nothing is cleared between a lane's rounds but what the initial op list writes: every slot of a live thread was written
//            by that list or by a transition (needle_captures.h).
//   A lane stops in the sink (state 0, whose row leads to itself without ops) or at its span's end; there it copies the slots of
//            fin[state]'s thread to the planes, relative to the row, or writes -1 everywhere.
//   Limit:   a span is walked by ONE lane: a long span runs at one lane's pace.
//   Result:  only m in [span_off[0], span_off[n_rows]) is written; one lane per span, no atomics.
#pragma once
#include "needle_captures.h"
#include "needle_csr_rows.h"
#include "needle_walk.h"

namespace needle {

#define NEEDLE_CAP_GLOBAL __attribute__((address_space(1)))

template <int CW>
__global__ __launch_bounds__(kWavesPerBlock * 64) void captures_spans_kernel(const CapSpansArgs a) {
    constexpr uint32_t CPP = 16 / CW;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_waves = blockDim.x >> 6;

    // ---- stage the program in LDS (once per workgroup)
    for (uint32_t i = tid * 16u; i < a.hdr.lds_bytes; i += blockDim.x * 16u)
        *(u32x4 *)(smem + i) = *(const u32x4 *)(a.prog + i);
    __syncthreads();

    const uint8_t *cmap = smem + a.hdr.off_cmap, *pages = smem + a.hdr.off_pages;
    const uint32_t *table = (const uint32_t *)(smem + a.hdr.off_table), *opidx = (const uint32_t *)(smem + a.hdr.off_opidx),
                   *ops = (const uint32_t *)(smem + a.hdr.off_ops);
    const int32_t *fin = (const int32_t *)(smem + a.hdr.off_fin);
    const uint32_t n_cols = a.hdr.n_cols, G = a.hdr.n_groups;

    // the wave's offsets and slot file, behind the program
    unsigned char *wbase = smem + a.hdr.lds_bytes + (uint32_t)wave * cap_wave_lds(a.hdr.n_slots);
    uint64_t *mo = (uint64_t *)wbase, *ino = mo + 65;
    int32_t *slots = (int32_t *)(wbase + kCapWaveOffsets) + lane; // slot r: slots[r * 64]
    const uint64_t dbase = (uint64_t)(uintptr_t)a.rows;
    const uint64_t n_groups = (a.n_rows + 63u) >> 6;

    uint32_t st = 0;
    auto run_ops = [&](uint32_t id, int32_t pos) __attribute__((always_inline)) {
        const uint32_t ix = opidx[id];
        for (uint32_t i = ix & 0xFFFFFu, e = i + (ix >> 20); i < e; ++i) {
            const uint32_t w = ops[i], src = w >> 16;
            const int32_t v = src == kCapDevPos ? pos : src == kCapDevNone ? -1 : slots[src * 64u];
            slots[(w & 0xFFFFu) * 64u] = v;
        }
    };
    auto step = [&](uint32_t ch, int32_t pos_behind) __attribute__((always_inline)) {
        uint32_t col;
        if constexpr (CW == 1) col = cmap[ch];
        else col = pages[((uint32_t)cmap[ch >> 8] << 8) | (ch & 255u)];
        const uint32_t e = table[st * n_cols + col];
        st = e & 0xFFFFu;
        if (e >> 16) run_ops(e >> 16, pos_behind);
    };
    auto load16 = [](uint64_t at) __attribute__((always_inline)) { return *(const NEEDLE_CAP_GLOBAL u32x4 *)(uintptr_t)at; };
    // the chars p0 .. p0 + CPP - 1 (counted from block 0's first char) of one block; guarded: only those in [skip, rem)
    auto walk_block = [&](const u32x4 c, uint32_t p0, uint32_t rem, uint32_t skip, auto guard) __attribute__((always_inline)) {
        constexpr bool GUARD = decltype(guard)::value;
        const uint32_t wv[4] = {c[0], c[1], c[2], c[3]};
#pragma unroll
        for (uint32_t i = 0; i < CPP; ++i) {
            const uint32_t ch = CW == 1 ? (wv[i >> 2] >> ((i & 3u) * 8u)) & 0xFFu : (wv[i >> 1] >> ((i & 1u) * 16u)) & 0xFFFFu;
            const uint32_t idx = p0 + i;
            if (!GUARD || (idx >= skip && idx < rem)) step(ch, (int32_t)(idx - skip) + 1);
        }
    };

    for (uint64_t grp = (uint64_t)blockIdx.x * (uint64_t)n_waves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * (uint64_t)n_waves) {
        csr_group_offsets(a.span_off, a.offsets, a.n_rows, grp << 6, lane, mo, ino);
        csr_wave_sync();
        const uint64_t m0 = mo[0], m1 = mo[64];
        for (uint64_t mb = m0; mb < m1; mb += 64u) { // (wave-uniform)
            const uint64_t m = mb + (uint64_t)lane;
            const bool own = m < m1;
            uint64_t b0 = 0;            // the span's first aligned 16-byte block
            uint32_t nblk = 0;          // blocks that hold a byte of the span
            uint32_t skip = 0, rem = 0; // chars of block 0 before the span; chars from block 0's first to the span's end
            int32_t s_row = 0, e_row = 0;
            st = 0;
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
                s_row = (int32_t)sc;
                e_row = (int32_t)ec;
                st = a.hdr.start;
                run_ops(a.hdr.init_op, 0);
            }
            u32x4 cur = {0u, 0u, 0u, 0u}, nxt = {0u, 0u, 0u, 0u};
            if (nblk > 0u) { // the first block: guarded
                cur = load16(b0);
                if (nblk > 1u) nxt = load16(b0 + 16u);
                walk_block(cur, 0u, rem, skip, std::true_type());
                cur = nxt;
            }
            uint32_t k = 1; // cur = block k
            while (__ballot(k + 1u < nblk && st != 0u) != 0ull) { // the blocks in between: whole blocks of the span
                if (k + 1u < nblk && st != 0u) {
                    nxt = load16(b0 + (uint64_t)(k + 1u) * 16u); // next block: its latency hides below
                    walk_block(cur, k * CPP, 0u, skip, std::false_type());
                    cur = nxt;
                    ++k;
                }
            }
            if (nblk > 1u && st != 0u) walk_block(cur, (nblk - 1u) * CPP, rem, skip, std::true_type()); // the last block: guarded
            if (own) {
                const int32_t f = fin[st]; // (the sink's is -1)
                a.gstart[m] = f < 0 ? -1 : s_row;
                a.gend[m] = f < 0 ? -1 : e_row;
                const int32_t *th = slots + (uint32_t)(f < 0 ? 0 : f) * 2u * G * 64u;
                for (uint32_t g = 1; g <= G; ++g) {
                    int32_t gs = -1, ge = -1;
                    if (f >= 0) {
                        gs = th[(2u * (g - 1u)) * 64u];
                        ge = th[(2u * (g - 1u) + 1u) * 64u];
                        gs = gs < 0 ? -1 : gs + s_row;
                        ge = ge < 0 ? -1 : ge + s_row;
                    }
                    a.gstart[(uint64_t)g * a.plane_stride + m] = gs;
                    a.gend[(uint64_t)g * a.plane_stride + m] = ge;
                }
            }
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

template <int CW>
static hipError_t launch_captures_spans_cw(const CapSpansArgs &a, int grid, int waves, size_t lds, hipStream_t stream) {
    auto k = captures_spans_kernel<CW>;
    static thread_local uint64_t configured = 0;
    if (hipError_t e = allow_full_lds((const void *)k, configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(waves * 64), lds, stream, a);
    return hipGetLastError();
}

} // namespace needle
