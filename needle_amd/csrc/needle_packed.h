// needle_packed.h -- the scan kernel of PACKED row batches (needle_packed_view: one buffer of code units + offsets[n + 1]),
// hand-written for gfx950 (CDNA4), and its launch templates.  Included by one translation unit per reference loop
// (needle_packed_*.hip), which compile in parallel.
//
// The fixed-stride kernels (needle_scan.h) read every row as whole 128-byte lines at its stride: for a packed batch that
// needs a conversion first (needle_rows_from_packed_dev: the text read once, up to 2-4x as many padded bytes written and read
// back).  This kernel reads the packed text itself, every byte once:
//
//   Rows to waves.  A wave owns 64 consecutive rows ("group", persistent over groups as scan_kernel).  Their text is ONE
//   contiguous span [offsets[64g], offsets[64g + 64]); lane l reads its row's two offsets (coalesced), the span's ends come
//   from lanes 0 and 63.
//   Staging.  The span is streamed through the wave's LDS window (the tile scan_kernel would use: 64 x CHB bytes, i.e.
//   4 or 8 KiB next to the automaton) by lane-linear 16-byte `nt` loads -- load j of lane l reads window byte (64 j + l) * 16,
//   whole 128-byte lines, window bases 128-byte aligned.  The NEXT window (of this group, or the next group's first one) is
//   loaded into VGPRs while the current one is walked.
//   Walk.  Each lane walks the resident 16-byte blocks of its own row out of the window with the per-char code of the tiled
//   scan (walk_piece, needle_walk.h).  A row starts and ends at arbitrary code units: its first and last block of a window
//   are walked GUARDED -- chars before the row's start take the PRE column (identity: the find() cursor's mechanism), chars
//   at or after its end the PAD column -- the blocks in between unguarded.  Positions count from the row's first char
//   rounded down to its 16-byte block ("origin"), so that the guards are the plain skip / rem of walk_piece.  The automaton
//   state and find()'s lastMatch carry across windows in registers.
//   Early exit / skipping.  After each window the next one starts at the first byte still wanted: the lowest row that is
//   neither resolved (sink, accepted for containedIn, a dead find() state) nor finished.  Offsets are non-decreasing, so
//   that is the lowest such LANE's row.  A group whose rows all have their verdict stops reading its span; text of resolved
//   rows between live ones is skipped a window at a time.
//   find() variants (template argument EXT, instantiated in translation units of their own so that the plain kernels keep their
//   registers): per-row cursors (PK_CURSOR, ScanArgs::from, needle_find_next_packed_dev: the walk starts at the cursor's char,
//   the origin and so the positions stay the row's; 64-byte windows for most 8-bit programs: packed_cursor_narrow), and the result as one dword / uint16 per row with
//   an escape for matches the form cannot hold (PK_FORMS, ScanArgs::packed / packed8, PackedArgs::overflow:
//   needle_find_packed{16,8}_packed_dev).
//   Long rows are correct at one lane's pace (every window of such a row is walked by its one lane).  Intra-row parallelism
//   for few huge rows stays with the stripe paths of the fixed-stride entries (needle_rows_from_packed_dev first).
//
// Memory safety: a 16-byte block is loaded only when it holds a byte of the group's span [first row's start, last row's
// end) -- inside [data + offsets[0] * cw, data + offsets[n] * cw) -- so nothing past the batch's last byte is read, whatever
// the padding of its allocation (the view only promises 4 bytes); blocks are aligned in ABSOLUTE addresses (the data pointer
// itself is only 4-byte aligned), so a block around a valid byte stays inside that byte's page.  Bytes of neighbouring rows
// reach a lane's lookups only as PRE / PAD chars.
//
// The loops restated (reference: DFAClassBuilder.java): matches() :892-910, containedIn() :1004-1022, find() :629-657 with
// indexForwards() :438-468 and indexBackwards() :565-583 -- exactly as scan_kernel's guarded (ragged-row) form.
#pragma once
#include "needle_walk.h"

namespace needle {

// ------------------------------------------------------------------------------------------------
// The staging shared by the packed-rows kernels (packed_kernel below, packed_find_all_kernel in needle_packed_find_all.h)
// ------------------------------------------------------------------------------------------------
// A wave's LDS window: 64 slots of CHB bytes, slot_stride apart (the tile scan_kernel's wave would use).  in_f_rows: the first
// four waves' slots lie in the upper 128 B of F rows wave*64 .. wave*64+63 (scan programs only; 0 for every other program).
template <int CHB>
struct PackedWindow {
    uint32_t base, slot_stride;
    __device__ __forceinline__ PackedWindow(uint32_t prog_lds_bytes, uint32_t in_f_rows, int wave) {
        if (in_f_rows && wave < 4) {
            base = kLdsF1 + (uint32_t)wave * 64u * 256u + 128u;
            slot_stride = 256u;
        } else {
            const uint32_t first = in_f_rows ? 4u : 0u;
            base = ((prog_lds_bytes + 15u) & ~15u) + ((uint32_t)wave - first) * (64u * CHB);
            slot_stride = CHB;
        }
    }
    // LDS address of window byte bo (a 16-byte block never straddles slots)
    __device__ __forceinline__ uint32_t at(uint32_t bo) const { return base + (bo / CHB) * slot_stride + (bo % CHB); }
};

__device__ __forceinline__ uint64_t packed_lane_u64(uint64_t v, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return (uint64_t)hi << 32 | lo;
}

// Streams every group of this wave (persistent: groups wave, wave + wave_cnt, ...) through its window.  Per group, with rs / re =
// the lane's row as absolute byte addresses [rs, re) (rows past n_rows: empty, at the batch's end):
//   begin_group(grp)   the lane's per-row state
//   walk_window(w)     the window at absolute address w (128-byte aligned, kWin bytes) is in LDS: walk the lane's part of it
//   unresolved()       the lane's row still wants text (a row also stops wanting it at its end)
//   wanted_from()      the first byte of its row the lane still wants (rs, or where a find() cursor starts the walk)
//   finish_rows(grp)   the group's results
template <int CW, int CHB, class BeginGroup, class WalkWindow, class Unresolved, class WantedFrom, class FinishRows>
__device__ __forceinline__ void packed_stream(int lane, int wave, int n_waves, const uint8_t *rows, const uint64_t *offsets, uint64_t n_rows,
                                              const PackedWindow<CHB> &win, uint64_t &rs, uint64_t &re, BeginGroup &&begin_group, WalkWindow &&walk_window,
                                              Unresolved &&unresolved, WantedFrom &&wanted_from, FinishRows &&finish_rows) {
    constexpr uint32_t kWin = 64u * CHB;      // window bytes per wave
    constexpr int kLoads = CHB / 16;          // 16-byte loads per lane per window
    const uint64_t n_groups = (n_rows + 63) >> 6;
    const uint64_t wave_cnt = (uint64_t)gridDim.x * n_waves;
    uint64_t g = (uint64_t)blockIdx.x * n_waves + wave;
    if (g >= n_groups) return;
    const uint64_t data = (uint64_t)(uintptr_t)rows;

    auto row_bounds = [&](uint64_t grp, uint64_t &b0, uint64_t &b1) __attribute__((always_inline)) {
        const uint64_t r = (grp << 6) + (uint64_t)lane;
        const uint64_t i0 = r < n_rows ? r : n_rows;
        const uint64_t i1 = r + 1 < n_rows ? r + 1 : n_rows;
        b0 = data + offsets[i0] * CW;
        b1 = data + offsets[i1] * CW;
    };

    u32x4 R[kLoads];
    // Load the window at absolute address w (128-byte aligned) into R: only the 16-byte blocks inside [lo16, hi) -- lo16 = the
    // span's first byte rounded down to its block -- the rest are zero and never reach a lane's automaton.
    auto fetch = [&](uint64_t w, uint64_t lo16, uint64_t hi) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            const uint64_t b = w + (uint64_t)((j * 64 + lane) * 16);
            u32x4 v = {0, 0, 0, 0};
            if (b >= lo16 && b < hi) v = load_row16<true>((const uint8_t *)(uintptr_t)b);
            R[j] = v;
        }
    };
    // Store the window held in R to LDS; with do_fetch, re-issue each register's load for the window at w right behind its
    // store (as scan_kernel's stage_and_fetch: one window's registers live, loads in flight while the window is walked).
    auto stage_and_fetch = [&](bool do_fetch, uint64_t w, uint64_t lo16, uint64_t hi) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < kLoads; ++j) {
            *(lds_u32x4 *)(uintptr_t)win.at((uint32_t)((j * 64 + lane) * 16)) = R[j];
            asm volatile("" ::: "memory"); // keep store j ahead of load j
            if (do_fetch) {
                const uint64_t b = w + (uint64_t)((j * 64 + lane) * 16);
                u32x4 v = {0, 0, 0, 0};
                if (b >= lo16 && b < hi) v = load_row16<true>((const uint8_t *)(uintptr_t)b);
                R[j] = v;
            }
            asm volatile("" ::: "memory");
        }
    };

    uint64_t span_lo, span_hi;
    uint64_t nrs = 0, nre = 0; // the next group's rows (loaded while this group is walked)
    row_bounds(g, rs, re);
    span_lo = packed_lane_u64(rs, 0);
    span_hi = packed_lane_u64(re, 63);
    begin_group(g);
    bool have = false; // R holds (or has in flight) the current group's first window
    for (;;) {
        const uint64_t ng = g + wave_cnt;
        const bool has_next = ng < n_groups;
        if (has_next) row_bounds(ng, nrs, nre); // (in flight while this group is walked)
        bool pf_next = false;                   // the last prefetch was the next group's first window
        if (span_lo < span_hi) {
            uint64_t w = span_lo & ~(uint64_t)127;
            const uint64_t lo16 = span_lo & ~(uint64_t)15;
            if (!have) fetch(w, lo16, span_hi);
            for (;;) {
                const uint64_t wn = w + kWin;
                const bool same = wn < span_hi; // wave-uniform
                // prefetch target: this group's next window, else the next group's first one
                uint64_t pw = wn, plo = lo16, phi = span_hi;
                if (!same && has_next) {
                    const uint64_t nlo = packed_lane_u64(nrs, 0);
                    phi = packed_lane_u64(nre, 63);
                    pw = nlo & ~(uint64_t)127;
                    plo = nlo & ~(uint64_t)15;
                    pf_next = true; // (an empty next span: nothing to load, the predicate below is false everywhere)
                }
                stage_and_fetch(same || has_next, pw, plo, phi);
                asm volatile("" ::: "memory"); // keep the prefetch issued ahead of the walk
                walk_window(w);
                const uint64_t live = __ballot(unresolved() && re > wn);
                if (live == 0ull) break;
                // the next window starts at the first byte some unresolved row still needs: the lowest live lane's
                const uint64_t rl = packed_lane_u64(wanted_from(), __builtin_ctzll(live));
                const uint64_t nxt = (rl > wn ? rl : wn) & ~(uint64_t)127;
                if (nxt != wn) fetch(nxt, lo16, span_hi); // (skipped text of resolved rows)
                w = nxt;
            }
        }
        finish_rows(g);
        if (!has_next) break;
        g = ng;
        rs = nrs;
        re = nre;
        span_lo = packed_lane_u64(rs, 0);
        span_hi = packed_lane_u64(re, 63);
        begin_group(g);
        have = pf_next;
    }
}

// find() variants (EXT): the plain int32 pairs (PK_PLAIN, needle_find_packed_dev and matches / containedIn), per-row cursors with
// int32 pairs (PK_CURSOR, needle_find_next_packed_dev), one dword / uint16 per row with escapes (PK_FORMS,
// needle_find_packed{16,8}_packed_dev).  Instantiated apart (needle_packed_next*.hip, needle_packed_forms*.hip), so that the
// plain kernels carry none of the others' registers.
constexpr int PK_PLAIN = 0, PK_CURSOR = 1, PK_FORMS = 2;

template <int OP, int CW, int MODE, int CHB, bool LEN, int EXT = PK_PLAIN>
__global__ __launch_bounds__(kWavesPerBlock * 64) void packed_kernel(const PackedArgs pa) {
    const ScanArgs &a = pa.s;
    constexpr uint32_t kWin = 64u * CHB;      // window bytes per wave
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_waves = blockDim.x >> 6;

    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();
    // ---- stage the automaton in LDS (once per workgroup)
    for (uint32_t i = tid * 16u; i < a.hdr.lds_bytes; i += blockDim.x * 16u)
        *(u32x4 *)(smem + i) = *(const u32x4 *)(a.prog + i);
    __syncthreads();

    // ---- walk constants: as scan_kernel sets them up
    Walk wk;
    constexpr uint32_t ELEM = (MODE == MODE_TABLE16 || MODE == MODE_HYBRID) ? 2u : 1u;
    wk.ncols_e = a.hdr.n_cols * ELEM;
    wk.pad_e = (MODE == MODE_PACK) ? a.hdr.pad_f : a.hdr.pad_col * ELEM;
    wk.pre_e = (MODE == MODE_PACK) ? a.hdr.pre_f : (a.hdr.pad_col + 1u) * ELEM;
    wk.pad_b = wk.pre_b = 0;
    if (MODE == MODE_PAIR) {
        wk.ncols_e = a.hdr.n_cols * a.hdr.n_cols * 2u;
        wk.pad_e = a.hdr.pad_col * a.hdr.n_cols * 2u;
        wk.pre_e = (a.hdr.pad_col + 1u) * a.hdr.n_cols * 2u;
        wk.pad_b = a.hdr.pad_col * 2u;
        wk.pre_b = (a.hdr.pad_col + 1u) * 2u;
    }
    if (MODE == MODE_SPARSE) wk.pad_e = wk.pre_e = a.hdr.win_lo_e;
    wk.win_on = a.hdr.win_on;
    wk.win_lo = a.hdr.win_lo_e;
    wk.win_hi = a.hdr.win_hi_e;
    wk.dead_hi = OP == OP_FIND ? a.hdr.fa_dead_hi : 0u;
    wk.sp_chains = a.hdr.sp_chains;
    wk.sp_pad_ident = a.hdr.sp_pad_ident;
    wk.flat = (CW == 2 && (MODE == MODE_TABLE8 || MODE == MODE_TABLE16)) ? a.hdr.flat_pages : 0u;
    wk.table_off = a.hdr.off_table - (MODE == MODE_SPARSE ? 0u : a.hdr.win_lo_e);
    wk.lane4 = (uint32_t)(lane & 31) * 4u;
    wk.gtable = (const uint16_t *)(a.prog + (MODE == MODE_HYBRID ? a.hdr.off_gtable : a.hdr.off_table));
    if (MODE == MODE_HYBRID) wk.gtable = (const uint16_t *)((const uint8_t *)wk.gtable - a.hdr.win_lo_e);
    wk.hot_last = a.hdr.hot_bytes - 2u + a.hdr.win_lo_e;
    const uint32_t accept_lo = MODE == MODE_PACK ? a.hdr.accept_off : a.hdr.accept_lo;
    const uint32_t start_state = MODE == MODE_PACK ? a.hdr.start_off : a.hdr.start;

    const PackedWindow<CHB> win(a.hdr.lds_bytes, a.tiles_in_f_rows, wave);
    const uint64_t n_rows = a.n_rows;

    // per-group state
    uint64_t rs, re;           // this lane's row as absolute byte addresses [rs, re) (packed_stream)
    uint32_t st, skip, rem;    // skip: chars from the origin to the walk's first char -- the row's start (PK_CURSOR: its cursor)
    int32_t last_o;            // OP_FIND: lastMatch + (rs & 15) / CW (origin-relative), -1 = none
    bool row_ok;
    auto begin_group = [&](uint64_t grp) __attribute__((always_inline)) {
        if constexpr (EXT == PK_CURSOR) {
            // Matcher.nextStart per row, as scan_kernel's `cursor`: the origin stays the row's first block, so positions stay
            // row-relative; chars before the cursor take PRE, blocks wholly before it are not walked, an exhausted row (< 0) starts
            // parked in the sink (find(): `if nextStart == -1 return false`, DFAClassBuilder.java:629-630)
            const uint64_t r = (grp << 6) + (uint64_t)lane;
            row_ok = r < n_rows;
            const uint32_t skip0 = (uint32_t)(rs & 15u) / CW;
            const uint32_t len = (uint32_t)((re - rs) / CW);
            rem = skip0 + len;
            // (the cursor pointer: read from the kernel arguments here, not held in SGPRs through the walk -- kernarg_here, needle_walk.h)
            const int32_t *const from = kernarg_ptr<const int32_t>(kernarg_here(), (uint32_t)offsetof(ScanArgs, from));
            const int32_t cur = row_ok ? from[r] : -1;
            st = cur < 0 ? 0u : start_state;
            skip = skip0 + (cur > 0 ? (uint32_t)cur : 0u);
            // :356 literal 0, then the first iteration's wasAccepted (:440) moves it to FROM if FROM < length (as scan_kernel)
            last_o = (a.hdr.root_accepting && cur >= 0) ? (int32_t)(skip0 + ((uint32_t)cur < len ? (uint32_t)cur : 0u)) : -1;
        } else {
            row_ok = ((grp << 6) + (uint64_t)lane) < n_rows;
            skip = (uint32_t)(rs & 15u) / CW;                 // chars of the origin block before the row
            rem = skip + (uint32_t)((re - rs) / CW);          // chars from the origin to the row's end
            st = start_state;
            last_o = (OP == OP_FIND && a.hdr.root_accepting) ? (int32_t)skip : -1; // :356, the first iteration's wasAccepted (:440)
        }
    };
    auto resolved = [&]() __attribute__((always_inline)) {
        return OP == OP_CONTAINED_IN ? (st >= accept_lo || st == 0u) : (st <= wk.dead_hi);
    };
    // the first byte the lane's walk needs: rs, or (PK_CURSOR) its cursor's char, at most re
    auto wanted_from = [&]() __attribute__((always_inline)) {
        if constexpr (EXT == PK_CURSOR) {
            // (recomputed at each use -- the window's first block, the advance after the walk -- rather than held across the walk:
            // that would cost 2 VGPRs in the kernel's busiest stretch)
            uint32_t k = skip < rem ? skip : rem;
            asm volatile("" : "+v"(k));
            return (rs & ~(uint64_t)15) + (uint64_t)k * CW;
        } else {
            return rs;
        }
    };
    // the row still wants text (PK_CURSOR: a cursor at or past the row's end wants none)
    auto unresolved = [&]() __attribute__((always_inline)) {
        if constexpr (EXT == PK_CURSOR) return !resolved() && skip < rem;
        else return !resolved();
    };

    // Walk the window at w (its bytes are in LDS): this lane's blocks of [max(wanted_from(), w), min(re, w + kWin)).
    auto walk_window = [&](uint64_t w) __attribute__((always_inline)) {
        const uint64_t from = wanted_from();
        const uint64_t lo = from > w ? from : w;
        const uint64_t hi = re < w + kWin ? re : w + kWin;
        if (lo < hi && !resolved()) {
            const uint32_t kb0 = (uint32_t)(lo - w) >> 4, kb1 = (uint32_t)(hi - 1u - w) >> 4; // first / last block (window-relative)
            const uint32_t rel = (uint32_t)(w - (rs & ~(uint64_t)15));                            // window start - origin (mod 2^32)
            auto p0_of = [&](uint32_t kb) __attribute__((always_inline)) { return (rel + kb * 16u) / CW; };
            {
                const u32x4 c = *(const lds_u32x4 *)(uintptr_t)win.at(kb0 * 16u);
                const uint32_t wv[4] = {c[0], c[1], c[2], c[3]};
                walk_piece<OP, CW, MODE, true>(wk, wv, p0_of(kb0), rem, skip, accept_lo, st, last_o);
            }
            if (kb1 > kb0) {
                u32x4 v = *(const lds_u32x4 *)(uintptr_t)win.at((kb0 + 1u) * 16u);
                for (uint32_t kb = kb0 + 1u; kb < kb1; ++kb) {
                    const uint32_t wv[4] = {v[0], v[1], v[2], v[3]};
                    v = *(const lds_u32x4 *)(uintptr_t)win.at((kb + 1u) * 16u); // next block: its latency hides below
                    walk_piece<OP, CW, MODE, false>(wk, wv, p0_of(kb), 0u, 0u, accept_lo, st, last_o);
                }
                const uint32_t wv[4] = {v[0], v[1], v[2], v[3]};
                walk_piece<OP, CW, MODE, true>(wk, wv, p0_of(kb1), rem, skip, accept_lo, st, last_o);
            }
        }
    };

    // Verdicts: the group's bitmap word (one vector store by lane 0) and find()'s start / end per row (DFAClassBuilder.java:640-656) --
    // two int32 arrays, or (PK_FORMS) one dword / uint16 per row with the escapes of pack16_or_over / pack8_or_over.
    auto finish_rows = [&](uint64_t grp) __attribute__((always_inline)) {
        bool res;
        const uint32_t skip0 = EXT == PK_CURSOR ? (uint32_t)(rs & 15u) / CW : skip; // chars of the origin block before the row
        const int32_t last = last_o >= 0 ? last_o - (int32_t)skip0 : -1; // row-relative lastMatch
        if (OP == OP_FIND) res = row_ok && last >= 0;
        else res = row_ok && st >= accept_lo;
        const uint64_t word = __ballot(res);
        if (lane == 0) a.bitmap[grp] = word;
        if (OP != OP_FIND) return;
        int32_t s = -1;
        const int32_t e = res ? last : -1;
        if (a.fixed_len >= 0) {
            s = res ? last - a.fixed_len : -1; // :640-646
        } else if (LEN) {
            uint32_t pidx = st;                // the lengths automaton's stop state names the match length (needle_lower.h)
            if (MODE == MODE_SPARSE) {
                const uint32_t st_end = sparse_end<CW>(wk, st, st > wk.dead_hi, a.hdr.sp_end_col4);
                pidx = (st_end & 0xFFFFu) - a.hdr.sp_dead_row0;
            }
            s = res ? last - (int32_t)lds_u8(a.hdr.fa_len_off + pidx) : -1;
        } else {
            // indexBackwards(end - 1, FROM), :536-583, on the row's text in memory (read a moment ago: L2).  No LDS window (0 bytes):
            // every char comes from the row itself, so the walk reads nothing outside it.  FROM: the cursor (PK_CURSOR), else 0.
            const uint8_t *rowp = (const uint8_t *)(uintptr_t)rs;
            s = backward_walk<CW>(a, res, last, EXT == PK_CURSOR ? (int32_t)(skip - skip0) : 0, win.base, 0u, 0u, 0u, rowp);
            s = res ? s : -1;
        }
        if constexpr (EXT == PK_FORMS) {
            // (the form's words: read from the kernel arguments here, once per group, not held in SGPRs through the walk --
            // kernarg_here, needle_walk.h)
            const KernargPtr ka = kernarg_here();
            uint32_t *const o_packed = kernarg_ptr<uint32_t>(ka, (uint32_t)offsetof(ScanArgs, packed));
            const bool form8 = kernarg_u32(ka, (uint32_t)offsetof(ScanArgs, packed8)) != 0u;
            bool over = false; // this row's match does not fit the form
            if (row_ok) {
                const uint64_t r = (grp << 6) + (uint64_t)lane;
                if (form8) {
                    over = e > 256;
                    ((uint16_t *)o_packed)[r] = pack8_or_over(s, e);
                } else {
                    over = e > 65534;
                    o_packed[r] = pack16_or_over(s, e);
                }
            }
            int32_t *const o_overflow = kernarg_ptr<int32_t>(ka, (uint32_t)offsetof(PackedArgs, overflow));
            const uint64_t esc = __ballot(over);
            if (o_overflow && esc != 0ull && lane == __builtin_ctzll(esc)) *o_overflow = 1; // one store per wave
        } else if (row_ok) {
            const uint64_t r = (grp << 6) + (uint64_t)lane;
            a.start[r] = s;
            a.end[r] = e;
        }
    };

    packed_stream<CW, CHB>(lane, wave, n_waves, a.rows, pa.offsets, n_rows, win, rs, re, begin_group, walk_window, unresolved, wanted_from,
                           finish_rows);
}

// ------------------------------------------------------------------------------------------------
// launcher (shape: scan_kernel's, from the automaton's LDS footprint -- the window is the tile of that shape)
// ------------------------------------------------------------------------------------------------
struct PackedShape {
    int grid, waves, chb;
    size_t lds;
};

template <int OP, int CW, int MODE, int CHB, bool LEN, int EXT>
static hipError_t launch_packed_one(const PackedArgs &a, PackedShape sh, hipStream_t stream) {
    auto k = packed_kernel<OP, CW, MODE, CHB, LEN, EXT>;
    static thread_local uint64_t configured = 0;
    if (hipError_t e = allow_full_lds((const void *)k, configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(sh.grid), dim3(sh.waves * 64), sh.lds, stream, a);
    return hipGetLastError();
}

// The cursor kernels of 8-bit rows in the LDS-table, HBM-table, hot-rows and compressed modes take 64-byte windows only (launch_packed
// narrows the shape): with 128-byte windows their cursor bookkeeping needs 120-121 VGPRs, above the plain kernels' 119
// (scripts/kernel_resources.py).  Packed-function and pair-table programs and UTF-16 rows keep the plain kernels' windows.
constexpr bool packed_cursor_narrow(int cw, uint32_t mode) { return cw == 1 && mode != MODE_PACK && mode != MODE_PAIR; }

template <int OP, int CW, int MODE, int EXT>
static hipError_t launch_packed_g(const PackedArgs &a, PackedShape sh, hipStream_t s) {
    if constexpr (EXT == PK_CURSOR && packed_cursor_narrow(CW, MODE)) {
        if (sh.chb != 64) return hipErrorInvalidValue;
        if constexpr (MODE == MODE_TABLE8 || MODE == MODE_TABLE16 || MODE == MODE_SPARSE || MODE == MODE_PAIR)
            if (a.s.hdr.fa_len_off) return launch_packed_one<OP, CW, MODE, 64, true, EXT>(a, sh, s);
        return launch_packed_one<OP, CW, MODE, 64, false, EXT>(a, sh, s);
    } else {
        if constexpr (OP == OP_FIND && (MODE == MODE_TABLE8 || MODE == MODE_TABLE16 || MODE == MODE_SPARSE || MODE == MODE_PAIR)) {
            if (a.s.hdr.fa_len_off) // (a "lengths" program: only these modes)
                return sh.chb == 128 ? launch_packed_one<OP, CW, MODE, 128, true, EXT>(a, sh, s) : launch_packed_one<OP, CW, MODE, 64, true, EXT>(a, sh, s);
        }
        return sh.chb == 128 ? launch_packed_one<OP, CW, MODE, 128, false, EXT>(a, sh, s) : launch_packed_one<OP, CW, MODE, 64, false, EXT>(a, sh, s);
    }
}

template <int OP, int CW, int EXT = PK_PLAIN>
static hipError_t launch_packed_m(const PackedArgs &a, PackedShape sh, hipStream_t s) {
    switch (a.s.hdr.mode) {
    case MODE_PACK: return launch_packed_g<OP, CW, MODE_PACK, EXT>(a, sh, s);
    case MODE_TABLE8: return launch_packed_g<OP, CW, MODE_TABLE8, EXT>(a, sh, s);
    case MODE_TABLE16: return launch_packed_g<OP, CW, MODE_TABLE16, EXT>(a, sh, s);
    case MODE_PAIR: return CW == 1 ? launch_packed_g<OP, 1, MODE_PAIR, EXT>(a, sh, s) : hipErrorInvalidValue; // 8-bit rows only
    case MODE_HYBRID: return launch_packed_g<OP, CW, MODE_HYBRID, EXT>(a, sh, s);
    case MODE_SPARSE: return launch_packed_g<OP, CW, MODE_SPARSE, EXT>(a, sh, s);
    default: return launch_packed_g<OP, CW, MODE_GLOBAL, EXT>(a, sh, s);
    }
}

} // namespace needle
