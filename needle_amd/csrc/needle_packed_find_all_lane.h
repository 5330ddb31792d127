// needle_packed_find_all_lane.h -- every non-overlapping match of every row of a PACKED batch (needle_packed_view) for patterns WITHOUT a
// find-all transducer: nullable patterns (`[a-c]*`), unbounded ones whose starts need indexBackwards (`http://.+`), nested dictionaries
// (`international|inter|nation`), `abc+d|ab`.  The reference's repeated Matcher.find() (DFAClassBuilder.java:616-659, nextStart = end) on
// each row, hand-written for gfx950 (CDNA4).  Included by needle_packed_find_all_lane{1,2}.hip (one per char width).
//
//   Staging: packed_kernel's (needle_packed.h packed_stream, unchanged): a wave owns 64 consecutive rows and streams their one contiguous
//   span through its LDS window; no 16-byte block without a byte of the group's span is loaded.
//   Walk: find_all_kernel's (needle_find_all.hip walk_tile).  After a match [start, end) the search restarts AT `end`, chars the walk has
//   already consumed while it waited for the automaton to die, so the lanes of a wave stop being at the same char: every lane keeps its own
//   BLOCK index (16-byte block counted from its row's origin) and cursor, and walk_window iterates "every live lane walks its current
//   block" (walk_piece_fa, needle_find_all_walk.h) until every live lane stands at or past the window's end, or is done with its row.
//   Positions are origin-relative as in packed_kernel: the origin is the row's start rounded down to its 16-byte block, the lane's first
//   cursor the `skip` chars of the origin block in front of the row -- hidden by the guard that hides the chars before any restart cursor
//   (the lengths form with skip states: the search enters the block in skip state fa_skip_lo + skip - 1).  The row's end is the fixed-
//   stride kernel's ragged end: flags masked beyond `rem`, the CUT re-walk with the PAD column for the lengths form.
//   Restarts: a lane whose search died files the match and moves its cursor to `end`.  The block holding `end` is read from the window
//   while it is still there, else from memory, 16-byte blocks of the lane's own row, until the lane is back in the window: the stream
//   never moves backwards.  unresolved() = the row is not done; wanted_from() = the address of the lane's current block.
//   Starts: the three forms of find_all_kernel, chosen by the same FindAllArgs fields -- the lengths programs (lmode / LM), the immediate
//   form (one match length, nullable patterns: backward_walk per match, the window as its text), and the deferred starts_phase (the
//   group's matches numbered through and handed out 64 at a time, their text -- the block holding char end - 1 and the one before it,
//   clamped to the row's origin block -- back from memory / L2 into the lane's slot of the by then free window).
//   Results (FindAllArgs): counting only, or CSR filing at caller offsets (match k of row r at offsets[r] + k).  Result indices are
//   64-bit, positions row-relative int32 (rows of at most 2^31 - 1 chars); counts[r] = min(matches, room), *more = a row had more.
//
// Memory safety: the window loads are packed_stream's.  A restart block is block `pi` of the lane's row with pi * CPP < rem: it holds a
// char of the row.  The deferred starts read the block of char end - 1 and blocks between it and the origin block: each holds a char of the
// row.  backward_walk reads single chars of [bound, end) -- inside the row.  Nothing else is loaded.
#pragma once
#include "needle_packed.h"
#include "needle_find_all.h"
#include "needle_find_all_walk.h"

namespace needle {

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

    // walk constants: as find_all_kernel sets them up
    Walk wk;
    constexpr uint32_t ELEM = MODE == MODE_TABLE16 ? 2u : 1u;
    wk.ncols_e = a.hdr.n_cols * ELEM;
    wk.pad_e = (MODE == MODE_PACK) ? a.hdr.pad_f : a.hdr.pad_col * ELEM;
    wk.pre_e = (MODE == MODE_PACK) ? a.hdr.pre_f : (a.hdr.pad_col + 1u) * ELEM;
    wk.pad_b = wk.pre_b = 0;
    wk.table_off = a.hdr.off_table;
    wk.win_on = 0, wk.win_lo = 0, wk.win_hi = 0; // (the find-all programs are lowered without window addressing)
    wk.sp_chains = 0, wk.sp_pad_ident = 0, wk.dead_hi = 0;
    wk.flat = (CW == 2 && (MODE == MODE_TABLE8 || MODE == MODE_TABLE16)) ? a.hdr.flat_pages : 0u;
    if ((MODE == MODE_TABLE8 || MODE == MODE_TABLE16) && a.hdr.win_on) { // a lengths program in window layout
        wk.win_on = 1, wk.win_lo = a.hdr.win_lo_e, wk.win_hi = a.hdr.win_hi_e;
        wk.table_off = a.hdr.off_table - a.hdr.win_lo_e;
    }
    wk.lane4 = (uint32_t)lane * 4u; // packed mode on 8-bit rows: all 64 lane copies of F are there (no windows in the F rows)
    wk.gtable = (const uint16_t *)(a.prog + a.hdr.off_table);
    wk.hot_last = a.hdr.hot_bytes - 2u;
    const uint32_t accept_lo = MODE == MODE_PACK ? a.hdr.accept_off : a.hdr.accept_lo;
    const uint32_t start_state = MODE == MODE_PACK ? a.hdr.start_off : a.hdr.start;

    const PackedWindow<CHB> win(a.hdr.lds_bytes, 0u, wave);
    const uint32_t slot_addr = win.at((uint32_t)lane * CHB); // this lane's CHB bytes of the window (the deferred starts' text)
    const uint64_t n_rows = a.n_rows;

    // ---- per-group (per-row) state
    uint64_t rs, re;            // this lane's row as absolute byte addresses [rs, re) (packed_stream)
    uint64_t org = 0;           // the row's origin: rs rounded down to its 16-byte block
    bool row_ok = false, done = true;
    uint32_t skip = 0, rem = 0; // chars of the origin block before the row; skip + the row's chars (the fixed-stride kernel's `len`)
    uint32_t st = 0, pi = 0, count = 0;
    int32_t last = -1, cursor = 0; // origin-relative
    uint64_t out0 = 0;          // index of this row's first result slot (offsets[row])
    uint32_t cap = 0;           // matches this row may file

    auto begin_group = [&](uint64_t grp) __attribute__((always_inline)) {
        const uint64_t my_row = (grp << 6) + (uint64_t)lane;
        row_ok = my_row < n_rows;
        org = rs & ~(uint64_t)15;
        skip = (uint32_t)(rs & 15u) / CW;
        rem = skip + (uint32_t)((re - rs) / CW);
        cursor = (int32_t)skip;
        pi = 0;
        count = 0;
        st = start_state;
        if (LM) st = skip ? a.hdr.fa_skip_lo + skip - 1u : start_state; // S_k swallows the skip chars in front of the row
        last = a.hdr.root_accepting ? (int32_t)skip : -1; // :356 literal 0 (row-relative)
        out0 = 0;
        cap = fa.count_only ? 0xFFFFFFFFu : 0u;
        if (fa.offsets) {
            out0 = row_ok ? fa.offsets[my_row] : 0ull;
            cap = row_ok ? (uint32_t)(fa.offsets[my_row + 1] - out0) : 0u;
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(cap)); // (no vmcnt wait inside the walk)
        }
        done = !row_ok;
        // An EMPTY row has no block of its own (a group of empty rows has no window at all): its find() is decided here -- the one empty
        // match of a pattern that accepts the empty string (what the fixed-stride kernel's walk over PAD arrives at), else nothing.
        if (row_ok && rem == skip) {
            done = true;
            if (a.hdr.root_accepting) {
                const bool file = count < cap;
                if (!file) *fa.more = 1;
                if (file && !fa.count_only) {
                    fa.starts[out0] = 0;
                    fa.ends[out0] = 0;
                }
                count = file ? 1u : 0u;
            }
        }
    };

    // Walk the window at w (its bytes are in LDS) until every live lane is past it or done.
    auto walk_window = [&](uint64_t w) __attribute__((always_inline)) {
        const uint64_t wend = w + kWin;
        const int32_t win_b0 = (int32_t)(uint32_t)(w - org); // the window's first byte, origin-relative (mod 2^32: negative when the row starts inside it)
        // (the immediate form's backward walks take their text from the window only where origin-relative BYTE offsets fit an int32)
        const uint32_t bw_bytes = rem < (1u << 30) ? kWin : 0u;
        for (;;) {
            const uint32_t p0 = pi * CPP;
            const uint64_t ba = org + ((uint64_t)pi << 4); // the lane's current block
            const bool beyond = p0 >= rem; // nothing of the row there (a walk over PAD: the search ends)
            const bool active = !done && (ba < wend || beyond);
            if (__ballot(active) == 0ull) break;
            // The iteration is straight-line code for all 64 lanes, as in find_all_kernel: idle lanes walk a block too and their results
            // are dropped by selects.
            const bool in_lds = active && !beyond && ba >= w;
            u32x4 v = *(const lds_u32x4 *)(uintptr_t)win.at(in_lds ? (uint32_t)(ba - w) : 0u);
            const bool in_mem = active && !beyond && ba < w;
            if (__ballot(in_mem) != 0ull) { // a restart behind the window (rare): waited for HERE, so that the common path carries no
                                            // vmcnt wait (the window prefetch and match stores are in flight)
                if (in_mem) {
                    v = *(const u32x4 *)(uintptr_t)ba; // (block pi of the row, pi * CPP < rem: it holds a char of the row)
                    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v));
                }
            }
            const uint32_t w4[4] = {v[0], v[1], v[2], v[3]}; // (a block beyond the row: whatever is there -- its flags are masked)
            const uint32_t skip_rel = (uint32_t)cursor > p0 ? (uint32_t)cursor - p0 : 0u; // < CPP: the cursor's block, or none
            const uint32_t st_old = st;
            uint32_t st_new = st;
            const uint32_t in_row = rem > p0 ? rem - p0 : 0u; // chars of the block inside the row (all, if >= CPP)
            uint32_t acc = walk_piece_fa<CW, MODE, false, LM>(wk, w4, skip_rel, accept_lo, st_new, in_row);
            if (!LM) acc &= ~((1u << skip_rel) - 1u);          // an accepting start state does not count before the cursor
            acc &= in_row < (uint32_t)CPP ? (1u << in_row) - 1u : 0xFFFFFFFFu;
            acc = active ? acc : 0u;
            last = acc ? (int32_t)(p0 + 32u - (uint32_t)__builtin_clz(acc)) : last;
            st = active ? st_new : st;
            // (fa_dead_n: the "lengths" automaton's dead-with-a-match-pending states; 0 for every other program)
            const bool died = st_new == 0u || st_new - a.hdr.fa_dead_lo < a.hdr.fa_dead_n;
            const bool ended = active && (died || p0 + CPP >= rem);
            pi += (active && !ended) ? 1u : 0u;
            if (__ballot(ended) == 0ull) continue;
            // ---- find() returns for the lanes of `ended` (:629-657)
            const bool hit = ended && last >= 0;
            const int32_t en = last;
            if (ended && !hit) done = true; // no further match in this row
            if (LM || fa.lmode) {
                // The "lengths" automaton: start = end - pend[end state].  A row that ends INSIDE this block was walked past its end
                // above: that block is walked again from its entry state with the PAD column (find_all_kernel).
                uint32_t st_end = st_new;
                if (MODE == MODE_TABLE8 || MODE == MODE_TABLE16) { // (the only modes such a program has)
                    const bool cut = hit && in_row < (uint32_t)CPP;
                    if (__ballot(cut) != 0ull) {
                        uint32_t st_fix = st_old;
                        (void)walk_piece_fa<CW, MODE, true, LM>(wk, w4, skip_rel, accept_lo, st_fix, in_row);
                        st_end = cut ? st_fix : st_end;
                    }
                }
                const int32_t mlen = (int32_t)lds_u8(a.hdr.fa_len_off + (hit ? st_end : 0u));
                const bool file = hit && count < cap;
                if (hit && !file) *fa.more = 1;
                done = done || (hit && !file);
                if (file && !fa.count_only) {
                    fa.starts[out0 + count] = en - mlen - (int32_t)skip;
                    fa.ends[out0 + count] = en - (int32_t)skip;
                }
                count += file ? 1u : 0u;
                cursor = file ? en : cursor;
                const uint32_t pi_en = ((uint32_t)en * CW) >> 4;
                uint32_t st_again = start_state;
                if (LM) { // en - pi_en * CPP chars of the block lie before the new cursor: S_k swallows them
                    const uint32_t rel = (uint32_t)en - pi_en * (uint32_t)CPP;
                    st_again = rel ? a.hdr.fa_skip_lo + rel - 1u : start_state;
                }
                st = file ? st_again : st;
                last = file ? -1 : last;
                pi = file ? pi_en : pi;
            } else if (fa.defer) {
                // not nullable, start by indexBackwards: the match is not empty and ends beyond its cursor -- the row goes on.
                // (selects, not branches: find_all_kernel)
                const bool file = hit && count < cap;
                if (hit && !file) *fa.more = 1;
                done = done || (hit && !file);
                if (file && !fa.count_only) fa.ends[out0 + count] = en - (int32_t)skip; // (the start joins it in starts_phase)
                count += file ? 1u : 0u;
                cursor = file ? en : cursor;
                st = file ? start_state : st;
                last = file ? -1 : last;
                pi = file ? (((uint32_t)en * CW) >> 4) : pi;
            } else {
                int32_t s = en - a.fixed_len;
                if (a.fixed_len < 0) // indexBackwards(end - 1, cursor): the window as its text, anything else from the row in memory
                    s = backward_walk<CW>(a, hit, en, cursor, win.base, (uint32_t)win_b0, bw_bytes, 0u, (const uint8_t *)(uintptr_t)org);
                // en < s: the wrapped pseudo-match of a nullable pattern searched from cursor == length; dropped, ends the row
                const bool valid = hit && en >= s;
                if (hit && !valid) done = true;
                if (valid) {
                    if (count < cap) {
                        if (!fa.count_only) {
                            fa.starts[out0 + count] = s - (int32_t)skip;
                            fa.ends[out0 + count] = en - (int32_t)skip;
                        }
                        ++count;
                        // the row goes on only while the cursor advances (needle_hip.h)
                        if (en == s || en <= cursor) {
                            done = true;
                        } else {
                            cursor = en;
                            st = start_state;
                            last = a.hdr.root_accepting ? (((uint32_t)cursor < rem) ? cursor : (int32_t)skip) : -1;
                            pi = ((uint32_t)en * CW) >> 4;
                        }
                    } else {
                        *fa.more = 1;
                        done = true;
                    }
                }
            }
        }
    };

    // defer != 0: the starts of the group's matches, found at the end of the group as find_all_kernel's starts_phase finds them: the
    // matches of the 64 rows numbered through and handed out 64 at a time, one per lane, whichever row they belong to.  The text comes
    // back from memory / L2 into the lane's slot of the window (free: the next window waits in registers); the ends are read back with
    // agent-scope loads (this wave wrote them a moment ago).
    auto starts_phase = [&]() __attribute__((always_inline)) {
        uint32_t incl = count;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
            incl += lane >= o ? t : 0u;
        }
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (total == 0u) return;
        const uint32_t excl = incl - count;
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): this wave's stores of the ends have reached L2
        for (uint32_t j0 = 0; j0 < total; j0 += 64u) {
            const uint32_t j = j0 + (uint32_t)lane;
            const bool act = j < total;
            uint32_t lo = 0, hi = 63;
#pragma unroll
            for (int it = 0; it < 6; ++it) { // the first lane whose inclusive count exceeds j
                const uint32_t mid = (lo + hi) >> 1;
                const uint32_t pm = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(mid << 2), (int)incl);
                const bool right = pm <= j;
                lo = right ? mid + 1u : lo;
                hi = right ? hi : mid;
            }
            const uint32_t owner = act ? lo : (uint32_t)lane;
            auto of_owner = [&](uint32_t x) __attribute__((always_inline)) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(owner << 2), (int)x); };
            const uint32_t k = j - of_owner(excl);
            const uint64_t o_out0 = (uint64_t)of_owner((uint32_t)out0) | ((uint64_t)of_owner((uint32_t)(out0 >> 32)) << 32);
            const uint64_t o_org = (uint64_t)of_owner((uint32_t)org) | ((uint64_t)of_owner((uint32_t)(org >> 32)) << 32);
            const uint32_t o_skip = of_owner(skip);
            int32_t en = 1, bound = 0; // row-relative
            if (act) {
                en = __hip_atomic_load(&fa.ends[o_out0 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (k) bound = __hip_atomic_load(&fa.ends[o_out0 + k - 1u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const int32_t en_o = en + (int32_t)o_skip, bound_o = bound + (int32_t)o_skip; // origin-relative
            const uint32_t pa = ((uint32_t)(en_o - 1) * CW) >> 4; // text: the block holding char en - 1 and the one before it, not below the origin block
            const uint32_t pb = pa ? pa - 1u : 0u;
            u32x4 va = {0, 0, 0, 0}, vb = {0, 0, 0, 0};
            if (act) { // (en >= 1: both blocks lie between the origin block and the block of char en - 1 -- each holds a char of the row)
                va = *(const u32x4 *)(uintptr_t)(o_org + ((uint64_t)pa << 4));
                vb = *(const u32x4 *)(uintptr_t)(o_org + ((uint64_t)pb << 4));
            }
            *(lds_u32x4 *)(uintptr_t)(slot_addr) = vb;
            *(lds_u32x4 *)(uintptr_t)(slot_addr + 16u) = va;
            // (rows whose origin-relative byte offsets do not fit an int32: no text window, every char from the row in memory)
            const bool wide = (uint32_t)en_o >= (1u << 30);
            const uint32_t t_b0 = pa ? pb * 16u : 0u;
            const uint32_t t_addr = pa ? slot_addr : slot_addr + 16u;
            const uint32_t t_bytes = wide ? 0u : (pa ? 32u : 16u);
            const int32_t st_o = fa.defer == 2u ? bound_o : backward_walk<CW>(a, act, en_o, bound_o, t_addr, t_b0, t_bytes, 0u, (const uint8_t *)(uintptr_t)o_org); // (2: measurement aid)
            if (act) fa.starts[o_out0 + k] = st_o - (int32_t)o_skip;
        }
    };

    auto finish_rows = [&](uint64_t grp) __attribute__((always_inline)) {
        if (row_ok && fa.counts) fa.counts[(grp << 6) + (uint64_t)lane] = count;
        if (fa.defer && !fa.count_only) starts_phase();
    };

    packed_stream<CW, CHB>(lane, wave, n_waves, a.rows, pf.row_offsets, n_rows, win, rs, re, begin_group, walk_window,
                           [&]() __attribute__((always_inline)) { return !done; },
                           [&]() __attribute__((always_inline)) { return org + ((uint64_t)pi << 4); }, finish_rows);
}

// Waves per workgroup x window bytes per lane for a per-lane find-all program of prog_lds_bytes on rows of char_width: find_all_kernel's
// candidates (the program plus one window per wave within the 160 KiB of LDS) without those that spill.  false: no shape fits.
bool packed_find_all_lane_shape(uint32_t prog_lds_bytes, int char_width, int *waves, int *chb);

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
