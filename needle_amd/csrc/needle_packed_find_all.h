// needle_packed_find_all.h -- every non-overlapping match of every row of a PACKED batch (needle_packed_view: one buffer of code
// units + offsets[n + 1]) in one pass, hand-written for gfx950 (CDNA4).  The reference's repeated Matcher.find()
// (DFAClassBuilder.java:616-659, DFACompilerTest.java:66-78) on each row, as find_all_lockstep_kernel (needle_find_all_ls.hip) computes it
// for fixed-stride rows, without converting the batch first.  Included by needle_packed_find_all{1,2}.hip (one per char width).
//
//   Staging: packed_kernel's (needle_packed.h packed_stream): a wave owns 64 consecutive rows, streams their one contiguous span through
//   its LDS window by lane-linear 16-byte `nt` loads from 128-byte aligned bases, the next window held in VGPRs; no 16-byte block
//   without a byte of the group's span is loaded.
//   Walk: each lane walks its own row's blocks of the window with the transducer step of the lock-step kernel,
//       entry = T[(entry >> 4) * row_bytes + column(char)],   log = {entry, log} >> 4,
//   the 4-bit match codes filed from the log.  Both transducers: the lengths one (get_program variant 8, a code names (length, k))
//   and the RUN one (variant 11, bit 0: a match ends in front of this char, bit 1: this char may begin a run, with the per-lane
//   run_start register).  The walk set-up, the chain, the decode and the row's end below are a COPY of needle_find_all_ls_walk.h's
//   (the fixed-stride kernel's), kept on purpose: written over that header's lane-state struct and Rows policy this kernel's ISA is
//   the same up to a handful of instructions, yet three of its four rate figures run 0.4-0.8 % slower, in every round, whichever of the
//   chain and the decode it keeps to itself (profiles/find_all_packed.md).  A fix to the decode there is a fix to make here too.
//   Row edges.  A row starts and ends at arbitrary code units.  The transducer programs have no PRE (identity) column, so chars of the
//   row's first block that lie before its start are SELECTED away on the state chain: the entry stays the start entry (code 0, no run
//   start).  Chars at or after the row's end take the PAD column: the first one emits what is pending and leads to the dead state, whose
//   entries are all 0 -- and a row that ends on a block boundary takes its PAD transition after the group's last window.  So every row
//   takes exactly one PAD transition with effect, at its true end.
//   Positions are row-relative int32 (rows of at most 2^31 - 1 chars): the block's first char counted from the row's origin (its first
//   char rounded down to a 16-byte block) minus the chars of the origin block in front of the row.
//   Results (FindAllArgs): counting only (counts), CSR filing at caller offsets (match k of row r at offsets[r] + k, int32 start / end),
//   or group-blocked one-dword slots (kshift 6: match k of row r at ((r >> 6) * slots + k) * 64 + (r & 63), start | end << 16 -- a
//   packed group is the same 64 consecutive rows as a fixed-stride one, so needle_compact.hip's compaction applies unchanged).  Result
//   indices are 64-bit per lane: a packed group's span, and so its matches, has no bound.
#pragma once
#include "needle_packed.h"
#include "needle_find_all.h"

namespace needle {

template <int CW, int CHB, bool RUNS>
__global__ __launch_bounds__(kWavesPerBlock * 64) void packed_find_all_kernel(const PackedFindAllArgs pf) {
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

    // walk constants: as find_all_ls_setup (needle_find_all_ls_walk.h) sets them up
    Walk wk;
    wk.ncols_e = a.hdr.n_cols * 2u;
    wk.pad_e = a.hdr.pad_col * 2u;
    wk.pre_e = wk.pad_e; // (never taken: chars before a row's start are selected away)
    wk.pad_b = wk.pre_b = 0;
    wk.win_on = a.hdr.win_on, wk.win_lo = a.hdr.win_lo_e, wk.win_hi = a.hdr.win_hi_e;
    wk.table_off = a.hdr.off_table - a.hdr.win_lo_e;
    wk.sp_chains = 0, wk.sp_pad_ident = 0, wk.dead_hi = 0, wk.lane4 = 0, wk.gtable = nullptr, wk.hot_last = 0;
    wk.flat = 0;
    const uint32_t tbase = CW == 1 ? (uint32_t)kLdsTable1 : 0u;
    const uint32_t pad_addr = wk.pad_e + (CW == 1 ? (uint32_t)kLdsTable1 : wk.table_off);
    const uint32_t codes_off = a.hdr.ft_codes_off;
    const uint32_t e_start = a.hdr.start << 4;
    const bool blocked = fa.kshift != 0u; // (wave-uniform)

    const PackedWindow<CHB> win(a.hdr.lds_bytes, 0u, wave);
    const uint64_t n_rows = a.n_rows;

    // ---- per-group (per-row) state
    uint64_t rs, re;       // this lane's row as absolute byte addresses [rs, re) (packed_stream)
    bool row_ok = false, too_long = false;
    uint32_t skip = 0, rem = 0; // chars of the origin block before the row; skip + the row's chars
    uint32_t e = 0;
    uint32_t run_start = 0; // RUNS: row index of the last char that may have begun a run
    uint32_t count = 0;     // matches of this row so far -- ALL of them; the first `cap` are filed
    uint32_t cap = 0;       // matches this row may file
    uint64_t base = 0;      // result index of the row's first match (CSR: offsets[r]; group-blocked: the group's first slot + lane)

    auto begin_group = [&](uint64_t grp) __attribute__((always_inline)) {
        const uint64_t my_row = (grp << 6) + (uint64_t)lane;
        row_ok = my_row < n_rows;
        skip = (uint32_t)(rs & 15u) / CW;
        rem = skip + (uint32_t)((re - rs) / CW);
        e = row_ok ? e_start : 0u;
        count = 0;
        run_start = 0;
        cap = fa.count_only ? 0xFFFFFFFFu : fa.slots;
        base = blocked ? ((grp * fa.slots) << 6) + (uint64_t)lane : 0ull;
        if (fa.offsets) {
            const uint64_t o0 = row_ok ? fa.offsets[my_row] : 0ull;
            const uint64_t o1 = row_ok ? fa.offsets[my_row + 1] : 0ull;
            base = o0;
            cap = (uint32_t)(o1 - o0);
        }
        too_long = blocked && rem - skip > 65535u; // (the one-dword form holds 16-bit positions)
        if (too_long) cap = 0;
    };
    // one match [s, en) of this lane (the lanes of `hit`): filed while the row has room, counted always
    auto put = [&](bool hit, uint32_t s, uint32_t en) __attribute__((always_inline)) {
        if (hit && count < cap && !fa.count_only) {
            const uint64_t i = blocked ? base + ((uint64_t)count << 6) : base + count;
            if (fa.packed) {
                fa.packed[i] = s | en << 16;
            } else {
                fa.starts[i] = (int32_t)s;
                fa.ends[i] = (int32_t)en;
            }
        }
        count += hit ? 1u : 0u;
    };
    // a match filed at char index pos with d = codes[code] = (k + length) | k << 16: [pos - (k + length), pos - k) (needle_device.h)
    auto file = [&](bool hit, uint32_t pos, uint32_t d) __attribute__((always_inline)) { put(hit, pos - (d & 0xFFFFu), pos - (d >> 16)); };

    // The match codes of 8 consecutive chars (char j in nibble j of h; pos0 = row index of char 0) -- as find_all_ls_decode (needle_find_all_ls_walk.h)
    const bool direct_codes = a.hdr.ft_direct != 0u;
    const bool odd_codes = a.hdr.ft_odd != 0u;
    auto decode = [&](uint32_t h, uint32_t pos0) __attribute__((always_inline)) {
        if (RUNS) {
            uint32_t t = h & 0x11111111u;              // bit 4j: a match ends in front of char j
            const uint32_t tf = (h >> 1) & 0x11111111u; // bit 4j: char j may begin a run
            if (fa.count_only) {
                count += (uint32_t)__builtin_popcount(t);
                return;
            }
            if (__ballot(t != 0u) != 0ull) {
                do {
                    const bool has = t != 0u;
                    uint32_t b;
                    asm("v_ffbl_b32 %0, %1" : "=v"(b) : "v"(t));
                    t &= t - 1u;
                    const uint32_t below = tf & ((1u << (b & 31u)) - 1u);
                    const uint32_t st = below ? pos0 + ((31u - (uint32_t)__builtin_clz(below)) >> 2) : run_start;
                    put(has, st, pos0 + ((b & 31u) >> 2));
                } while (__ballot(t != 0u) != 0ull);
            }
            run_start = tf ? pos0 + ((31u - (uint32_t)__builtin_clz(tf)) >> 2) : run_start;
            return;
        }
        if (__ballot(h != 0u) == 0ull) return;
        uint32_t t = h;
        if (!odd_codes) {
            t |= t >> 1;
            t |= t >> 2;
        }
        t &= 0x11111111u;
        if (fa.count_only) {
            count += (uint32_t)__builtin_popcount(t);
            return;
        }
        if (direct_codes) { // the code names the match's length, k = 0
            const uint32_t hl = a.hdr.ft_direct == 2u ? h >> 1 : h;
            do {
                const bool has = t != 0u;
                uint32_t b;
                asm("v_ffbl_b32 %0, %1" : "=v"(b) : "v"(t));
                t &= t - 1u;
                file(has, pos0 + (b >> 2), __builtin_amdgcn_ubfe(hl, b, a.hdr.ft_direct == 2u ? 3u : 4u));
            } while (__ballot(t != 0u) != 0ull);
            return;
        }
        do {
            const bool has = t != 0u;
            uint32_t b;
            asm("v_ffbl_b32 %0, %1" : "=v"(b) : "v"(t));
            t &= t - 1u;
            file(has, pos0 + (b >> 2), lds_u32(codes_off + (__builtin_amdgcn_ubfe(h, b, 4) << 2)));
        } while (__ballot(t != 0u) != 0ull);
    };

    // One 16-byte block of the row: p0 = origin-relative index of its first char.  GUARD (the row's first / last block of a window):
    // chars before the row's start leave the entry as it is (the start entry: code 0), chars at or after its end take PAD.
    auto walk_block = [&](const u32x4 &v, uint32_t p0, auto guard) __attribute__((always_inline)) {
        constexpr bool G = decltype(guard)::value;
        const uint32_t w[4] = {v[0], v[1], v[2], v[3]};
        uint32_t col[CPP];
        piece_lookups<MODE_TABLE16, CW, G>(wk, w, p0, rem, 0u, col);
        uint32_t h0 = 0, h1 = 0;
#pragma unroll
        for (int i = 0; i < CPP; ++i) {
            uint32_t ne = lds_u16(__umul24(e >> 4, wk.ncols_e) + col[i] + tbase);
            if (G) ne = (p0 + (uint32_t)i < skip) ? e : ne;
            e = ne;
            if (i < 8) h0 = __builtin_amdgcn_alignbit(e, h0, 4);
            else h1 = __builtin_amdgcn_alignbit(e, h1, 4);
        }
        const uint32_t pos0 = p0 - skip; // (mod 2^32: chars before the row carry code 0 and are never filed)
        decode(h0, pos0);
        if (CPP > 8) decode(h1, pos0 + 8u);
    };

    // Walk the window at w (its bytes are in LDS): this lane's blocks of [max(rs, w), min(re, w + kWin)).
    auto walk_window = [&](uint64_t w) __attribute__((always_inline)) {
        const uint64_t lo = rs > w ? rs : w;
        const uint64_t hi = re < w + kWin ? re : w + kWin;
        if (lo < hi) {
            const uint32_t kb0 = (uint32_t)(lo - w) >> 4, kb1 = (uint32_t)(hi - 1u - w) >> 4;
            // window start - origin in chars (both 16-byte aligned: exact; negative when the row starts inside the window)
            const uint32_t relc = (uint32_t)((int64_t)(w - (rs & ~(uint64_t)15)) / CW);
            {
                const u32x4 c = *(const lds_u32x4 *)(uintptr_t)win.at(kb0 * 16u);
                walk_block(c, relc + kb0 * CPP, std::true_type{});
            }
            if (kb1 > kb0) {
                u32x4 v = *(const lds_u32x4 *)(uintptr_t)win.at((kb0 + 1u) * 16u);
                for (uint32_t kb = kb0 + 1u; kb < kb1; ++kb) {
                    const u32x4 c = v;
                    v = *(const lds_u32x4 *)(uintptr_t)win.at((kb + 1u) * 16u); // next block: its latency hides below
                    walk_block(c, relc + kb * CPP, std::false_type{});
                }
                walk_block(v, relc + kb1 * CPP, std::true_type{});
            }
        }
    };

    auto finish_rows = [&](uint64_t grp) __attribute__((always_inline)) {
        const uint32_t len = rem - skip;
        // the row's end: the PAD transition of a row that ended on a block boundary (one that ended inside a block took it there and
        // sits in the dead state, whose PAD entry is 0)
        const uint32_t ee = lds_u16(__umul24(e >> 4, wk.ncols_e) + pad_addr);
        const uint32_t code = ee & 15u;
        if (RUNS) {
            if (__ballot(code != 0u) != 0ull) {
                if (fa.count_only) count += code & 1u;
                else put((code & 1u) != 0u, run_start, len);
            }
        } else if (__ballot(code != 0u) != 0ull) {
            file(code != 0u, len, lds_u32(codes_off + (code << 2)));
        }
        if (row_ok && fa.counts) fa.counts[(grp << 6) + (uint64_t)lane] = too_long ? 0u : (count < cap ? count : cap);
        if (__ballot(row_ok && !too_long && count > cap) != 0ull && lane == 0) *fa.more = 1;
        if (pf.too_long && __ballot(row_ok && too_long) != 0ull && lane == 0) *pf.too_long = 1;
    };

    packed_stream<CW, CHB>(lane, wave, n_waves, a.rows, pf.row_offsets, n_rows, win, rs, re, begin_group, walk_window,
                           []() __attribute__((always_inline)) { return true; }, [&]() __attribute__((always_inline)) { return rs; }, finish_rows);
}

template <int CW, int CHB, bool RUNS>
static hipError_t launch_packed_find_all_one(const PackedFindAllArgs &a, int grid, int waves, size_t lds, hipStream_t stream) {
    auto k = packed_find_all_kernel<CW, CHB, RUNS>;
    static thread_local uint64_t configured = 0;
    if (hipError_t e = allow_full_lds((const void *)k, configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(waves * 64), lds, stream, a);
    return hipGetLastError();
}

// (8-bit rows: 64-byte windows per lane only -- with 128 the 16-char blocks' lookups and the window's 32 registers spill)
template <int CW>
static hipError_t launch_packed_find_all_w(const PackedFindAllArgs &a, int chb, int grid, int waves, size_t lds, hipStream_t s) {
    if constexpr (CW == 1) {
        if (chb != 64) return hipErrorInvalidValue;
        if (a.f.s.hdr.ft_on == 2u) return launch_packed_find_all_one<1, 64, true>(a, grid, waves, lds, s);
        return launch_packed_find_all_one<1, 64, false>(a, grid, waves, lds, s);
    } else {
        if (a.f.s.hdr.ft_on == 2u)
            return chb == 128 ? launch_packed_find_all_one<CW, 128, true>(a, grid, waves, lds, s) : launch_packed_find_all_one<CW, 64, true>(a, grid, waves, lds, s);
        return chb == 128 ? launch_packed_find_all_one<CW, 128, false>(a, grid, waves, lds, s) : launch_packed_find_all_one<CW, 64, false>(a, grid, waves, lds, s);
    }
}

} // namespace needle
