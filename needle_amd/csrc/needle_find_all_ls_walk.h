// needle_find_all_ls_walk.h -- the walk of the lock-step find-all kernel of fixed-stride rows (find_all_lockstep_kernel,
// needle_find_all_ls.hip), apart from its staging: the kernel keeps its tiles and says where a match is filed in a small `Rows` policy.
// Written for both row layouts, but packed_find_all_kernel (needle_packed_find_all.h) keeps a copy of this walk on its own variables:
// over these structs it measured 0.4-0.8 % slower on three of its four rate figures (profiles/find_all_packed.md).  A fix here is a fix
// to make there too.  Here: the walk constants of a transducer program staged in LDS (find_all_ls_setup), one 16-byte block of a lane's row -- the transition
// chain and its two logs (find_all_ls_block) --, what a log word's match codes mean (find_all_ls_decode) and the row's end, the one
// PAD transition (find_all_ls_row_end).
//
// A Rows policy (an aggregate of scalars, built where it is used and inlined away) has:
//   file_code(k, pos, d)   file match k of the lane's row: filed at char index pos with d = codes[code] = (k' + length) | k' << 16
//                          (needle_device.h) -- the match [pos - (k' + length), pos - k')
//   file_span(k, st, en)   file match k of the lane's row: [st, en) as it stands
#pragma once
#include "needle_find_all.h"
#include "needle_walk.h"

namespace needle {

// The walk constants of a find-all transducer program (lengths or RUN transducer, staged in LDS).
struct LsWalk {
    Walk wk;
    uint32_t tbase;     // added to a column on the chain (UTF-16: piece_lookups has added the table's offset to the columns)
    uint32_t pad_addr;  // the PAD column, as the chain addresses it
    uint32_t codes_off; // codes[16] in LDS: d of a match code
    uint32_t e_start;   // the entry a row starts with
    uint32_t ft_direct; // wave-uniform: != 0: codes are lengths, k = 0 -- 1: code == length, 2: code == length << 1 | 1
    uint32_t ft_odd;    // wave-uniform: at most 8 codes, all odd -- bit 0 of a nibble = "a match ends here"
};
template <int CW>
__device__ __forceinline__ void find_all_ls_setup(const ScanArgs &a, LsWalk &lw) {
    Walk &wk = lw.wk;
    wk.ncols_e = a.hdr.n_cols * 2u;
    wk.pad_e = a.hdr.pad_col * 2u;
    wk.pre_e = wk.pad_e; // (never taken: no cursors here, and the programs have no PRE column)
    wk.pad_b = wk.pre_b = 0;
    wk.win_on = a.hdr.win_on, wk.win_lo = a.hdr.win_lo_e, wk.win_hi = a.hdr.win_hi_e;
    wk.table_off = a.hdr.off_table - a.hdr.win_lo_e; // (window addressing: column offsets are not rebased, needle_device.h)
    wk.sp_chains = 0, wk.sp_pad_ident = 0, wk.dead_hi = 0, wk.lane4 = 0, wk.gtable = nullptr, wk.hot_last = 0;
    wk.flat = 0;
    lw.tbase = CW == 1 ? (uint32_t)kLdsTable1 : 0u;
    lw.pad_addr = wk.pad_e + (CW == 1 ? (uint32_t)kLdsTable1 : wk.table_off);
    lw.codes_off = a.hdr.ft_codes_off;
    lw.e_start = a.hdr.start << 4;
    lw.ft_direct = a.hdr.ft_direct;
    lw.ft_odd = a.hdr.ft_odd;
}

// A lane's row in the walk.
struct LsRow {
    uint32_t e;         // the transducer entry: state << 4 | match code
    uint32_t run_start; // RUN transducer: row index of the last char that may have begun a run
    uint32_t count;     // matches of this row so far -- ALL of them; the first `cap` are filed
    uint32_t cap;       // matches this row may file
};

// One match of the lanes of `hit`: filed while the row has room, counted always.
template <class Rows>
__device__ __forceinline__ void find_all_ls_file_code(const FindAllArgs &fa, const Rows &rows, bool hit, uint32_t pos, uint32_t d, LsRow &r) {
    if (hit && r.count < r.cap && !fa.count_only) rows.file_code(r.count, pos, d);
    r.count += hit ? 1u : 0u;
}
// (the RUN transducer: a run's length is not bounded by 16 bits the way (length, k) codes are)
template <class Rows>
__device__ __forceinline__ void find_all_ls_file_span(const FindAllArgs &fa, const Rows &rows, bool hit, uint32_t st, uint32_t en, LsRow &r) {
    if (hit && r.count < r.cap && !fa.count_only) rows.file_span(r.count, st, en);
    r.count += hit ? 1u : 0u;
}

// The match codes of 8 consecutive chars: char j of them in nibble j of h; pos0 = row index of char 0.  Matches are filed a lane at a
// time where there are any -- the walk itself never branches on them.
// RUNS (the run transducer, needle_lower.h lower_find_all_runs): a code's bit 0 says "a match ends in front of this char", bit 1 "this
// char may begin a run"; the lane keeps the index of the last char that could (run_start) -- brought up to date from the log's bit-1
// nibbles (four VALU ops) -- and a match ending at char i starts at the last such char below i.  No lengths, no backward walk
// (DFAClassBuilder.java:529-586 finds the same start: the lowering proved it on the tables).
// Otherwise (the lengths transducer): a non-zero nibble at char j with codes[code] = (length, k) is the match [end - length, end),
// end = index(j) - k (k chars lie between a match's last char and the char that killed its walk).
template <bool RUNS, class Rows>
__device__ __forceinline__ void find_all_ls_decode(const FindAllArgs &fa, const LsWalk &lw, const Rows &rows, uint32_t h, uint32_t pos0, LsRow &r) {
    if (RUNS) {
        uint32_t t = h & 0x11111111u;              // bit 4j: a match ends in front of char j
        const uint32_t tf = (h >> 1) & 0x11111111u; // bit 4j: char j may begin a run
        if (fa.count_only) {
            r.count += (uint32_t)__builtin_popcount(t);
            return;
        }
        if (__ballot(t != 0u) != 0ull) {
            do {
                const bool has = t != 0u;
                uint32_t b;
                asm("v_ffbl_b32 %0, %1" : "=v"(b) : "v"(t));
                t &= t - 1u;
                const uint32_t below = tf & ((1u << (b & 31u)) - 1u); // the chars of this log in front of the match's end
                const uint32_t st = below ? pos0 + ((31u - (uint32_t)__builtin_clz(below)) >> 2) : r.run_start;
                const uint32_t en = pos0 + ((b & 31u) >> 2);
                find_all_ls_file_span(fa, rows, has, st, en, r);
            } while (__ballot(t != 0u) != 0ull);
        }
        r.run_start = tf ? pos0 + ((31u - (uint32_t)__builtin_clz(tf)) >> 2) : r.run_start;
        return;
    }
    if (__ballot(h != 0u) == 0ull) return;
    uint32_t t = h; // bit 4j: char j ends a match
    if (!lw.ft_odd) {
        t |= t >> 1;
        t |= t >> 2;
    }
    t &= 0x11111111u;
    if (fa.count_only) { // wave-uniform: nothing is filed, no limit
        r.count += (uint32_t)__builtin_popcount(t);
        return;
    }
    if (lw.ft_direct) { // wave-uniform: the code names the match's length, k = 0 -- no lookup on the filing chain
        const uint32_t hl = lw.ft_direct == 2u ? h >> 1 : h; // (2: length << 1 | 1)
        do {
            const bool has = t != 0u;
            uint32_t b; // bit index of the next match's nibble (lanes that have none: 0xFFFFFFFF -- nothing filed)
            asm("v_ffbl_b32 %0, %1" : "=v"(b) : "v"(t));
            t &= t - 1u;
            find_all_ls_file_code(fa, rows, has, pos0 + (b >> 2), __builtin_amdgcn_ubfe(hl, b, lw.ft_direct == 2u ? 3u : 4u), r);
        } while (__ballot(t != 0u) != 0ull);
        return;
    }
    do {
        const bool has = t != 0u;
        uint32_t b;
        asm("v_ffbl_b32 %0, %1" : "=v"(b) : "v"(t));
        t &= t - 1u;
        const uint32_t d = lds_u32(lw.codes_off + (__builtin_amdgcn_ubfe(h, b, 4) << 2));
        find_all_ls_file_code(fa, rows, has, pos0 + (b >> 2), d, r);
    } while (__ballot(t != 0u) != 0ull);
}

// One 16-byte block w of the lane's row: ONE dependent table lookup per char,
//     entry = T[(entry >> 4) * row_bytes + column(char)]        (v_lshrrev, v_mad_u32_u24, ds_read_u16)
//     log   = {entry, log} >> 4                                 (v_alignbit: the entry's low 4 bits = the match code, 0 = none)
// and after 8 chars the log's 8 codes are decoded.  p0: index of the block's first char as piece_lookups counts it against `rem` (GUARD:
// chars at or after rem take the PAD column); pos0: its row index.  Rows start on a block: no select on the chain (the packed rows'
// copy has one for the chars in front of a row).
template <int CW, bool GUARD, bool RUNS, class Rows>
__device__ __forceinline__ void find_all_ls_block(const FindAllArgs &fa, const LsWalk &lw, const Rows &rows, const uint32_t (&w)[4], uint32_t p0,
                                                  uint32_t rem, uint32_t pos0, LsRow &r) {
    constexpr int CPP = 16 / CW; // chars per 16-byte block
    uint32_t col[CPP];
    piece_lookups<MODE_TABLE16, CW, GUARD>(lw.wk, w, p0, rem, 0u, col);
    uint32_t h0 = 0, h1 = 0;
#pragma unroll
    for (int i = 0; i < CPP; ++i) {
        r.e = lds_u16(__umul24(r.e >> 4, lw.wk.ncols_e) + col[i] + lw.tbase);
        if (i < 8) h0 = __builtin_amdgcn_alignbit(r.e, h0, 4);
        else h1 = __builtin_amdgcn_alignbit(r.e, h1, 4);
    }
    find_all_ls_decode<RUNS>(fa, lw, rows, h0, pos0, r);
    if (CPP > 8) find_all_ls_decode<RUNS>(fa, lw, rows, h1, pos0 + 8u, r);
}

// The row's end (len: its chars): one more transition, on the PAD column -- a pending match is emitted.  Rows that ended inside a block
// took it there and sit in the dead state, whose PAD entry is 0.
template <bool RUNS, class Rows>
__device__ __forceinline__ void find_all_ls_row_end(const FindAllArgs &fa, const LsWalk &lw, const Rows &rows, uint32_t len, LsRow &r) {
    const uint32_t ee = lds_u16(__umul24(r.e >> 4, lw.wk.ncols_e) + lw.pad_addr);
    const uint32_t code = ee & 15u;
    if (RUNS) {
        if (__ballot(code != 0u) != 0ull) {
            if (fa.count_only) r.count += code & 1u;
            else find_all_ls_file_span(fa, rows, (code & 1u) != 0u, r.run_start, len, r);
        }
    } else if (__ballot(code != 0u) != 0ull) find_all_ls_file_code(fa, rows, code != 0u, len, lds_u32(lw.codes_off + (code << 2)), r);
}

} // namespace needle
