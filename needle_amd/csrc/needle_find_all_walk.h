// needle_find_all_walk.h -- the per-char walk of one 16-byte piece in the per-lane find-all kernels: find_all_kernel (needle_find_all.hip,
// fixed-stride rows) and packed_find_all_lane_kernel (needle_packed_find_all_lane.h, packed rows).
#pragma once
#include "needle_walk.h"

namespace needle {

// One 16-byte piece of one row in the find-all walk.  Chars before the lane's cursor (the first skip_rel of the piece)
// go through the PRE column (identity); chars past the row's end are walked like any others -- the search ends with
// that piece whatever its state is, and the caller masks their accept flags.  Accept flags are LOGGED, one shift per
// char (walk_piece selects a position per char: three VALU ops in a walk that is issue-bound under its guards):
// returns the flags of the piece's chars, char i at bit i.
// CUT (the "lengths" form on the piece a ragged row ends in): chars from in_row on take the PAD column, which there leads
// to the dead state that remembers the pending match -- the state the piece ends in is then the one the ROW ends in.
// SKIPST (programs with skip states, needle_device.h fa_skip_lo): no cursor guard at all -- a search restarted inside the piece
// enters it in the skip state that swallows the chars before its cursor.
template <int CW, int MODE, bool CUT = false, bool SKIPST = false>
__device__ __forceinline__ uint32_t walk_piece_fa(const Walk &wk, const uint32_t (&w)[4], uint32_t skip_rel, uint32_t accept_lo,
                                                  uint32_t &st, uint32_t in_row = 0) {
    constexpr int CPP = 16 / CW;
    uint32_t col[CPP];
    piece_lookups<MODE, CW, false>(wk, w, 0, 0, 0, col);
    const uint32_t tb_in_col = col_has_table_off<MODE, CW>() ? wk.table_off : 0u; // (UTF-16 table programs: needle_walk.h)
    if (MODE == MODE_PACK) lds_fence();
    if (MODE == MODE_SPARSE) {
        // The compressed automaton (needle_device.h) has no PRE / PAD columns: chars before the lane's cursor and chars past the
        // row's end (in_row: chars of the piece inside the row) leave the state as it is -- a lengths program's state FREEZES
        // at the row's end and its END record names the pending length (needle_scan.h finish_rows).
        uint32_t h = 0;
#pragma unroll
        for (int i = 0; i < CPP; ++i) {
            const uint32_t ns = apply<MODE, CW>(wk, st, col[i]);
            st = ((uint32_t)i >= skip_rel && (uint32_t)i < in_row) ? ns : st;
            h |= (st >= accept_lo ? 1u : 0u) << i; // (flags of chars outside [skip_rel, in_row) are masked by the caller)
        }
        return h;
    }
    if (CUT) {
#pragma unroll
        for (int i = 0; i < CPP; ++i) col[i] = ((uint32_t)i < in_row) ? col[i] : wk.pad_e + tb_in_col;
    }
    if (!SKIPST) {
#pragma unroll
        for (int i = 0; i < CPP; ++i) col[i] = ((uint32_t)i < skip_rel) ? wk.pre_e + tb_in_col : col[i];
    }
    uint32_t h = 0;
    const uint32_t acc_m1 = accept_lo - 1u;
#pragma unroll
    for (int i = 0; i < CPP; ++i) {
        st = apply<MODE, CW>(wk, st, col[i]);
        if (MODE == MODE_PACK) h = __builtin_amdgcn_alignbit(st, h, 1);                 // accepting states: odd field offsets
        else if (MODE == MODE_HYBRID) h = __builtin_amdgcn_alignbit(h, st << 16, 31);   // accepting: bit 15 of the entry
        else h = __builtin_amdgcn_alignbit(h, acc_m1 - st, 31);                          // accepting: st >= accept_lo
    }
    // packed: char i at bit 32 - CPP + i; the others: char i at bit CPP - 1 - i
    if (MODE != MODE_PACK) h = __builtin_bitreverse32(h);
    return h >> (32 - CPP);
}

} // namespace needle
