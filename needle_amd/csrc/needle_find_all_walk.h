// needle_find_all_walk.h -- the walk of the per-lane find-all kernels, stated once for both row layouts: find_all_kernel
// (needle_find_all.hip, fixed-stride rows) and packed_find_all_lane_kernel (needle_packed_find_all_lane.h, packed rows).  The kernels
// differ in how text reaches LDS and where results go; each says so in a small `Rows` policy next to its staging code.  Here:
// the walk constants (find_all_walk_setup), one 16-byte piece (walk_piece_fa), what a lane does with its piece -- the reference's
// repeated Matcher.find(), DFAClassBuilder.java:616-659 (find_all_lane_step) -- and the deferred starts (find_all_starts_phase).
// Positions are ORIGIN-relative chars: the origin is the 16-byte block the row starts in, rows.skip the chars of that block in front
// of the row (fixed-stride rows start on a block: a compile-time 0).  Filed results are row-relative (- rows.skip).
//
// A Rows policy (an aggregate of scalars, built where it is used and inlined away) has:
//   skip                         chars of the origin block in front of the lane's row
//   file_match(out0, k, s, en)   file match k of the row whose first result slot is out0: [s, en), row-relative
//   file_end(out0, k, en)        ... only its end;  read_end(out0, k): that end again, by an agent-scope load;
//   file_start(out0, k, s, en)   ... and the start that joins it in find_all_starts_phase
//   backward(act, en, bound)     indexBackwards(en - 1, bound) of the immediate form: the text in LDS as its window
//   owner(grp, l)                FindAllOwner of lane l's row of group grp: its origin block in memory and its skip
//   no_text(en)                  true: a deferred start's text must all come from memory (byte offsets beyond an int32)
//   slot_addr()                  32 free bytes of LDS of this lane, for the text of a deferred start
#pragma once
#include "needle_find_all.h"
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

// The walk constants of a find-all program (staged in LDS) as walk_piece_fa and find_all_lane_step take them.
struct FindAllWalk {
    Walk wk;
    uint32_t accept_lo, start_state;
};
template <int CW, int MODE>
__device__ __forceinline__ void find_all_walk_setup(const ScanArgs &a, int lane, FindAllWalk &fw) {
    Walk &wk = fw.wk;
    constexpr uint32_t ELEM = (MODE == MODE_TABLE16 || MODE == MODE_HYBRID) ? 2u : 1u;
    wk.ncols_e = a.hdr.n_cols * ELEM;
    wk.pad_e = (MODE == MODE_PACK) ? a.hdr.pad_f : a.hdr.pad_col * ELEM;
    wk.pre_e = (MODE == MODE_PACK) ? a.hdr.pre_f : (a.hdr.pad_col + 1u) * ELEM;
    wk.pad_b = wk.pre_b = 0;
    wk.table_off = a.hdr.off_table;
    wk.win_on = 0, wk.win_lo = 0, wk.win_hi = 0; // (the find-all programs are lowered without window addressing)
    wk.sp_chains = 0, wk.sp_pad_ident = 0, wk.dead_hi = 0;
    wk.flat = (CW == 2 && (MODE == MODE_TABLE8 || MODE == MODE_TABLE16)) ? a.hdr.flat_pages : 0u;
    if ((MODE == MODE_TABLE8 || MODE == MODE_TABLE16) && a.hdr.win_on) { // a lengths program in window layout (needle_scan.h sets these up the same way)
        wk.win_on = 1, wk.win_lo = a.hdr.win_lo_e, wk.win_hi = a.hdr.win_hi_e;
        wk.table_off = a.hdr.off_table - a.hdr.win_lo_e;
    }
    if constexpr (MODE == MODE_SPARSE) { // the scan kernels' compressed lengths program (needle_scan.h sets these up the same way)
        wk.pad_e = wk.pre_e = a.hdr.win_lo_e;
        wk.win_on = a.hdr.win_on, wk.win_lo = a.hdr.win_lo_e, wk.win_hi = a.hdr.win_hi_e;
        wk.dead_hi = a.hdr.fa_dead_hi;
        wk.sp_chains = a.hdr.sp_chains, wk.sp_pad_ident = a.hdr.sp_pad_ident;
    }
    wk.lane4 = (uint32_t)lane * 4u; // packed mode on 8-bit rows: all 64 lane copies of F are there (no tiles in the F rows)
    wk.gtable = (const uint16_t *)(a.prog + (MODE == MODE_HYBRID ? a.hdr.off_gtable : a.hdr.off_table));
    wk.hot_last = a.hdr.hot_bytes - 2u;
    fw.accept_lo = MODE == MODE_PACK ? a.hdr.accept_off : a.hdr.accept_lo;
    fw.start_state = MODE == MODE_PACK ? a.hdr.start_off : a.hdr.start;
}

// A lane's row in the walk.  Positions are origin-relative chars.
struct FindAllRow {
    uint32_t st, pi, count; // automaton state; index of the lane's current 16-byte piece; matches filed (or counted) so far
    int32_t last, cursor;   // end of the last accepting prefix of this search (-1: none); where this search started
    bool done;              // nothing more to find in this row
    uint64_t out0;          // index of the row's first result slot
    uint32_t cap;           // matches this row may file
    uint32_t len;           // the row's end
};
struct FindAllOwner { const uint8_t *text; uint32_t skip; }; // a row's origin block in memory, and its Rows::skip

// One lane, one piece: w holds piece r.pi (chars p0 = r.pi * CPP on) of an `active` lane's row; the others take part idle.
// This is straight-line code for all 64 lanes -- idle lanes walk a piece too and their results are dropped by selects: every
// divergent region here costs the compiler a copy of the loop-carried lane state per path, and with it more VALU ops than the
// walk itself.  After a match [start, end) the search restarts AT `end` (r.cursor), in the piece holding it (r.pi steps back).
template <int CW, int MODE, bool LM, class Rows>
__device__ __forceinline__ void find_all_lane_step(const FindAllArgs &fa, const FindAllWalk &fw, const Rows &rows, const uint32_t (&w)[4],
                                                   bool active, uint32_t p0, FindAllRow &r) {
    const ScanArgs &a = fa.s;
    const Walk &wk = fw.wk;
    constexpr int CPP = 16 / CW; // chars per 16-byte piece
    const uint32_t start_state = fw.start_state;
    const int32_t skip = (int32_t)rows.skip;
    const uint32_t skip_rel = (uint32_t)r.cursor > p0 ? (uint32_t)r.cursor - p0 : 0u; // < CPP: the cursor's piece, or none
    const uint32_t st_old = r.st;
    uint32_t st_new = r.st;
    const uint32_t in_row = r.len > p0 ? r.len - p0 : 0u; // chars of the piece inside the row (all, if >= CPP)
    uint32_t acc = walk_piece_fa<CW, MODE, false, LM>(wk, w, skip_rel, fw.accept_lo, st_new, in_row);
    if (!LM) acc &= ~((1u << skip_rel) - 1u);          // an accepting start state does not count before the cursor
    acc &= in_row < (uint32_t)CPP ? (1u << in_row) - 1u : 0xFFFFFFFFu;
    acc = active ? acc : 0u;
    r.last = acc ? (int32_t)(p0 + 32u - (uint32_t)__builtin_clz(acc)) : r.last;
    r.st = active ? st_new : r.st;
    // (fa_dead_n: the "lengths" automaton's dead-with-a-match-pending states; 0 for every other program)
    const bool died = MODE == MODE_SPARSE ? st_new <= wk.dead_hi : (st_new == 0u || st_new - a.hdr.fa_dead_lo < a.hdr.fa_dead_n);
    const bool ended = active && (died || p0 + CPP >= r.len);
    r.pi += (active && !ended) ? 1u : 0u;
    if (__ballot(ended) == 0ull) return;
    // ---- find() returns for the lanes of `ended` (:629-657)
    const bool hit = ended && r.last >= 0;
    const int32_t en = r.last;
    if (ended && !hit) r.done = true; // no further match in this row
    if (LM || fa.lmode) {
        // The "lengths" automaton (needle_lower.h): the state the search ended in remembers how long its last match
        // was -- start = end - pend[state], no indexBackwards (DFAClassBuilder.java:640-646 generalised per state).
        // A ragged row that ends INSIDE this piece was walked past its end above (harmless for the flags, which are
        // masked, but not for the state): that piece is walked again from its entry state with the PAD column.
        uint32_t st_end = st_new;
        if (MODE == MODE_TABLE8 || MODE == MODE_TABLE16) { // (the only modes such a program has)
            const bool cut = hit && in_row < (uint32_t)CPP;
            if (__ballot(cut) != 0ull) {
                uint32_t st_fix = st_old;
                (void)walk_piece_fa<CW, MODE, true, LM>(wk, w, skip_rel, fw.accept_lo, st_fix, in_row);
                st_end = cut ? st_fix : st_end;
            }
        }
        if (MODE == MODE_SPARSE) { // a live end state (the row ended) asks its END record for the D_L of its pending length
            const uint32_t e_st = sparse_end<CW>(wk, st_new, hit && st_new > wk.dead_hi, a.hdr.sp_end_col4);
            st_end = (e_st & 0xFFFFu) - a.hdr.sp_dead_row0;
        }
        const int32_t mlen = (int32_t)lds_u8(a.hdr.fa_len_off + (hit ? st_end : 0u));
        const bool file = hit && r.count < r.cap;
        if (hit && !file) *fa.more = 1;
        r.done = r.done || (hit && !file);
        if (file && !fa.count_only) rows.file_match(r.out0, r.count, en - mlen - skip, en - skip);
        r.count += file ? 1u : 0u;
        r.cursor = file ? en : r.cursor;
        const uint32_t pi_en = ((uint32_t)en * CW) >> 4;
        uint32_t st_again = start_state;
        if (LM) { // en - pi_en * CPP chars of the piece lie before the new cursor: S_k swallows them
            const uint32_t rel = (uint32_t)en - pi_en * (uint32_t)CPP;
            st_again = rel ? a.hdr.fa_skip_lo + rel - 1u : start_state;
        }
        r.st = file ? st_again : r.st;
        r.last = file ? -1 : r.last;
        r.pi = file ? pi_en : r.pi;
    } else if (fa.defer) {
        // not nullable, start by indexBackwards: the match is not empty and ends beyond its cursor -- the row goes on.
        // Written as selects, not branches: this block runs in most iterations (some lane of 64 has just resolved)
        // and every divergent branch costs a copy of the loop-carried lane state per path.
        const bool file = hit && r.count < r.cap;
        if (hit && !file) *fa.more = 1;
        r.done = r.done || (hit && !file);
        if (file && !fa.count_only) rows.file_end(r.out0, r.count, en - skip); // (counting: nothing is filed)
        r.count += file ? 1u : 0u;
        r.cursor = file ? en : r.cursor;
        r.st = file ? start_state : r.st;
        r.last = file ? -1 : r.last;
        r.pi = file ? (((uint32_t)en * CW) >> 4) : r.pi;
    } else {
        int32_t s = en - a.fixed_len;
        if (a.fixed_len < 0) s = rows.backward(hit, en, r.cursor);
        // en < s: the wrapped pseudo-match of a nullable pattern searched from cursor == length; dropped, ends the row
        const bool valid = hit && en >= s;
        if (hit && !valid) r.done = true;
        if (valid) {
            if (r.count < r.cap) {
                if (!fa.count_only) rows.file_match(r.out0, r.count, s - skip, en - skip);
                ++r.count;
                // the row goes on only while the cursor advances (needle_hip.h)
                if (en == s || en <= r.cursor) {
                    r.done = true;
                } else {
                    r.cursor = en;
                    r.st = start_state;
                    r.last = a.hdr.root_accepting ? (((uint32_t)r.cursor < r.len) ? r.cursor : skip) : -1;
                    r.pi = ((uint32_t)en * CW) >> 4;
                }
            } else {
                *fa.more = 1;
                r.done = true;
            }
        }
    }
}

// fa.defer != 0: the starts of a 64-row group's matches, found at the end of the group.  indexBackwards (:529-586) at the moment a
// lane resolves would run the backward walk's code for the one or two lanes resolving in any given iteration, so the walk files only
// the ENDS.  Match k of a row was searched from the end of match k - 1: every start is an independent indexBackwards, and the
// matches of the 64 rows are numbered through (prefix sum of the counts) and handed out 64 at a time, one per lane, whichever row
// they belong to -- no lane waits for another row's longer list.  The text (the piece holding char end - 1 and the one before it,
// not below the origin block) comes back from memory / L2 into the lane's by now free rows.slot_addr(); the ends are read back with
// agent-scope loads (this wave wrote them a moment ago: the plain stores are in L2 once vmcnt says so, a plain load might still hit
// a stale L1 line).  Patterns that match the empty string need every start at once -- an empty match ends its row
// (needle_find_all_dev in needle_hip.h) -- and take the immediate form of find_all_lane_step.
// (Tried before: a register stack of pending ends flushed tile by tile with the text still in LDS -- a round per pending match of
// the busiest lane and tile: dictionary 3.3 ms against 2.6; the same rounds as a kernel of its own: 3.0 ms, its re-reads of ends
// and text all miss the L2.)
template <int CW, class Rows>
__device__ __forceinline__ void find_all_starts_phase(const FindAllArgs &fa, const Rows &rows, int lane, uint64_t grp, const FindAllRow &r) {
    uint32_t incl = r.count;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, o);
        incl += lane >= o ? t : 0u;
    }
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    if (total == 0u) return;
    const uint32_t excl = incl - r.count;
    const uint32_t slot = rows.slot_addr();
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
        const uint32_t k = j - (uint32_t)__builtin_amdgcn_ds_bpermute((int)(owner << 2), (int)excl);
        const uint64_t o_out0 = (uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute((int)(owner << 2), (int)(uint32_t)r.out0) |
                                ((uint64_t)(uint32_t)__builtin_amdgcn_ds_bpermute((int)(owner << 2), (int)(uint32_t)(r.out0 >> 32)) << 32);
        const FindAllOwner o = rows.owner(grp, owner);
        int32_t en = 1, bound = 0; // row-relative
        if (act) {
            en = rows.read_end(o_out0, k);
            if (k) bound = rows.read_end(o_out0, k - 1u);
        }
        const int32_t en_o = en + (int32_t)o.skip, bound_o = bound + (int32_t)o.skip; // origin-relative
        const uint32_t pa = ((uint32_t)(en_o - 1) * CW) >> 4; // text: the piece holding char en - 1 and the one before it
        const uint32_t pb = pa ? pa - 1u : 0u;
        u32x4 va = {0, 0, 0, 0}, vb = {0, 0, 0, 0};
        if (act) { // (en >= 1: both pieces lie between the origin block and the piece of char en - 1 -- each holds a char of the row)
            va = *(const u32x4 *)(o.text + ((uint64_t)pa << 4));
            vb = *(const u32x4 *)(o.text + ((uint64_t)pb << 4));
        }
        *(lds_u32x4 *)(uintptr_t)(slot) = vb;
        *(lds_u32x4 *)(uintptr_t)(slot + 16u) = va;
        const uint32_t t_b0 = pa ? pb * 16u : 0u;
        const uint32_t t_addr = pa ? slot : slot + 16u;
        const uint32_t t_bytes = rows.no_text(en_o) ? 0u : (pa ? 32u : 16u);
        const int32_t st_o = fa.defer == 2u ? bound_o : backward_walk<CW>(fa.s, act, en_o, bound_o, t_addr, t_b0, t_bytes, 0u, o.text); // (2: measurement aid)
        if (act) rows.file_start(o_out0, k, st_o - (int32_t)o.skip, en);
    }
}

} // namespace needle
