// needle_ngram_packed.h -- containedIn() / find() of PACKED row batches (needle_packed_view: one buffer of code units + offsets[n + 1])
// behind the n-gram candidate filter: the filter kernel of needle_ngram.hip (needle_ngram_kernel.h, PACKED = true) and its launch
// templates.  Included by one translation unit per reference loop and char width (needle_ngram_packed_*.hip), which compile in parallel;
// the fixed-stride instantiations (needle_ngram.hip) and the plain packed kernels (needle_packed.h) keep their code and registers.
//
// The filter owns no rows -- a lane tests the windows that end in the 16 chars IT loaded -- so a packed batch, which is one stream of
// text already, needs no transposition.  What differs from the fixed-stride form:
//
//   Rows to waves.  A wave owns 64 consecutive rows ("group"), as both existing kernels: one bitmap word, the rows' result slots in
//   LDS.  The group's text is the span [offsets[64g], offsets[64g + 64]); lane l reads its row's two offsets (coalesced, one group
//   ahead), the span's ends come from lanes 0 and 63.  The rows' starts are kept as 32-bit STREAM positions in a 65-dword table per
//   wave in LDS (kNgWaveLdsPacked).
//   Text stream.  Stream position 0 of a group is its first char's address rounded down to 16 chars (absolute: the data pointer is only
//   4-byte aligned); the span streams from there in 1 KiB units -- 64 lanes x 16 chars, UTF-16 narrowed on load or hashed as it stands
//   (WIDE) -- kNgPF units in flight, no branch around a load.  Sampled positions are multiples of S in the STREAM: some phase per row,
//   which the filter's bitmap does not depend on (it holds every window o = 0 .. S - 1 chars ahead of an accept).  A group is a whole
//   number of batches of kNgPF units (at least one, also for an empty span: see "The prefetch cursor" below); units behind the
//   text are loaded (clamped) but not probed.
//   Memory.  A 16-byte block is loaded by the stream only when it holds a byte of [data + offsets[0] * cw, data + offsets[n] * cw):
//   lane offsets are clamped into the batch's first .. last block.  The verify walks and second-level windows read 16 chars
//   unaligned, clamped to start at most 16 chars before the batch's end and never before its start: nothing outside the batch is read.
//   Candidate to row.  A window's end (stream position) finds its row by six steps of a binary search over the table (the last row
//   that starts at or before the window's last char: empty rows share a start with the row behind them); a window that began in an
//   earlier row (qn < 4) is dropped -- matches are at least 4 + S - 1 chars long, none depends on it.  Rows below 4 chars own none.
//   Verify walks, second level, slots: walk_row / level2 / the 64-bit minimum of needle_ngram_kernel.h, on the row's own pointer.
//   Long rows.  The fixed-stride kernel's slot key holds 16-bit positions; here a row may have up to 2^31 - 1 chars and the answers
//   must be exact int32 in the same call.  Two other ways were tried or weighed: walking a group with a row above 65 534 chars row
//   by row inside this kernel (measured, profiles/packed_prefilter.md: 247 ms against the plain kernel's 73 ms on the long-row batch
//   -- one lane re-reading its row 16 chars at a time with nothing to hide the latency), and marking such groups for a second launch
//   of the plain packed kernel (a launch more per call and a variant more of every plain kernel).  Neither is needed: the packed
//   kernel's key is first accept (32 bits) | last - first (16) | match length (16) -- a lengths program's matches are at most 255
//   chars and a one-length pattern's at most 65 535 (run_packed_dev checks), so the key holds every row position -- and stream
//   positions are 32 bits.  A long row is then filtered like any other text: its wave streams it at the filter's pace, 64 lanes wide
//   (0.44 ms on that batch).  Only a group whose span exceeds 2^31 - 1 chars (NgramArgs::pk_direct_above) is DIRECT: no filter, every
//   lane walks its own row whole (walk_row from char 0, unaligned 16-char reads clamped into the batch), results straight from the
//   walk as exact int32, at one lane's pace per row as in the plain packed kernel.  More than 2 GiB of text in 64 rows is not
//   something a test can hold: NEEDLE_PACKED_DIRECT_ABOVE lowers the threshold so that tests walk ordinary groups that way.
//   The prefetch cursor.  It stands up to two batches ahead of the batch being filtered.  A group is at least one batch, so the
//   cursor is in the current group, this wave's next one, or -- when the next has a single batch -- the one after that: the rows'
//   offsets are therefore held for three groups (cur / nxt / nn) and asked for two groups ahead.
//   Tiny batches.  The host never sees the offsets, so the kernel is right for any amount of text: below 16 chars in all no 16-char
//   read fits the batch -- every group is direct and its chars are read one guarded load each; the stream's loads read the program
//   blob instead (no branch around a load) and nothing is probed.
//
// Served: containedIn() and find() with a lengths form or a fixed length -- 8-bit rows on LDS programs (table8, table16, compressed)
// and on walks out of HBM (MODE_GLOBAL), UTF-16 rows of one-page patterns (byte program of the page, narrowed on load) and of
// multi-page patterns (WIDE) -- with int32 pairs or the one-word forms (pack16_or_over / pack8_or_over + overflow flag).
// Find-all (OP_NG_FIND_ALL, needle_ngram_packed_find_all{1,2}.hip; count / CSR entries of big dictionaries): stream, offsets, candidate
// location and direct groups as above; filing and the group's end are the fixed-stride find-all form's (needle_ngram_kernel.h run_rows:
// two slots + a counter per row, lane = row sorts its candidates against its moving cursor, re-runs a window from the cursor, falls to
// the match-by-match loop).  The filed entry is 64 bits for rows of any length: window end (32, on top) | first - end (8, 0xFF: unknown) |
// 24 bits bounded by the pattern -- one length: last - end; a lengths program: last - end (16) and the match length (8).  A direct group
// runs the match-by-match loop on every row from char 0.  LDS per wave: kNgWaveLdsPackedFA (64 row starts: the position behind the last
// row is the group's end, held in a register).
// NOT served, these keep the plain packed kernels: matches() (the filter never serves it), per-row cursors
// (needle_find_next_packed_dev), find() of patterns without bounded match lengths (the fixed-stride variant
// 12 with backward walks has no packed form), and the *_packed_host entries' routing is unchanged.
#pragma once
#include "needle_ngram_kernel.h"

namespace needle {

template <int OP, int MODE, int S, int CW, bool WIDE = false>
__global__ __launch_bounds__(kWavesPerBlock * 64) void ngram_packed_kernel(const NgramArgs A) {
    ngram_body<OP, MODE, S, CW, WIDE, false, true>(A);
}

template <int OP, int MODE, int S, int CW, bool WIDE = false>
static hipError_t launch_ngp(const NgramArgs &A, int n_cus, size_t lds, hipStream_t stream) {
    auto k = ngram_packed_kernel<OP, MODE, S, CW, WIDE>;
    static thread_local uint64_t configured = 0;
    if (hipError_t e = allow_full_lds((const void *)k, configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(n_cus), dim3(kWavesPerBlock * 64), lds, stream, A);
    return hipGetLastError();
}

// one op x char width: the program's mode and the filter's stride
template <int OP, int CW>
static hipError_t launch_ngp_m(const NgramArgs &A, int n_cus, size_t lds, hipStream_t stream) {
    const bool s4 = A.ng.stride == 4;
    if (A.ng.wide) {
        if constexpr (CW == 2) {
            if (A.a.hdr.mode != MODE_GLOBAL) return hipErrorInvalidValue;
            return s4 ? launch_ngp<OP, MODE_GLOBAL, 4, 2, true>(A, n_cus, lds, stream) : launch_ngp<OP, MODE_GLOBAL, 2, 2, true>(A, n_cus, lds, stream);
        }
        return hipErrorInvalidValue;
    }
    switch (A.a.hdr.mode) {
    case MODE_TABLE8: return s4 ? launch_ngp<OP, MODE_TABLE8, 4, CW>(A, n_cus, lds, stream) : launch_ngp<OP, MODE_TABLE8, 2, CW>(A, n_cus, lds, stream);
    case MODE_TABLE16: return s4 ? launch_ngp<OP, MODE_TABLE16, 4, CW>(A, n_cus, lds, stream) : launch_ngp<OP, MODE_TABLE16, 2, CW>(A, n_cus, lds, stream);
    case MODE_SPARSE: return s4 ? launch_ngp<OP, MODE_SPARSE, 4, CW>(A, n_cus, lds, stream) : launch_ngp<OP, MODE_SPARSE, 2, CW>(A, n_cus, lds, stream);
    case MODE_GLOBAL: return s4 ? launch_ngp<OP, MODE_GLOBAL, 4, CW>(A, n_cus, lds, stream) : launch_ngp<OP, MODE_GLOBAL, 2, CW>(A, n_cus, lds, stream);
    default: return hipErrorInvalidValue;
    }
}

} // namespace needle
