// needle_ngram.hip -- containedIn() / find() behind the n-gram candidate filter: hand-written for gfx950.
//
// The ordinary kernel (needle_scan.h) walks the automaton over every char of every row; with an automaton that fills the LDS
// (a 1000-keyword dictionary: 4487 states, 96 KB) that walk is a chain of dependent LDS lookups at 1024 chains per CU and runs
// at 0.30 of the HBM rate.  Here the text is never transposed and no lane owns a row: the batch is one byte stream, a lane
// tests the windows that end in the 16 bytes IT loaded (needle_ngram.h: no dependence between chars), and the automaton only
// runs where a window passes -- one candidate per lane, 64 candidates at a time, K + S - 1 chars each, on text re-read from
// L2 -- from the start state, K chars ahead of the window's end.  What makes that the same answer as the reference's walk from
// the row's start (DFAClassBuilder.java:438-468 indexForwards, :1004-1022 containedIn) is established on the table by
// needle_ngram_host.cpp: a restarted walk has caught up after K chars, and no first accept happens without a window in the bitmap.
//
// Per wave: 64-row groups, as in the scan kernel (one bitmap word per group).  A group is a contiguous run of 64 * stride
// bytes = a whole number of 1 KiB units (stride % 64 == 0: four units per batch); unit u is loaded as 64 lanes x 16 bytes,
// four units in flight.  Candidates -- byte offset of the window's END inside the group -- go to the wave's LDS queue; full
// sets of 64 are run as soon as they exist, the rest at the group's end.  A run that accepts reports (first accepting index,
// end, start) to its row's LDS slot by a 64-bit minimum: several windows of a row may find matches, the reference's is the one
// that accepts first.  find() takes "lengths" programs (start = end - pend[stop state], needle_lower.h) or patterns of one
// length (DFAClassBuilder.java:640-646).
#include <string.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "needle_ngram_kernel.h"
#include "needle_launch.h"

namespace needle {

template <int OP, int MODE>
static hipError_t launch_ng_s(const NgramArgs &A, int n_cus, size_t lds, hipStream_t stream) {
    if (A.char_width == 2) return A.ng.stride == 4 ? launch_ng<OP, MODE, 4, 2>(A, n_cus, lds, stream) : launch_ng<OP, MODE, 2, 2>(A, n_cus, lds, stream);
    if constexpr (OP == OP_FIND) {
        if (A.a.bprog) // find() of a pattern without bounded match lengths: starts by backward walks
            return A.ng.stride == 4 ? launch_ng<OP, MODE, 4, 1, false, true>(A, n_cus, lds, stream) : launch_ng<OP, MODE, 2, 1, false, true>(A, n_cus, lds, stream);
    }
    return A.ng.stride == 4 ? launch_ng<OP, MODE, 4, 1>(A, n_cus, lds, stream) : launch_ng<OP, MODE, 2, 1>(A, n_cus, lds, stream);
}

template <int OP>
static hipError_t launch_ng_m(const NgramArgs &A, int n_cus, size_t lds, hipStream_t stream) {
    if (A.ng.wide) { // UTF-16 rows, windows of four code units, walks on the UTF-16 HBM-table program (lower_filter_wide)
        if (A.char_width != 2 || A.a.hdr.mode != MODE_GLOBAL) return hipErrorInvalidValue;
        return A.ng.stride == 4 ? launch_ng<OP, MODE_GLOBAL, 4, 2, true>(A, n_cus, lds, stream) : launch_ng<OP, MODE_GLOBAL, 2, 2, true>(A, n_cus, lds, stream);
    }
    switch (A.a.hdr.mode) {
    case MODE_TABLE8: return launch_ng_s<OP, MODE_TABLE8>(A, n_cus, lds, stream);
    case MODE_TABLE16: return launch_ng_s<OP, MODE_TABLE16>(A, n_cus, lds, stream);
    case MODE_SPARSE: return launch_ng_s<OP, MODE_SPARSE>(A, n_cus, lds, stream);
    case MODE_GLOBAL: return launch_ng_s<OP, MODE_GLOBAL>(A, n_cus, lds, stream);
    default: return hipErrorInvalidValue;
    }
}

// LDS a launch takes; 0 = does not fit (the caller keeps the ordinary kernel)
size_t ngram_lds_bytes(const ProgHeader &h, const NgramParams &ng) {
    NgramLayout l;
    if (ng.on2 && ngram_layout(h.lds_bytes, ng.bm_bytes, &l, kNgWaveLds, ng.bm2_bytes)) return l.total;
    return ngram_layout(h.lds_bytes, ng.bm_bytes, &l) ? l.total : 0;
}

// Whether this batch shape can take the filter kernel at all: 8-bit rows 64 .. 4096 bytes apart in steps of 16 (a 64-row group is then
// stride / 16 KiB units), where rounding a group up to whole batches of kNgPF units wastes at most a quarter of the reads.
bool ngram_shape_ok(const ScanArgs &a) {
    const uint64_t units = a.stride_bytes / 16, rounded = (units + (kNgPF - 1)) & ~(uint64_t)(kNgPF - 1);
    return a.stride_bytes % 16 == 0 && a.stride_bytes >= 64 && a.stride_bytes <= 4096 && rounded * 4 <= units * 5 && a.total_bytes >= 16384 &&
           a.from == nullptr && a.end_state == nullptr && a.row_len <= 65535u;
}

static hipError_t launch_ngram_any(int op, const ScanArgs &a, const NgramParams &ng, const uint32_t *d_bitmap, uint32_t *d_stats, int n_cus, hipStream_t stream,
                                   const NgramArgs *fa, int char_width = 1, int page = 0, int sub = 0xFF);

// char_width 2: UTF-16 rows behind the BYTE program's filter (patterns below 0xFF only: the caller checks) -- a.stride_bytes and
// a.total_bytes count chars then
hipError_t launch_ngram(int op, const ScanArgs &a, const NgramParams &ng, const uint32_t *d_bitmap, uint32_t *d_stats, int n_cus, hipStream_t stream,
                        int char_width, int page, int sub) {
    return launch_ngram_any(op, a, ng, d_bitmap, d_stats, n_cus, stream, nullptr, char_width, page, sub);
}

// LDS of the find-all form; 0 = does not fit
size_t ngram_find_all_lds_bytes(const ProgHeader &h, const NgramParams &ng) {
    NgramLayout l;
    if (ng.on2 && ngram_layout(h.lds_bytes, ng.bm_bytes, &l, kNgWaveLdsFA + kNgQueue * 4u, ng.bm2_bytes)) return l.total;
    return ngram_layout(h.lds_bytes, ng.bm_bytes, &l, kNgWaveLdsFA) ? l.total : 0;
}

// Every non-overlapping match of every row behind the filter (dense per-row slots, compact filing or counting only; needle_find_all.h FindAllArgs): `a` carries the
// rows and the lengths program, the outputs are the find-all ones.
hipError_t launch_ngram_find_all(const ScanArgs &a, const NgramParams &ng, const uint32_t *d_bitmap, uint32_t *d_stats, uint32_t slots, uint32_t *counts,
                                 int32_t *starts, int32_t *ends, uint32_t *packed, int32_t *more, const uint64_t *offsets, bool count_only, int n_cus,
                                 hipStream_t stream, int char_width, int page, int sub, uint32_t kshift) {
    NgramArgs F;
    memset(&F, 0, sizeof(F));
    F.fa_kshift = offsets ? 0u : kshift;
    F.fa_slots = slots, F.fa_counts = counts, F.fa_starts = starts, F.fa_ends = ends, F.fa_packed = packed, F.fa_more = more;
    F.fa_offsets = offsets, F.fa_count_only = count_only ? 1u : 0u;
    return launch_ngram_any(OP_NG_FIND_ALL, a, ng, d_bitmap, d_stats, n_cus, stream, &F, char_width, page, sub);
}

static hipError_t launch_ngram_any(int op, const ScanArgs &a, const NgramParams &ng, const uint32_t *d_bitmap, uint32_t *d_stats, int n_cus, hipStream_t stream,
                                   const NgramArgs *fa, int char_width, int page, int sub) {
    NgramArgs A;
    memset(&A, 0, sizeof(A));
    if (fa) A = *fa;
    A.char_width = (uint32_t)char_width;
    A.page4 = (uint32_t)(page & 255) * 0x01010101u, A.sub4 = (uint32_t)(sub & 255) * 0x01010101u;
    A.a = a;
    A.ng = ng;
    A.ng_bitmap = d_bitmap;
    A.stats = d_stats;
    const uint32_t stride = (uint32_t)a.stride_bytes;
    A.stride_log2 = 0xFFFFFFFFu;
    if ((stride & (stride - 1u)) == 0u) A.stride_log2 = (uint32_t)__builtin_ctz(stride);
    A.stride_recip = (uint32_t)((1ull << 32) / stride);
    // the second level needs its bitmap and a second queue per wave in LDS: find / containedIn were sized for it by the host; the find-all
    // form (two slots + a counter per row beside the queues) takes it where it still fits (walks out of HBM: yes; a 96 KB automaton: no)
    const uint32_t wb1 = op == OP_NG_FIND_ALL ? kNgWaveLdsFA : kNgWaveLds;
    const uint32_t wb2 = op == OP_NG_FIND_ALL ? kNgWaveLdsFA + kNgQueue * 4u : kNgWaveLds;
    if (ng.on2 && !ngram_layout(a.hdr.lds_bytes, ng.bm_bytes, &A.lay, wb2, ng.bm2_bytes)) A.ng.on2 = 0;
    if (!A.ng.on2 && !ngram_layout(a.hdr.lds_bytes, ng.bm_bytes, &A.lay, wb1)) return hipErrorInvalidValue;
    if (ng.addr_shift != 24u) return hipErrorInvalidValue;
    A.dbg = 0;
#ifdef NEEDLE_TUNING
    static const uint32_t dbg_env = getenv("NEEDLE_NG_DBG") ? (uint32_t)atoi(getenv("NEEDLE_NG_DBG")) : 0u;
    A.dbg = dbg_env;
#endif
    const size_t lds = A.lay.total;
#ifdef NEEDLE_TUNING
    // NEEDLE_NG_STAMPS=1: every launch is followed by a device synchronisation and one line on stderr -- the waves' shader cycles by
    // section (the kernel's NG_STAMP points), summed over all waves, as shares of their total lifetime
    static const bool stamps_env = getenv("NEEDLE_NG_STAMPS") && atoi(getenv("NEEDLE_NG_STAMPS")) != 0;
    if (stamps_env) {
        static uint64_t *d_stamps = nullptr;
        const size_t n_waves = (size_t)n_cus * kWavesPerBlock, bytes = n_waves * 8 * sizeof(uint64_t);
        if (!d_stamps && hipMalloc((void **)&d_stamps, 4096 * 8 * sizeof(uint64_t)) != hipSuccess) return hipErrorOutOfMemory;
        if (n_waves > 4096) return hipErrorInvalidValue;
        (void)hipMemsetAsync(d_stamps, 0, bytes, stream);
        A.stamps = d_stamps;
        hipError_t e = op == OP_NG_FIND_ALL ? launch_ng_m<OP_NG_FIND_ALL>(A, n_cus, lds, stream)
                       : op == OP_FIND      ? launch_ng_m<OP_FIND>(A, n_cus, lds, stream)
                                            : launch_ng_m<OP_CONTAINED_IN>(A, n_cus, lds, stream);
        if (e != hipSuccess) return e;
        std::vector<uint64_t> h(n_waves * 8);
        e = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = hipMemcpy(h.data(), d_stamps, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return e;
        double sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mx = 0;
        for (size_t w = 0; w < n_waves; ++w) {
            for (int k = 0; k < 8; ++k) sum[k] += (double)h[w * 8 + k];
            if ((double)h[w * 8 + 7] > mx) mx = (double)h[w * 8 + 7];
        }
        fprintf(stderr, "NG-STAMPS op %d mode %u S %u cw %d wide %u: waves %zu, mean lifetime %.0f cycles (max %.0f); shares: text-wait %.3f probe %.3f queue %.3f level2 %.3f walk %.3f group %.3f staging %.3f\n",
                op, a.hdr.mode, ng.stride, char_width, ng.wide, n_waves, sum[7] / n_waves, mx, sum[0] / sum[7], sum[1] / sum[7], sum[2] / sum[7],
                sum[3] / sum[7], sum[4] / sum[7], sum[5] / sum[7], sum[6] / sum[7]);
        { // how unevenly the waves finish: percentiles of their lifetimes, and the mean by XCD (block % 8) and by wave slot
            std::vector<double> life(n_waves);
            double xcd[8] = {0, 0, 0, 0, 0, 0, 0, 0}, slot[kWavesPerBlock];
            for (int k = 0; k < kWavesPerBlock; ++k) slot[k] = 0;
            for (size_t w = 0; w < n_waves; ++w) life[w] = (double)h[w * 8 + 7], xcd[(w / kWavesPerBlock) % 8] += life[w], slot[w % kWavesPerBlock] += life[w];
            std::vector<double> srt = life;
            std::sort(srt.begin(), srt.end());
            fprintf(stderr, "NG-LIFE p01 %.0f p10 %.0f p50 %.0f p90 %.0f p99 %.0f max %.0f; by xcd:", srt[n_waves / 100], srt[n_waves / 10], srt[n_waves / 2], srt[n_waves * 9 / 10],
                    srt[n_waves * 99 / 100], srt[n_waves - 1]);
            for (int k = 0; k < 8; ++k) fprintf(stderr, " %.0f", xcd[k] / (n_waves / 8));
            fprintf(stderr, "; by wave slot:");
            for (int k = 0; k < kWavesPerBlock; ++k) fprintf(stderr, " %.0f", slot[k] / n_cus);
            fprintf(stderr, "\n");
            for (int q = 0; q < 4; ++q) { // the four waves of a SIMD, oldest first: mean cycles by section
                double sec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (size_t w = 0; w < n_waves; ++w)
                    if ((int)((w % kWavesPerBlock) / 4) == q)
                        for (int k = 0; k < 8; ++k) sec[k] += (double)h[w * 8 + k];
                fprintf(stderr, "NG-SLOT %d: text-wait %.0f probe %.0f queue %.0f level2 %.0f walk %.0f group %.0f total %.0f\n", q, sec[0] / (n_waves / 4), sec[1] / (n_waves / 4),
                        sec[2] / (n_waves / 4), sec[3] / (n_waves / 4), sec[4] / (n_waves / 4), sec[5] / (n_waves / 4), sec[7] / (n_waves / 4));
            }
        }
        return hipSuccess;
    }
#endif
    if (op == OP_NG_FIND_ALL) return launch_ng_m<OP_NG_FIND_ALL>(A, n_cus, lds, stream);
    return op == OP_FIND ? launch_ng_m<OP_FIND>(A, n_cus, lds, stream) : launch_ng_m<OP_CONTAINED_IN>(A, n_cus, lds, stream);
}

} // namespace needle
