// C ABI of libneedle_hip.so (include/needle_hip.h): pattern objects and pattern sets, the per-device program cache, the choice of the
// scan route, and the batch entry points for rows in DEVICE memory.  The entries for rows in host memory and the Matcher mirror are
// needle_host.cpp's, built on the _dev entries here.  No CPU matching path exists in this library.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <functional>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/needle_hip.h"
#include "needle_captures.h"
#include "needle_device.h"
#include "needle_find_all.h"
#include "needle_internal.h"
#include "needle_launch.h"
#include "needle_lower.h"
#include "needle_regex.h"
#include "needle_set.h"
#include "needle_template.h"

using namespace needle;

static thread_local std::string g_err;

static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#ifdef NEEDLE_TUNING // measurement builds only (scripts/build_tuning.sh): a switch that changes ANSWERS (start = end) never ships
static bool debug_no_backward() {
    static const bool on = getenv("NEEDLE_DEBUG_NO_BACKWARD") != nullptr;
    return on;
}
#endif

namespace needle {
int set_error(int code, const std::string &msg) { return fail(code, msg); } // (the other translation units report through the same channel)
} // namespace needle

// Stream-ordered scratch memory comes from a pool of the library's own, one per device, that KEEPS what it is given back:
// HIP's default pool returns freed memory to the driver at the next synchronisation point (release threshold 0), so a
// caller that synchronises after every call would pay a fresh driver allocation of tens of megabytes per call
// (needle_find_compact_dev: 2.5 ms per step on a 10M-row batch before this).  What the pool keeps is bounded:
// NEEDLE_SCRATCH_KEEP_MB (default 512) is its release threshold -- freed memory above it goes back to the driver at the next
// synchronisation point, so one large batch does not pin its peak scratch for the life of the process -- and
// needle_trim_scratch() hands back everything that is free.
namespace needle {
static std::mutex g_scratch_mu;
static std::map<int, hipMemPool_t> g_scratch_pools;
hipError_t scratch_trim(size_t keep_bytes) {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    hipError_t first = hipSuccess;
    for (auto &kv : g_scratch_pools)
        if (kv.second) {
            const hipError_t e = hipMemPoolTrimTo(kv.second, keep_bytes);
            if (e != hipSuccess && first == hipSuccess) first = e;
        }
    return first;
}
hipError_t scratch_malloc(void **out, size_t bytes, hipStream_t stream) {
    std::mutex &mu = g_scratch_mu;
    std::map<int, hipMemPool_t> &pools = g_scratch_pools;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipMemPool_t pool = nullptr;
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = pools.find(dev);
        if (it == pools.end()) {
            hipMemPoolProps props;
            memset(&props, 0, sizeof(props));
            props.allocType = hipMemAllocationTypePinned;
            props.handleTypes = hipMemHandleTypeNone;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = dev;
            if (hipMemPoolCreate(&pool, &props) == hipSuccess) {
                static const uint64_t keep_mb = getenv("NEEDLE_SCRATCH_KEEP_MB") ? (uint64_t)atoll(getenv("NEEDLE_SCRATCH_KEEP_MB")) : 512;
                uint64_t keep = keep_mb << 20;
                (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
            } else {
                (void)hipGetLastError();
                pool = nullptr; // (no pool of our own: the device's default one)
            }
            it = pools.emplace(dev, pool).first;
        }
        pool = it->second;
    }
    return pool ? hipMallocFromPoolAsync(out, bytes, pool, stream) : hipMallocAsync(out, bytes, stream);
}
hipError_t scratch_free(void *p, hipStream_t stream) { return hipFreeAsync(p, stream); }
} // namespace needle

struct DevProgram {
    Program prog;
    uint8_t *d_blob = nullptr;
    uint32_t *d_ng = nullptr; // the n-gram filter's bitmap (prog.ng.p.on)
    // Flood watch of the n-gram filter kernel.  Text that passes the filter almost everywhere (built from the dictionary's own
    // keyword tails: one automaton run per window) makes that kernel several times SLOWER than the ordinary scan (measured:
    // 5.3 against 1.13 ms on the C3-sparse dictionary, scripts/ngram_worstcase.py).  Every filter launch adds its candidates
    // and KiB of text to d_ng_stats; the pair is copied to the pinned h_ng_stats behind the kernel (on ng_stream, below).  The NEXT call
    // reads it without waiting: above 16 candidates per KiB (the break-even; the bench text has 3.3) the filter is suspended for
    // the program's next 32 calls, doubling up to 1024 while the text stays like that.  Answers are the same either way.
    uint32_t *d_ng_stats = nullptr;            // {candidates, KiB of text}: MONOTONIC device counters (never reset by the host)
    volatile uint64_t *h_ng_stats = nullptr;    // pinned: the pair as it stood behind the last completed filter launch (one 8-byte copy)
    // The copy runs on a stream of its own behind an event of the launch: on the caller's stream it could queue behind another stream's
    // bulk D2H on the copy engine and hold the NEXT scan back until that finished (measured: pipelined host landing of a 1.1 ms scan
    // at 1.86 ms per step = scan + copy, serialised).
    hipStream_t ng_stream = nullptr;
    hipEvent_t ng_ev = nullptr;
    // the watch's own state, per program (= per pattern x device x op), shared by every stream and thread that uses it
    mutable std::mutex ng_mu;
    mutable uint32_t ng_seen_cand = 0, ng_seen_kib = 0; // what the last evaluation had seen: the watch works on deltas
    mutable int ng_suspend = 0, ng_backoff = 32;
    mutable float ng_last_rate = 0.0f;
    mutable uint64_t ng_launches = 0, ng_suspended_calls = 0;
    DevProgram() = default;
    DevProgram(DevProgram &&o) noexcept
        : prog(std::move(o.prog)), d_blob(o.d_blob), d_ng(o.d_ng), d_ng_stats(o.d_ng_stats), h_ng_stats(o.h_ng_stats), ng_stream(o.ng_stream), ng_ev(o.ng_ev) { // (moved before first use: the watch's state starts fresh)
        o.d_blob = nullptr, o.d_ng = nullptr, o.d_ng_stats = nullptr, o.h_ng_stats = nullptr, o.ng_stream = nullptr, o.ng_ev = nullptr;
    }
};

// The forms a pattern's automaton is lowered to: the last part of a program's cache key (the numbers ARE the keys: they do not change).
enum Variant : int {
    V_PLAIN = 0,            // the ordinary program
    V_WALK = 1,             // global-walk layout (backward automaton of find)
    V_BACKMAPS = 2,         // forward + backward column maps
    V_HBM_TABLE = 3,        // HBM-table layout forced (column maps + uint16 table in one blob: the speculative-stripe fix-up walks it)
    V_FA_PLAIN = 4,         // 4 / 5 as 0 / 2 without the pair table (the one-pass find-all kernel)
    V_FA_BACKMAPS = 5,
    V_FA_LENGTHS = 6,       // the find-all "lengths" automaton (W_FORWARDS only; absent when the pattern does not allow it)
    V_LENGTHS = 7,          // the same for find() in the scan kernels
    V_FA_TRANSDUCER = 8,    // the find-all transducer (lock-step find-all, needle_find_all_ls.hip; absent when the pattern does not allow it)
    V_FILTER_HBM = 9,       // the filter program of an automaton that fits the LDS in no form (lower_filter_hbm: HBM-table layout + n-gram filter;
                            // W_CONTAINED_IN, or W_FORWARDS in the lengths form / for one-length patterns; absent when no filter can be built)
    V_FILTER_WIDE = 10,     // the WIDE filter program (lower_filter_wide: char_width 2 only -- UTF-16 rows of a pattern on several pages of the BMP:
                            // windows of four code units, UTF-16 HBM-table program); absent when no filter can be built
    V_FA_RUNS = 11,         // the RUN transducer (lock-step find-all of patterns without bounded match lengths whose matches are runs: `[0-9]+`;
                            // needle_lower.h lower_find_all_runs); absent when the pattern is not of that kind
    V_FILTER_UNBOUNDED = 12 // V_FILTER_HBM for find() of a pattern WITHOUT bounded match lengths: the forward search automaton itself (no lengths
                            // form) with the backward automaton's column maps in its LDS part -- verified candidates find their starts by backward walks
};

struct needle_pattern {
    RefTables t;
    std::mutex mu;
    // (device, which, char_width, Variant) -> program resident in that device's HBM
    std::map<std::tuple<int, int, int, int>, DevProgram> cache;
    std::map<int, int> cus; // device -> CU count
    // needle_pattern_prefilter_info answers (lowering a big dictionary takes seconds): per `which`, filled once
    struct PrefilterCache {
        bool have = false;
        needle_prefilter_info info;
        uint32_t m1b = 0, m2b = 0;
        std::vector<uint32_t> bitmap;
    } pf_cache[8]; // [which]: the byte programs' filter; [4 + which]: the WIDE filter's (needle_pattern_prefilter_info2)
    std::mutex pf_mu;
    std::atomic<int> pf_mode{0}; // needle_pattern_set_prefilter: 0 auto (the flood watch decides), 1 on (never suspended), 2 off (never used)
    // UTF-16 rows behind a BYTE program (utf16_route): the pattern's one page and the byte that stands for every char outside it;
    // the tables rebased to that page (page_tables: what the byte programs of a page other than 0 are lowered from)
    std::mutex u16_mu;
    int u16_state = 0, u16_page = -1, u16_sub = 0; // state 0: not looked at yet
    struct PageTables {
        RefTables t;
        bool have_ml = false;
        MatchLengths ml;
    };
    std::map<int, PageTables> page_tables; // (under `mu`)
    std::mutex ml_mu;       // guards the one-time match-length analysis only: scans of programs that exist already do not wait for it
    int ml_state = 0;       // 0: not analysed yet, 1: find-all can report starts as end - length (ml), -1: it cannot
    MatchLengths ml;
    // The capture program (needle_captures.h) is built from the regex TEXT, which only needle_compile has: kept here, not in the blob.
    bool has_regex = false;
    std::u16string regex;
    int regex_flags = 0;
    std::mutex cap_mu;      // guards everything below
    bool cap_built = false;
    int cap_rc = NEEDLE_OK; // (the second parse's own status: NEEDLE_OK wherever compile_regex accepted the regex)
    std::string cap_err;
    CapTables cap;
    bool cap_lowered[2] = {false, false};
    CapProgram cap_prog[2];                             // [char_width - 1]
    std::map<std::pair<int, int>, uint8_t *> cap_resident; // (device, char_width) -> the program in that device's HBM
    std::map<int, int> cap_cus;                         // device -> CU count
    ~needle_pattern() {
        for (auto &kv : cap_resident)
            if (kv.second) (void)hipFree(kv.second);
        for (auto &kv : cache) {
            if (kv.second.ng_stream) (void)hipStreamSynchronize(kv.second.ng_stream); // (a stats copy may still be on its way into h_ng_stats)
            if (kv.second.d_blob) (void)hipFree(kv.second.d_blob);
            if (kv.second.d_ng) (void)hipFree(kv.second.d_ng);
            if (kv.second.d_ng_stats) (void)hipFree(kv.second.d_ng_stats);
            if (kv.second.h_ng_stats) (void)hipHostFree((void *)kv.second.h_ng_stats);
            if (kv.second.ng_stream) (void)hipStreamDestroy(kv.second.ng_stream);
            if (kv.second.ng_ev) (void)hipEventDestroy(kv.second.ng_ev);
        }
    }
};

needle::MatcherRoots needle::matcher_roots(const needle_pattern *p) {
    auto root = [&](int w) { return !p->t.dfa[w].accepting.empty() && p->t.dfa[w].accepting[0] != 0; };
    return {root(W_FORWARDS), root(W_BACKWARDS), p->t.fixed_len};
}
bool needle::find_all_rounds_forced() {
    static const bool forced = (getenv("NEEDLE_FIND_ALL_ROUNDS") ? atoi(getenv("NEEDLE_FIND_ALL_ROUNDS")) : 0) != 0;
    return forced;
}

// Automaton LDS budget.  NEEDLE_MAX_PROG_LDS (bytes) lowers it: tests use that to force the HBM-table mode.
static size_t max_prog_lds() {
    static const size_t v = getenv("NEEDLE_MAX_PROG_LDS") ? (size_t)atol(getenv("NEEDLE_MAX_PROG_LDS")) : (size_t)kMaxProgLdsBytes;
    return v < kMaxProgLdsBytes ? v : (size_t)kMaxProgLdsBytes;
}

// The pattern's match-length analysis (needle_lower.h), run once per pattern -- it can take seconds of host time on a big
// dictionary -- and shared by every caller: the scans, needle_pattern_program_info / _prefilter_info / _match_lengths.
// nullptr: the pattern does not allow the "lengths" form.
static const MatchLengths *pattern_ml(const needle_pattern *cp) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    std::lock_guard<std::mutex> lk(p->ml_mu);
    if (p->ml_state == 0) {
        p->ml = match_length_automaton(p->t);
        p->ml_state = p->ml.ok ? 1 : -1;
    }
    return p->ml_state > 0 ? &p->ml : nullptr;
}

// Whether lowering `variant` asks for the pattern's match-length analysis (pattern_ml: taken BEFORE p->mu, see ml_mu)
static bool variant_wants_ml(const needle_pattern *p, int which, Variant variant) {
    return variant == V_FA_LENGTHS || variant == V_LENGTHS || variant == V_FA_TRANSDUCER ||
           ((variant == V_FILTER_HBM || variant == V_FILTER_WIDE) && which == W_FORWARDS && p->t.fixed_len < 0);
}
// The tables a program of char width cw | page << 8 is lowered from (under p->mu): the pattern's own, or -- page != 0 -- rebased to that
// page of the BMP; *ml (when given) is moved along.
static const RefTables *tables_for_page(needle_pattern *p, int page, const MatchLengths **ml) {
    const MatchLengths *ml67 = *ml;
    const RefTables *tt = &p->t;
    if (page) { // chars page << 8 | b become bytes b: the class map's page in front, every automaton's maxChar moved along
        auto pit = p->page_tables.find(page);
        if (pit == p->page_tables.end()) {
            needle_pattern::PageTables pt;
            pt.t = p->t;
            for (int b = 0; b < 256; ++b) pt.t.class_map[b] = p->t.class_map[(size_t)(page << 8) | b];
            auto rebase = [&](int32_t mc) { const int32_t r = mc - (page << 8); return r > 255 ? 255 : (r < -1 ? -1 : r); };
            for (int w = 0; w < 4; ++w) pt.t.dfa[w].max_char = rebase(p->t.dfa[w].max_char);
            pit = p->page_tables.emplace(page, std::move(pt)).first;
        }
        if (ml67 && !pit->second.have_ml) {
            pit->second.ml = *ml67;
            const int32_t r = ml67->dfa.max_char - (page << 8);
            pit->second.ml.dfa.max_char = r > 255 ? 255 : (r < -1 ? -1 : r);
            pit->second.have_ml = true;
        }
        tt = &pit->second.t;
        if (ml67) ml67 = &pit->second.ml;
    }
    *ml = ml67;
    return tt;
}
// One variant's program, lowered on the host: what get_program makes resident, and what the host-side route queries look at.  false: the
// pattern has no such program (no bounded match lengths, no filter, not a pattern of runs, no plain LDS table for the lengths form).
static bool lower_variant(const RefTables &tt, int which, int cw, Variant variant, bool wants_ml, const MatchLengths *ml67, Program *out) {
    if (variant == V_FILTER_HBM || variant == V_FILTER_WIDE || variant == V_FILTER_UNBOUNDED) {
        if ((wants_ml && !ml67) || (variant == V_FILTER_WIDE && cw != 2) || (variant == V_FILTER_UNBOUNDED && (which != W_FORWARDS || cw != 1))) return false;
        *out = variant == V_FILTER_WIDE ? lower_filter_wide(tt, (Which)which, ml67)
                                        : lower_filter_hbm(tt, (Which)which, variant == V_FILTER_UNBOUNDED ? nullptr : ml67, variant == V_FILTER_UNBOUNDED);
        return !out->blob.empty() && out->ng.p.on; // (no filter: the ordinary program is what runs)
    }
    if (variant == V_FA_RUNS) { // (absent when the pattern is not one of runs)
        *out = lower_find_all_runs(tt, cw, max_prog_lds());
        return !out->blob.empty();
    }
    if (variant == V_FA_LENGTHS || variant == V_LENGTHS || variant == V_FA_TRANSDUCER) {
        // "lengths" form: the refined forward automaton + pend[] (needle_lower.h); V_FA_LENGTHS: the find-all kernel's plain layout,
        // V_LENGTHS: the scan kernels' (window addressing); V_FA_TRANSDUCER: the find-all transducer built on it
        if (!ml67) return false;
        *out = variant == V_FA_TRANSDUCER ? lower_find_all_transducer(tt, *ml67, cw, max_prog_lds())
                                          : lower_match_lengths(tt, *ml67, cw, max_prog_lds(), variant == V_FA_LENGTHS);
        return !out->blob.empty(); // (empty: does not fit the LDS as a plain table -- the ordinary program with backward walks)
    }
    *out = lower(tt, (Which)which, cw, variant == V_HBM_TABLE ? 0 : max_prog_lds(), variant == V_WALK, variant == V_BACKMAPS || variant == V_FA_BACKMAPS,
                 variant == V_FA_PLAIN || variant == V_FA_BACKMAPS);
    return true;
}

static int get_program(needle_pattern *p, int which, int cw, Variant variant, const DevProgram **out, int *n_cus) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    // cw = 1 | page << 8: the BYTE program of the pattern rebased to one page of the BMP (UTF-16 rows narrowed on the fly: utf16_route)
    const int page = cw >> 8, cw_key = cw;
    cw &= 0xFF;
    const bool wants_ml = variant_wants_ml(p, which, variant);
    const MatchLengths *ml67 = wants_ml ? pattern_ml(p) : nullptr; // (before p->mu: see ml_mu)
    std::lock_guard<std::mutex> lk(p->mu);
    const RefTables *tt = tables_for_page(p, page, &ml67);
    if (!p->cus.count(dev)) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        p->cus[dev] = prop.multiProcessorCount;
    }
    if (n_cus) *n_cus = p->cus[dev];
    auto key = std::make_tuple(dev, which, cw_key, (int)variant);
    auto it = p->cache.find(key);
    if (it == p->cache.end()) {
        DevProgram dp;
        if (!lower_variant(*tt, which, cw, variant, wants_ml, ml67, &dp.prog)) { // (an empty entry = "not available for this pattern / width")
            p->cache.emplace(key, DevProgram());
            *out = nullptr;
            return NEEDLE_OK;
        }
        HIP_TRY(hipMalloc((void **)&dp.d_blob, dp.prog.blob.size()));
        if (hipError_t ce = hipMemcpy(dp.d_blob, dp.prog.blob.data(), dp.prog.blob.size(), hipMemcpyHostToDevice); ce != hipSuccess) {
            (void)hipFree(dp.d_blob);
            return hip_fail(ce, "hipMemcpy(program blob)");
        }
        if (dp.prog.ng.p.on) {
            const size_t nb = dp.prog.ng.bitmap.size() * 4, nb2 = dp.prog.ng.p.on2 ? dp.prog.ng.bitmap2.size() * 4 : 0; // (the second level's follows)
            hipError_t ce = hipMalloc((void **)&dp.d_ng, nb + nb2 + 16);
            if (ce == hipSuccess) ce = hipMemcpy(dp.d_ng, dp.prog.ng.bitmap.data(), nb, hipMemcpyHostToDevice);
            if (ce == hipSuccess && nb2) ce = hipMemcpy((uint8_t *)dp.d_ng + nb, dp.prog.ng.bitmap2.data(), nb2, hipMemcpyHostToDevice);
            if (ce == hipSuccess) ce = hipMalloc((void **)&dp.d_ng_stats, 8);
            if (ce == hipSuccess) ce = hipMemset(dp.d_ng_stats, 0, 8);
            if (ce == hipSuccess) ce = hipHostMalloc((void **)&dp.h_ng_stats, 8, hipHostMallocDefault);
            if (ce == hipSuccess) ce = hipStreamCreateWithFlags(&dp.ng_stream, hipStreamNonBlocking);
            if (ce == hipSuccess) ce = hipEventCreateWithFlags(&dp.ng_ev, hipEventDisableTiming);
            if (ce != hipSuccess) {
                (void)hipFree(dp.d_blob);
                if (dp.d_ng) (void)hipFree(dp.d_ng);
                if (dp.d_ng_stats) (void)hipFree(dp.d_ng_stats);
                if (dp.h_ng_stats) (void)hipHostFree((void *)dp.h_ng_stats);
                if (dp.ng_stream) (void)hipStreamDestroy(dp.ng_stream);
                if (dp.ng_ev) (void)hipEventDestroy(dp.ng_ev);
                return hip_fail(ce, "hipMalloc/hipMemcpy(n-gram bitmap)");
            }
            dp.h_ng_stats[0] = 0;
        }
        it = p->cache.emplace(key, std::move(dp)).first;
    }
    *out = it->second.d_blob ? &it->second : nullptr; // (an empty entry = "not available for this pattern / width")
    return NEEDLE_OK;
}

static int check_view(const needle_batch_view *v) {
    if (!v) return fail(NEEDLE_ERR_INVALID, "batch view is NULL");
    if (v->char_width != 1 && v->char_width != 2) return fail(NEEDLE_ERR_INVALID, "char_width must be 1 or 2");
    if (v->n_rows && !v->rows) return fail(NEEDLE_ERR_INVALID, "rows is NULL");
    if (v->row_len > v->row_stride) return fail(NEEDLE_ERR_INVALID, "row_len > row_stride");
    if ((v->row_stride * v->char_width) % 16 != 0)
        return fail(NEEDLE_ERR_INVALID, "row_stride * char_width must be a multiple of 16 bytes for device batches");
    if (((uintptr_t)v->rows) % 16 != 0) return fail(NEEDLE_ERR_INVALID, "rows must be 16-byte aligned");
    if (v->n_rows && v->row_stride == 0) return fail(NEEDLE_ERR_INVALID, "row_stride is 0");
    return NEEDLE_OK;
}

// 16-bit result offsets: what the API can tell about the longest row -- row_len, or with per-row lengths (device memory, not
// readable here) the stride, which may be the caller's limit rounded up to the 16-byte alignment of device rows (65 536); the
// lengths themselves must stay within `limit` (the host entry points check them).
static bool offsets16_ok(const needle_batch_view *v, uint32_t limit) {
    return v->lengths ? v->row_stride <= 65536u : v->row_len <= limit;
}

// Where a scan's results go.  packed (find() only): a row's start / end as one dword -- or one uint16, with packed8 -- stored by the kernel
// itself; start / end are not used then.
struct ScanOut {
    uint64_t *bitmap = nullptr;
    int32_t *start = nullptr, *end = nullptr;
    uint32_t *packed = nullptr;
    bool packed8 = false;
};

// THE ScanArgs of forward program fp on n_rows rows at `rows`: bp = the backward program, where find() walks back for its starts
// (nullptr: none), fixed_len = -1 or the pattern's one match length.  Every field not named here stays zero; a call that has more
// to say (cursors, end states) adds it to what it gets back.  This is all a packed batch needs: its offsets travel beside the ScanArgs.
static ScanArgs scan_args(const void *rows, uint64_t n_rows, const DevProgram *fp, const DevProgram *bp, int32_t fixed_len, const ScanOut &out) {
    ScanArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = (const uint8_t *)rows;
    a.n_rows = n_rows;
    a.prog = fp->d_blob;
    a.hdr = fp->prog.hdr;
    if (bp) a.bprog = bp->d_blob, a.bhdr = bp->prog.hdr;
    a.fixed_len = fixed_len;
    a.bitmap = out.bitmap;
    a.start = out.start;
    a.end = out.end;
    a.packed = out.packed;
    a.packed8 = out.packed8 ? 1u : 0u;
    return a;
}
static ScanArgs scan_args(const needle_packed_view *v, const DevProgram *fp, const DevProgram *bp, int32_t fixed_len, const ScanOut &out) {
    return scan_args(v->data, v->n_rows, fp, bp, fixed_len, out);
}
// Fixed-stride rows.  stride: bytes between rows -- or CHARS, for UTF-16 rows behind a byte program's filter (launch_ngram and
// launch_ngram_find_all with char_width 2 scale the addresses).
static ScanArgs scan_args(const needle_batch_view *v, uint64_t stride, const DevProgram *fp, const DevProgram *bp, int32_t fixed_len, const ScanOut &out) {
    ScanArgs a = scan_args(v->rows, v->n_rows, fp, bp, fixed_len, out);
    a.stride_bytes = stride;
    a.total_bytes = a.n_rows * a.stride_bytes;
    a.row_len = v->row_len;
    a.lengths = v->lengths;
    return a;
}

static int which_of(int op) { return op == OP_MATCHES ? W_MATCHES : op == OP_CONTAINED_IN ? W_CONTAINED_IN : W_FORWARDS; }

// The backward automaton find() walks for a match's start (global-walk layout) where the pattern has no one length and the forward
// program is not the lengths form.
static int backward_program(needle_pattern *p, int cw, const DevProgram **bp) { return get_program(p, W_BACKWARDS, cw, V_WALK, bp, nullptr); }

// find()'s starts after the fact, one lane per matched row: indexBackwards from the lastMatch in d_end (needle_stripe.hip backward_rows).
static hipError_t launch_find_starts(int cw, const void *rows, uint64_t n_rows, uint64_t stride_bytes, const DevProgram *fp, const DevProgram *bp, int32_t fixed_len,
                                     uint64_t *d_bitmap, int32_t *d_start, int32_t *d_end, hipStream_t stream) {
    StripeArgs ba;
    memset(&ba, 0, sizeof(ba));
    ba.rows = (const uint8_t *)rows;
    ba.n_rows = n_rows;
    ba.stride_bytes = stride_bytes;
    ba.prog = fp->d_blob;
    ba.hdr = fp->prog.hdr;
    ba.bitmap = d_bitmap;
    ba.start = d_start;
    ba.end = d_end;
    ba.fixed_len = fixed_len;
    ba.op = OP_FIND;
    if (bp) ba.bprog = bp->d_blob, ba.bhdr = bp->prog.hdr;
    return launch_backward_rows(cw, ba, stream);
}

// Few, long rows: one row per lane would leave the chip idle.  Packed-mode automata take the stripe path (function
// composition across 4 KiB stripes, needle_stripe.hip); NEEDLE_LONG_ROWS=0 turns it off, =1 forces it (tests).
static int long_rows_force() {
    static const int force = getenv("NEEDLE_LONG_ROWS") ? atoi(getenv("NEEDLE_LONG_ROWS")) : -1;
    return force;
}
static bool wants_stripe_path(const needle_batch_view *v, const ProgHeader &hdr, bool has_cursors) {
    const int force = long_rows_force();
    const uint64_t stride_bytes = v->row_stride * v->char_width;
    const bool wanted = force >= 0 ? force == 1 : (v->n_rows < 65536 && stride_bytes >= 8 * (uint64_t)kStripeBytes);
    return wanted && hdr.mode == MODE_PACK && !has_cursors;
}

static int run_stripe_path(needle_pattern *p, int op, const needle_batch_view *v, const DevProgram *fp, int n_cus,
                           uint64_t *d_bitmap, int32_t *d_start, int32_t *d_end, void *stream) {
    const uint64_t stride_bytes = v->row_stride * v->char_width;
    StripeArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.rows = (const uint8_t *)v->rows;
    sa.n_rows = v->n_rows;
    sa.stride_bytes = stride_bytes;
    sa.row_len = v->row_len;
    sa.lengths = v->lengths;
    sa.prog = fp->d_blob;
    sa.hdr = fp->prog.hdr;
    sa.spr = (uint32_t)((stride_bytes + kStripeBytes - 1) / kStripeBytes);
    sa.bitmap = d_bitmap;
    sa.start = d_start;
    sa.end = d_end;
    sa.fixed_len = op == OP_FIND ? p->t.fixed_len : -1;
    sa.op = (uint32_t)op;
    if (op == OP_FIND && sa.fixed_len < 0) {
        const DevProgram *bp = nullptr;
        int rc = backward_program(p, (int)v->char_width, &bp);
        if (rc) return rc;
        sa.bprog = bp->d_blob;
        sa.bhdr = bp->prog.hdr;
    }
    // find(): pass 1 also marks the stripes that pass through an accepting state, and only the last such stripe of a row is walked
    // again for lastMatch (needle_stripe.hip).  NEEDLE_STRIPE_CAND=0: every stripe is (A/B, tests).
    static const bool cand_on = (getenv("NEEDLE_STRIPE_CAND") ? atoi(getenv("NEEDLE_STRIPE_CAND")) : 1) != 0;
    const size_t fn_bytes = ((size_t)sa.n_rows * sa.spr * 4 + 15) & ~(size_t)15;
    const bool cand = op == OP_FIND && cand_on;
    HIP_TRY(scratch_malloc((void **)&sa.fn, fn_bytes * (cand ? 2 : 1) + (cand ? (size_t)sa.n_rows * 4 : 0), (hipStream_t)stream));
    if (cand) {
        sa.cand = (uint32_t *)((uint8_t *)sa.fn + fn_bytes);
        sa.cand_stripe = (int32_t *)((uint8_t *)sa.fn + 2 * fn_bytes);
    }
    hipError_t e = launch_long_rows((int)v->char_width, sa, n_cus, (hipStream_t)stream);
    (void)scratch_free(sa.fn, (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "launch_long_rows");
    return NEEDLE_OK;
}

// Flood watch of the filter kernel (DevProgram).  Text that passes the filter almost everywhere makes that kernel several times
// slower than the ordinary scan; every filter launch ADDS its candidates and KiB of text to two monotonic device counters, copied
// (one 8-byte copy) to pinned memory behind the kernel.  The next call of that program looks at what has arrived -- without waiting --
// and works on the DELTA against what the last evaluation saw: above 16 candidates per KiB the filter is suspended for the program's
// next 32 calls, doubling to 1024 while the text stays like that.  One mutex per program: the state is per pattern x device x op, NOT per
// stream -- concurrent streams share one verdict (and one backoff).  Answers are the same either way.
//   needle_pattern_set_prefilter(p, NEEDLE_PREFILTER_AUTO | _ON | _OFF) pins the decision (ON: never suspended; OFF: the ordinary kernels);
//   needle_pattern_prefilter_state() reports it.  Under HIP-graph capture the decision is the one taken at CAPTURE time and is replayed
//   as captured -- the stats copy is not captured (a captured graph neither feeds nor obeys the watch): pin the mode for captured work.
// false = this call takes the ordinary kernel.  NEEDLE_PREFILTER_WATCH=0: the watch never suspends.
static bool ngram_watch_allows(const needle_pattern *p, const DevProgram *fp) {
    const int mode = p->pf_mode.load();
    if (mode == 2) return false;
    static const bool watch_on = !(getenv("NEEDLE_PREFILTER_WATCH") && atoi(getenv("NEEDLE_PREFILTER_WATCH")) == 0);
    std::lock_guard<std::mutex> lk(fp->ng_mu);
    const uint64_t both = fp->h_ng_stats[0]; // (one aligned 8-byte read of what one 8-byte copy wrote)
    const uint32_t cand = (uint32_t)both, kib = (uint32_t)(both >> 32);
    const uint32_t d_cand = cand - fp->ng_seen_cand, d_kib = kib - fp->ng_seen_kib; // (unsigned: the counters may wrap)
    if (d_kib >= 1024u) {
        fp->ng_seen_cand = cand, fp->ng_seen_kib = kib;
        fp->ng_last_rate = (float)d_cand / (float)d_kib;
        if (mode == 1) {
            // (pinned ON: the rate is still reported; no suspension is scheduled for a later return to AUTO)
        } else if ((uint64_t)d_cand > 16ull * d_kib) {
            fp->ng_suspend = fp->ng_backoff;
            fp->ng_backoff = fp->ng_backoff < 1024 ? 2 * fp->ng_backoff : 1024;
        } else {
            fp->ng_backoff = 32;
        }
    }
    if (mode == 1 || !watch_on || fp->ng_suspend <= 0) {
        ++fp->ng_launches;
        return true;
    }
    --fp->ng_suspend;
    ++fp->ng_suspended_calls;
    return false;
}
// (behind the kernel, on the program's own copy stream; neither the host nor the caller's stream ever waits for it)
static hipError_t ngram_watch_after_launch(const DevProgram *fp, hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (stream && hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return hipSuccess; // (not captured: see above)
    std::lock_guard<std::mutex> lk(fp->ng_mu); // (one event per program: record / wait pairs of concurrent callers must not interleave)
    hipError_t e = hipEventRecord(fp->ng_ev, stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(fp->ng_stream, fp->ng_ev, 0);
    if (e == hipSuccess) e = hipMemcpyAsync((void *)fp->h_ng_stats, fp->d_ng_stats, 8, hipMemcpyDeviceToHost, fp->ng_stream);
    return e;
}

// UTF-16 rows behind a BYTE program's n-gram filter (needle_ngram.h narrow16).  The pattern must live on ONE page of the BMP: every char
// outside page P shares one class ("other": in no range of the pattern -- the class with the most chars), and some char P << 8 | sub of the
// page is of that class too.  Then a char outside the page behaves exactly as byte `sub` does in the program lowered from the tables
// REBASED to the page (get_program, cw = 1 | P << 8; page 0: the ordinary 8-bit program) -- the searching automata the filter runs have
// maxChar 0xFFFF, so "beyond maxChar" never comes into it.  ASCII / Latin-1 dictionaries: page 0, sub 0xFF; Cyrillic: page 4; ...
// NEEDLE_PREFILTER_UTF16=0: never.
struct Utf16Route {
    int page = -1, sub = 0;
};
static bool prefilter_utf16_off() {
    static const bool off = (getenv("NEEDLE_PREFILTER_UTF16") ? atoi(getenv("NEEDLE_PREFILTER_UTF16")) : 1) == 0;
    return off;
}
static Utf16Route utf16_route(const needle_pattern *cp) {
    const bool off = prefilter_utf16_off();
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    Utf16Route r;
    if (off) return r;
    std::lock_guard<std::mutex> lk(p->u16_mu);
    if (p->u16_state == 0) {
        p->u16_state = 1;
        const std::vector<uint8_t> &cm = p->t.class_map;
        if (cm.size() == 65536 && p->t.dfa[W_CONTAINED_IN].max_char == 0xFFFF && p->t.dfa[W_FORWARDS].max_char == 0xFFFF) {
            // classes with the same column in all four automata are one class here (the reference numbers every gap between two of the
            // pattern's ranges separately: "below 'a'" and "above 'z'" are two classes with identical columns)
            const int N = p->t.stride;
            std::vector<int> canon(256, 0);
            {
                std::vector<uint64_t> sig((size_t)N, 1469598103934665603ull);
                for (int w = 0; w < 4; ++w) {
                    const RefDfa &d = p->t.dfa[w];
                    for (int k = 0; k < N; ++k) {
                        uint64_t h = sig[(size_t)k];
                        for (int32_t st = 0; st < d.n_states; ++st) h = (h ^ (uint64_t)(uint16_t)d.table[(size_t)st * N + k]) * 1099511628211ull;
                        sig[(size_t)k] = h * 31u + (uint64_t)w;
                    }
                }
                for (int k = 0; k < N; ++k) {
                    canon[k] = k;
                    for (int j = 0; j < k; ++j) {
                        if (sig[(size_t)j] != sig[(size_t)k]) continue;
                        bool same = true; // (the hash only nominates: compared entry by entry)
                        for (int w = 0; w < 4 && same; ++w) {
                            const RefDfa &d = p->t.dfa[w];
                            for (int32_t st = 0; st < d.n_states && same; ++st) same = d.table[(size_t)st * N + j] == d.table[(size_t)st * N + k];
                        }
                        if (same) {
                            canon[k] = canon[j];
                            break;
                        }
                    }
                }
            }
            // (a char beyond an automaton's maxChar takes the `c > maxChar` exit there: only classes whose column is dead in that
            // automaton reach beyond it, so class equality covers it -- checked below for the chars the rule relies on)
            uint32_t n_of[256] = {0};
            for (uint8_t c : cm) ++n_of[canon[c]];
            int other = 0;
            for (int k = 1; k < 256; ++k)
                if (n_of[k] > n_of[other]) other = k;
            int page = -1;
            bool one = true;
            for (int c = 0; c < 65536 && one; ++c)
                if (canon[cm[c]] != other) {
                    if (page < 0) page = c >> 8;
                    else one = page == (c >> 8);
                }
            // "dead beyond maxChar" must be what the other class does anyway in the automata that have a maxChar below 0xFFFF
            for (int w = 0; w < 4 && one; ++w) {
                const RefDfa &d = p->t.dfa[w];
                if (d.max_char >= 0xFFFF) continue;
                for (int k = 0; k < N && one; ++k)
                    if (canon[k] == other)
                        for (int32_t st = 0; st < d.n_states && one; ++st) one = d.table[(size_t)st * N + k] < 0;
            }
            if (one && page >= 0) {
                for (int b = 255; b >= 0; --b)
                    if (canon[cm[(size_t)(page << 8) | b]] == other) {
                        p->u16_page = page, p->u16_sub = b;
                        break;
                    }
            }
        }
    }
    r.page = p->u16_page, r.sub = p->u16_sub;
    return r;
}

// NEEDLE_FIND_LENGTHS: 0 = find() always by forward + backward walks, 1 (default) = the "lengths" automaton where the ordinary
// program is a plain LDS table, 2 = also instead of the pair table (measured slower: DESIGN.md s4)
static int find_lengths_level() {
    static const int level = getenv("NEEDLE_FIND_LENGTHS") ? atoi(getenv("NEEDLE_FIND_LENGTHS")) : 1;
    return level;
}
static bool find_lengths_for(uint32_t mode) {
    static const bool sparse_too = (getenv("NEEDLE_FIND_LENGTHS_SPARSE") ? atoi(getenv("NEEDLE_FIND_LENGTHS_SPARSE")) : 1) != 0;
    static const bool pair_too = (getenv("NEEDLE_FIND_LENGTHS_PAIR") ? atoi(getenv("NEEDLE_FIND_LENGTHS_PAIR")) : 1) != 0;
    const int level = find_lengths_level();
    return level > 0 && (mode == MODE_TABLE8 || mode == MODE_TABLE16 || (sparse_too && mode == MODE_SPARSE) || ((pair_too || level > 1) && mode == MODE_PAIR));
}
// THE decision on find()'s lengths form -- the state the walk stops in remembers how long the match was, start = end - pend[state], no
// indexBackwards, no text snapshots (needle_lower.h): given the mode of the ordinary program and the mode the lengths program came out in,
// is the lengths program taken?  Where the ordinary program is a plain LDS table (the modes pend[] can be indexed in) -- but a pair-table
// automaton whose lengths program no longer fits the pair table keeps its two walks: two chars per lookup beat the saved backward walk
// (NEEDLE_FIND_LENGTHS=2 takes the plain table all the same).  NEEDLE_FIND_LENGTHS=0: never (A/B, tests).
static bool takes_lengths_form(uint32_t ordinary_mode, uint32_t lengths_mode) {
    const bool pair_lost = ordinary_mode == MODE_PAIR && lengths_mode != MODE_PAIR && find_lengths_level() <= 1;
    return find_lengths_for(ordinary_mode) && !pair_lost;
}
// The lengths program find() takes in place of ordinary program fp on this device, or *lp_out = nullptr: it keeps fp and walks back.
static int lengths_program(needle_pattern *p, int cw, const DevProgram *fp, const DevProgram **lp_out) {
    *lp_out = nullptr;
    if (!find_lengths_for(fp->prog.hdr.mode)) return NEEDLE_OK; // (not even lowered)
    const DevProgram *lp = nullptr;
    int rc = get_program(p, W_FORWARDS, cw, V_LENGTHS, &lp, nullptr);
    if (rc) return rc;
    if (lp && takes_lengths_form(fp->prog.hdr.mode, lp->prog.hdr.mode)) *lp_out = lp;
    return NEEDLE_OK;
}

// The WIDE filter (lower_filter_wide) stands in for the UTF-16 scan kernels where the ordinary UTF-16 program is NOT a plain LDS table
// (compressed automaton, hot rows + HBM table, HBM table): a latency-bound or collapsing walk.  NEEDLE_PREFILTER=2: for every
// automaton that allows a filter (tests, A/B), as for 8-bit rows.  NEEDLE_PREFILTER_WIDE=0: never.
static bool wide_filter_wanted(uint32_t ordinary_mode) {
    // (NEEDLE_PREFILTER_UTF16=0: no filter in front of UTF-16 rows at all -- the one-page route and this one)
    static const bool wide_off = (getenv("NEEDLE_PREFILTER_WIDE") ? atoi(getenv("NEEDLE_PREFILTER_WIDE")) : 1) == 0;
    if (wide_off || prefilter_utf16_off() || ngram_level() <= 0) return false;
    return ordinary_mode == MODE_SPARSE || ordinary_mode == MODE_HYBRID || ordinary_mode == MODE_GLOBAL || ngram_level() > 1;
}

// Few, long rows of an automaton too big for function composition: speculative stripes (needle_stripe.hip).  Returns
// NEEDLE_OK with *done = false when the path does not apply or did not reach its fixpoint (the caller then walks the
// rows one lane each).  scan_stripes(view, bitmap, start, end, end_state): the fixed-stride scan that runs pass 1 -- every stripe as a row
// of its own, with its end state and without backward walks.
template <class ScanStripes>
static int run_speculative_stripes(needle_pattern *p, int op, const needle_batch_view *v, uint64_t *d_bitmap, int32_t *d_start,
                                   int32_t *d_end, void *stream_, bool *done, ScanStripes &&scan_stripes) {
    *done = false;
    const int force = long_rows_force();
    const uint64_t stride_bytes = v->row_stride * v->char_width;
    // measured (scripts/mid_rows_table_rate.py): containedIn gains up to 60 000 rows; find breaks even around 20 000;
    // matches() usually dies in the first chars of a row, which only the lane path turns into an early exit
    const uint64_t max_rows = op == OP_CONTAINED_IN ? 65536 : op == OP_FIND ? 8192 : 256;
    const bool wanted = force >= 0 ? force == 1 : (v->n_rows < max_rows && stride_bytes >= 8 * (uint64_t)kStripeBytes);
    if (!wanted) return NEEDLE_OK;
    uint32_t stripe = kStripeBytes; // largest power of two <= 4 KiB that divides the row stride
    while (stripe > 256 && stride_bytes % stripe) stripe >>= 1;
    if (stride_bytes % stripe || stride_bytes / stripe < 2) return NEEDLE_OK;
    const int which = which_of(op);
    if (op != OP_MATCHES && p->t.dfa[which].accepting[0]) return NEEDLE_OK; // an accepting start state makes every stripe start look like a match
    const DevProgram *gp = nullptr, *fp = nullptr, *bp = nullptr;
    int n_cus = 0;
    int rc = get_program(p, which, (int)v->char_width, V_HBM_TABLE, &gp, &n_cus); // column maps + uint16 table
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    SpecArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.rows = (const uint8_t *)v->rows;
    sa.n_rows = v->n_rows;
    sa.stride_bytes = stride_bytes;
    sa.stripe_bytes = stripe;
    sa.spr = (uint32_t)(stride_bytes / stripe);
    sa.char_width = v->char_width;
    sa.op = (uint32_t)op;
    sa.row_len = v->row_len;
    sa.lengths = v->lengths;
    sa.gprog = gp->d_blob;
    sa.hdr = gp->prog.hdr;
    const size_t ns = (size_t)(sa.n_rows * sa.spr), words = (ns + 63) / 64;
    // slen | spec_end_state | spec_last | spec_start(unused) | entry | entry_done | true_end_state | true_last  (4 B each), bitmap, flag
    uint8_t *tmp = nullptr;
    const size_t o_bm = 8 * ns * 4, o_flag = o_bm + words * 8, total = o_flag + 16;
    HIP_TRY(scratch_malloc((void **)&tmp, total, stream));
    auto finish = [&](int code) {
        (void)scratch_free(tmp, stream);
        return code;
    };
    uint32_t *u = (uint32_t *)tmp;
    sa.slen = u;
    uint32_t *spec_end_state = u + ns;
    int32_t *spec_last = (int32_t *)(u + 2 * ns), *spec_start = (int32_t *)(u + 3 * ns);
    sa.spec_end_state = spec_end_state;
    sa.spec_last = spec_last;
    sa.entry = u + 4 * ns;
    sa.entry_done = u + 5 * ns;
    sa.true_end_state = u + 6 * ns;
    sa.true_last = (int32_t *)(u + 7 * ns);
    sa.spec_bitmap = (const uint64_t *)(tmp + o_bm);
    sa.changed = (int32_t *)(tmp + o_flag);
    sa.bitmap = d_bitmap;
    sa.end = d_end;
    hipError_t e = launch_spec_len(sa, stream);
    if (e != hipSuccess) return finish(hip_fail(e, "spec_len"));
    // pass 1: every stripe as a row of its own, from the start state, through the tiled kernel
    needle_batch_view sv;
    memset(&sv, 0, sizeof(sv));
    sv.rows = v->rows;
    sv.char_width = v->char_width;
    sv.n_rows = ns;
    sv.row_stride = stripe / v->char_width;
    sv.lengths = sa.slen;
    rc = scan_stripes(&sv, (uint64_t *)(tmp + o_bm), spec_start, spec_last, spec_end_state);
    if (rc) return finish(rc);
    e = launch_spec_init(sa, stream);
    if (e != hipSuccess) return finish(hip_fail(e, "spec_init"));
    bool fixed = false;
    for (int round = 0; round < 48 && !fixed; ++round) {
        if (hipMemsetAsync(sa.changed, 0, 4, stream) != hipSuccess) return finish(fail(NEEDLE_ERR_DEVICE, "hipMemsetAsync"));
        e = launch_spec_fix(sa, stream);
        int32_t changed = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&changed, sa.changed, 4, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return finish(hip_fail(e, "spec_fix"));
        fixed = changed == 0;
    }
    if (!fixed) return finish(NEEDLE_OK); // e.g. a DOTALL `.*` tail: every round settles one more stripe only
    if (op != OP_FIND && hipMemsetAsync(d_bitmap, 0, ((sa.n_rows + 63) / 64) * 8, stream) != hipSuccess)
        return finish(fail(NEEDLE_ERR_DEVICE, "hipMemsetAsync"));
    e = launch_spec_reduce(sa, stream);
    if (e != hipSuccess) return finish(hip_fail(e, "spec_reduce"));
    if (op == OP_FIND) { // matched bits + start: indexBackwards from lastMatch, one lane per row
        rc = get_program(p, W_FORWARDS, (int)v->char_width, p->t.fixed_len < 0 ? V_BACKMAPS : V_PLAIN, &fp, nullptr);
        if (rc) return finish(rc);
        if (p->t.fixed_len < 0 && (rc = backward_program(p, (int)v->char_width, &bp))) return finish(rc);
        e = launch_find_starts((int)v->char_width, v->rows, v->n_rows, stride_bytes, fp, bp, p->t.fixed_len, d_bitmap, d_start, d_end, stream);
        if (e != hipSuccess) return finish(hip_fail(e, "backward_rows"));
    }
    *done = true;
    return finish(NEEDLE_OK);
}

// ---- What each filter route picks.  *tp_out == nullptr: not this route.  The ORDER of the routes and their preconditions are choose_route's.
// UTF-16 rows of a pattern on ONE page of the BMP: the byte program of that page, the text narrowed on load (utf16_route, narrow16).  Every
// step is speculative -- lowering and uploading the page's byte programs for a pattern that may have no filter at all -- so a failure
// means "route unavailable", never an error.
static void filter_route_utf16_page(needle_pattern *p, int op, int which, bool need_backward, const Utf16Route &u16, const DevProgram **tp_out, int *n_cus) {
    *tp_out = nullptr;
    const DevProgram *tp = nullptr;
    const int cw8 = 1 | (u16.page << 8); // the byte program of the pattern's page
    if (get_program(p, which, cw8, need_backward ? V_BACKMAPS : V_PLAIN, &tp, n_cus)) return;
    bool ok = false;
    if (tp->prog.hdr.mode == MODE_HYBRID || tp->prog.hdr.mode == MODE_GLOBAL) {
        if (get_program(p, which, cw8, V_FILTER_HBM, &tp, nullptr)) return;
        ok = tp && tp->d_ng && tp->prog.ng.p.on && (op == OP_CONTAINED_IN || tp->prog.hdr.fa_len_off || p->t.fixed_len >= 0);
    } else {
        bool lengths8 = false;
        if (need_backward) {
            const DevProgram *lp = nullptr;
            if (lengths_program(p, cw8, tp, &lp)) return;
            // (this route never trades a pair table away, not even under NEEDLE_FIND_LENGTHS=2: such a program carries no filter anyway)
            if (lp && !(tp->prog.hdr.mode == MODE_PAIR && lp->prog.hdr.mode != MODE_PAIR)) tp = lp, lengths8 = true;
        }
        ok = tp->d_ng && tp->prog.ng.p.on && (op == OP_CONTAINED_IN || lengths8 || p->t.fixed_len >= 0);
    }
    if (ok) *tp_out = tp;
}
// UTF-16 rows of a pattern on SEVERAL pages: the WIDE filter's program, where wide_filter_wanted() says so for the ordinary UTF-16
// program's mode.
static int filter_route_wide(needle_pattern *p, int op, int which, const DevProgram **tp_out) {
    *tp_out = nullptr;
    const DevProgram *tp = nullptr;
    int rc = get_program(p, which, 2, V_FILTER_WIDE, &tp, nullptr);
    if (rc) return rc;
    if (tp && tp->d_ng && tp->prog.ng.p.on && (op == OP_CONTAINED_IN || tp->prog.hdr.fa_len_off || p->t.fixed_len >= 0)) *tp_out = tp;
    return NEEDLE_OK;
}
// NEEDLE_PREFILTER_UNBOUNDED=0: find() of a pattern without bounded match lengths never runs behind the filter.
static bool prefilter_unbounded_on() {
    static const bool on = (getenv("NEEDLE_PREFILTER_UNBOUNDED") ? atoi(getenv("NEEDLE_PREFILTER_UNBOUNDED")) : 1) != 0;
    return on;
}
// 8-bit rows of an automaton that fits the LDS in no form (hot rows + HBM table, or the HBM table alone): the filter with verify walks out
// of HBM / L2 (V_FILTER_HBM).  allow_unbounded: find() without bounded match lengths may take the forward search automaton + backward walks
// for the starts (V_FILTER_UNBOUNDED, *bwp_out = the backward program).
static int filter_route_hbm(needle_pattern *p, int op, int which, bool need_backward, bool allow_unbounded, const DevProgram **tp_out, const DevProgram **bwp_out) {
    *tp_out = *bwp_out = nullptr;
    const DevProgram *tp = nullptr;
    int rc = get_program(p, which, 1, V_FILTER_HBM, &tp, nullptr);
    if (rc) return rc;
    const DevProgram *bwp = nullptr;
    if (!tp && op == OP_FIND && need_backward && prefilter_unbounded_on() && allow_unbounded) {
        rc = get_program(p, which, 1, V_FILTER_UNBOUNDED, &tp, nullptr);
        if (rc) return rc;
        if (tp) {
            rc = backward_program(p, 1, &bwp);
            if (rc) return rc;
            if (!bwp) tp = nullptr;
        }
    }
    if (tp && tp->d_ng && tp->prog.ng.p.on && (op == OP_CONTAINED_IN || tp->prog.hdr.fa_len_off || p->t.fixed_len >= 0 || bwp)) *tp_out = tp, *bwp_out = bwp;
    return NEEDLE_OK;
}

// ---- THE route of a call: which program, and which kernel family, serves (pattern, op, char width, what the call carries) -- one
// decision for fixed-stride rows (run_dev) and packed rows (run_packed_dev), so that a pattern takes the same program on both.
struct Route {
    enum Kind {
        SCAN,   // the layout's plain scan kernel walks fp (+ bp)
        FILTER, // the layout's n-gram filter kernel runs in front of fp (+ bp): launched by the time choose_route returns
        DONE    // one of the layout's own paths (RouteCaps / own_paths) has served the call
    } kind = SCAN;
    const DevProgram *fp = nullptr; // the forward program
    const DevProgram *bp = nullptr; // the backward program find() walks for its starts; nullptr: none needed
    bool lengths_form = false;      // SCAN: fp is find()'s lengths program (start = end - pend[state])
    bool own_filter = false;        // SCAN: fp carries a filter of its own that this call may take: the caller offers it to its filter tail first
    int page = 0, sub = 0xFF;       // FILTER in front of UTF-16 rows: the page the byte program stands for and the byte of every char outside it
    int n_cus = 0;
};
// What the layout, its kernels and the call's arguments allow.  The defaults leave every route open.
struct RouteCaps {
    bool filter = true;         // a filter kernel may serve the call at all
    bool stand_in = true;       // ... with a program OTHER than the one the plain kernel would walk (routes 1, 3 and 4 below)
    bool utf16 = true;          // the UTF-16 filter routes (1 and 3) are open
    bool unbounded_find = true; // find() of a pattern without bounded match lengths may run behind the filter, its starts by backward walks
    bool lengths_form = true;   // find() may take the lengths program
};
// The routes in their order -- the first that applies and that its layout's filter tail launches is the call's:
//   1. UTF-16 rows, pattern on ONE page of the BMP: the filter of that page's byte program.  Tried BEFORE the ordinary UTF-16 program is asked
//      for: a call it serves does not lower that program.
//   2. the ordinary program of (op, char width): what the plain kernel walks, and what decides the routes below.
//   3. UTF-16 rows, pattern on SEVERAL pages, wide_filter_wanted(ordinary mode): the WIDE filter program.
//      -- own_paths(r, &done): the layout's own kernels, once the ordinary program is known (fixed stride: the stripe paths) --
//   4. 8-bit rows, ordinary program a hot-rows / HBM-table one: the filter program with its walks out of HBM / L2.
//   5. find() without one match length: the lengths program in place of the ordinary one (lengths_program), else the backward program.
//   6. 8-bit rows, the program of 5 carries a filter of its own: Route::own_filter -- the caller's last filter launch, in front of its plain kernel.
// try_filter(candidate, &launched) is the layout's filter tail: its kernel's gate, then the flood watch (which counts: asked LAST, once per
// candidate that passed the gate), the launch, the stats copy.  launched == false: the order goes on.
// No filter route at all for matches(), under NEEDLE_PREFILTER=0, or where caps.filter says no.  Where the two layouts DIFFER, on purpose:
//   - fixed stride: per-row cursors, the speculative-stripe pass (d_end_state, no_backward) close every filter route, and that pass keeps the
//     ordinary program (no lengths form); packed: cursors close the filter routes, NEEDLE_PREFILTER_PACKED=0 does too.
//   - find() of a pattern without bounded match lengths behind a filter (V_FILTER_UNBOUNDED in route 4, backward walks in route 6) is fixed-stride
//     only: the packed filter kernel has no backward walk.
//   - the gates (inside try_filter): fixed stride asks ngram_shape_ok (stride 64 .. 4096 B, >= 16 KiB in all, ...) and ngram_lds_bytes; packed has no
//     shape gate, but the four modes its kernel is instantiated for, fixed_len <= 65535 and ngram_packed_lds_bytes.
//   - fixed stride closes routes 1 and 3 from a stride of 8 x kStripeBytes on (such rows are the stripe paths'); packed rows have no stride.
//   - fixed stride, measurement builds: NEEDLE_DICT closes routes 1, 3 and 4 (caps.stand_in), not 6.
template <class TryFilter, class OwnPaths>
static int choose_route(needle_pattern *p, int op, int cw, const RouteCaps &caps, TryFilter &&try_filter, OwnPaths &&own_paths, Route *r) {
    const int which = which_of(op);
    const bool need_backward = op == OP_FIND && p->t.fixed_len < 0;
    const bool filter = caps.filter && op != OP_MATCHES && ngram_level() > 0, stand_in = filter && caps.stand_in;
    const Utf16Route u16 = cw == 2 ? utf16_route(p) : Utf16Route();
    bool served = false;
    auto offer = [&](const DevProgram *tp, const DevProgram *bwp, int page, int sub) {
        Route c = *r;
        c.kind = Route::FILTER, c.fp = tp, c.bp = bwp, c.page = page, c.sub = sub;
        const int rc = try_filter(c, &served);
        if (served) *r = c;
        return rc;
    };
    int rc = NEEDLE_OK;
    if (stand_in && cw == 2 && caps.utf16 && u16.page >= 0) { // 1
        const DevProgram *tp = nullptr;
        filter_route_utf16_page(p, op, which, need_backward, u16, &tp, &r->n_cus);
        if (tp && ((rc = offer(tp, nullptr, u16.page, u16.sub)) || served)) return rc;
    }
    rc = get_program(p, which, cw, need_backward ? V_BACKMAPS : V_PLAIN, &r->fp, &r->n_cus); // 2
    if (rc) return rc;
    if (stand_in && cw == 2 && caps.utf16 && u16.page < 0 && wide_filter_wanted(r->fp->prog.hdr.mode)) { // 3
        const DevProgram *tp = nullptr;
        rc = filter_route_wide(p, op, which, &tp);
        if (rc) return rc;
        if (tp && ((rc = offer(tp, nullptr, 0, 0)) || served)) return rc;
    }
    rc = own_paths(r, &served);
    if (served) r->kind = Route::DONE;
    if (rc || served) return rc;
    if (stand_in && cw == 1 && (r->fp->prog.hdr.mode == MODE_HYBRID || r->fp->prog.hdr.mode == MODE_GLOBAL)) { // 4
        const DevProgram *tp = nullptr, *bwp = nullptr;
        rc = filter_route_hbm(p, op, which, need_backward, caps.unbounded_find, &tp, &bwp);
        if (rc) return rc;
        if (tp && ((rc = offer(tp, bwp, 0, 0xFF)) || served)) return rc;
    }
    if (need_backward && caps.lengths_form) { // 5
        const DevProgram *lp = nullptr;
        rc = lengths_program(p, cw, r->fp, &lp);
        if (rc) return rc;
        if (lp) r->fp = lp, r->lengths_form = true;
    }
    if (need_backward && !r->lengths_form) {
        rc = backward_program(p, cw, &r->bp);
        if (rc) return rc;
    }
    // 6 (find() without bounded match lengths: verified candidates find their starts by indexBackwards, the lock-step backward walk on text out of L2)
    const bool by_backward_walk = r->bp && caps.unbounded_find && prefilter_unbounded_on();
    r->own_filter = filter && cw == 1 && r->fp->d_ng && r->fp->prog.ng.p.on && (op == OP_CONTAINED_IN || r->lengths_form || p->t.fixed_len >= 0 || by_backward_walk);
    return NEEDLE_OK;
}

// THE tail of a fixed-stride filter launch (needle_ngram.hip) of program tp: the kernel's gate -- the batch's shape, the LDS footprint --, the
// flood watch LAST (it counts what it allows), the launch, the stats copy behind it.  *launched == false: the call goes on to its next route.
static int launch_filter(const needle_pattern *p, int op, const ScanArgs &a, const DevProgram *tp, int n_cus, hipStream_t stream, int cw, int page, int sub,
                         bool *launched) {
    *launched = false;
    if (!ngram_shape_ok(a) || !ngram_lds_bytes(a.hdr, tp->prog.ng.p) || !ngram_watch_allows(p, tp)) return NEEDLE_OK;
    HIP_TRY(launch_ngram(op, a, tp->prog.ng.p, tp->d_ng, tp->d_ng_stats, n_cus, stream, cw, page, sub));
    HIP_TRY(ngram_watch_after_launch(tp, stream));
    *launched = true;
    return NEEDLE_OK;
}

// d_packed (OP_FIND, needle_find_packed16_dev): a row's start / end go there as one dword, stored by the scan kernel itself;
// d_start / d_end are not used.  The paths for few long rows (stripes) and the opt-in two-row-set kernel keep their int32
// arrays: they run into scratch and one pack pass follows.
// d_end_state / no_backward: the speculative-stripe pass (every stripe's end state; only lastMatch is wanted).
static int run_dev(const needle_pattern *cp, int op, const needle_batch_view *v, uint64_t *d_bitmap, int32_t *d_start, int32_t *d_end, void *stream_,
                   const int32_t *d_from = nullptr, uint32_t *d_end_state = nullptr, bool no_backward = false, uint32_t *d_packed = nullptr,
                   bool packed8 = false) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_view(v);
    if (rc) return rc;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!d_bitmap) return fail(NEEDLE_ERR_INVALID, "bitmap is NULL");
    if (op == OP_FIND && !d_packed && (!d_start || !d_end)) return fail(NEEDLE_ERR_INVALID, "start/end is NULL");
    hipStream_t stream = (hipStream_t)stream_;
#ifdef NEEDLE_TUNING
    static const int dict_env = getenv("NEEDLE_DICT") ? atoi(getenv("NEEDLE_DICT")) : 0;
#else
    constexpr int dict_env = 0;
#endif
    const int cw = (int)v->char_width;
    const uint64_t stride_bytes = v->row_stride * v->char_width;
    // (NEEDLE_LONG_ROWS=1 forces the stripe paths for any stride: they only know the int32 arrays)
    if (d_packed && (dict_env > 0 || long_rows_force() == 1 || stride_bytes >= 8 * (uint64_t)kStripeBytes)) {
        if (packed8) return fail(NEEDLE_ERR_UNSUPPORTED, "needle_find_packed8_dev: not on the stripe / two-row-set paths (tuning switches)");
        int32_t *tmp = nullptr;
        HIP_TRY(scratch_malloc((void **)&tmp, (size_t)v->n_rows * 8, stream));
        rc = run_dev(cp, op, v, d_bitmap, tmp, tmp + v->n_rows, stream_, d_from, d_end_state, no_backward, nullptr);
        if (rc == NEEDLE_OK) rc = needle_pack_start_end16_dev(tmp, tmp + v->n_rows, v->n_rows, d_packed, stream_);
        (void)scratch_free(tmp, stream);
        return rc;
    }
    const ScanOut out{d_bitmap, d_start, d_end, d_packed, packed8};
    const int32_t fixed_len = op == OP_FIND ? p->t.fixed_len : -1;
    RouteCaps caps;
    caps.filter = !d_from && !d_end_state && !no_backward;
    caps.stand_in = dict_env == 0;
    caps.utf16 = v->row_stride * 2 < 8 * (uint64_t)kStripeBytes; // (longer rows: the stripe paths')
    caps.lengths_form = !d_end_state && !no_backward;
    // (UTF-16 rows behind a byte program or the WIDE one: the stride in CHARS; 8-bit rows: the same number)
    auto try_filter = [&](const Route &c, bool *launched) {
        return launch_filter(p, op, scan_args(v, v->row_stride, c.fp, c.bp, fixed_len, out), c.fp, c.n_cus, stream, cw, c.page, c.sub, launched);
    };
    // Few long rows, once the ordinary program is known: function composition across stripes (packed-mode automata), speculative stripes (the
    // others); what is left walks its rows one lane each.
    auto stripe_paths = [&](Route *r, bool *done) -> int {
        if (d_end_state && (r->fp->prog.hdr.mode == MODE_HYBRID || r->fp->prog.hdr.mode == MODE_SPARSE)) {
            // the speculative-stripe pass wants every stripe's end state in the numbering of the HBM-table layout its fix-up
            // kernel walks; the hot-rows and compressed forms number / encode states their own way
            int rc = get_program(p, which_of(op), cw, V_HBM_TABLE, &r->fp, &r->n_cus);
            if (rc) return rc;
        }
        if (!d_end_state && wants_stripe_path(v, r->fp->prog.hdr, d_from != nullptr)) {
            *done = true;
            return run_stripe_path(p, op, v, r->fp, r->n_cus, d_bitmap, d_start, d_end, stream_);
        }
        if (!d_end_state && !d_from && r->fp->prog.hdr.mode != MODE_PACK) {
            // (pass 1: every stripe as a row of its own, through this function again)
            auto scan_stripes = [&](const needle_batch_view *sv, uint64_t *bm, int32_t *st, int32_t *en, uint32_t *end_state) {
                return run_dev(cp, op, sv, bm, st, en, stream_, nullptr, end_state, true);
            };
            int rc = run_speculative_stripes(p, op, v, d_bitmap, d_start, d_end, stream_, done, scan_stripes);
            if (rc || *done) return rc;
        }
        // the tiled kernel forms per-lane row offsets in 32 bits (up to 63 x stride); only the stripe paths above take
        // rows of tens of megabytes and more
        if (stride_bytes >= (1ull << 26))
            return fail(NEEDLE_ERR_UNSUPPORTED, "rows of 64 MiB or more are only supported on the stripe paths (automata of at most 5 states, or ones that re-synchronise; not with NEEDLE_LONG_ROWS=0, per-row cursors or empty-matching patterns)");
        return NEEDLE_OK;
    };
    Route r;
    rc = choose_route(p, op, cw, caps, try_filter, stripe_paths, &r);
    if (rc || r.kind != Route::SCAN) return rc;
    ScanArgs a = scan_args(v, stride_bytes, r.fp, r.bp, fixed_len, out);
    a.from = d_from;
    a.end_state = d_end_state;
    bool skip_backward = no_backward; // (speculative pass: only lastMatch is wanted)
#ifdef NEEDLE_TUNING // measurement builds only (scripts/build_tuning.sh): a switch that changes ANSWERS (start = end) never ships
    skip_backward = skip_backward || debug_no_backward();
#endif
    if (skip_backward && op == OP_FIND) a.fixed_len = 0, a.bprog = nullptr;
#ifdef NEEDLE_TUNING
    // Big automata on full 8-bit rows: two 64-row sets per wave (needle_dict.hip) over the whole 128-row pairs of the batch, the
    // ordinary kernel on what is left; find()'s starts by indexBackwards afterwards, one lane per matched row.
    // Measurement builds only (scripts/build_tuning.sh).  NEEDLE_DICT: 0 off (default: measured, it is no faster -- DESIGN.md s4),
    // 1 on for the compressed automaton, 2 also for plain uint16 LDS tables.
    if (dict_env > 0 && !r.lengths_form && (a.hdr.mode == MODE_SPARSE || dict_env > 1) && dict_kernel_applies(cw, a)) {
        HIP_TRY(launch_dict(op, a, r.n_cus, stream));
        const uint64_t done_rows = (a.n_rows >> 7) << 7;
        if (op == OP_FIND && a.fixed_len < 0 && done_rows) {
            HIP_TRY(launch_find_starts(cw, a.rows, done_rows, a.stride_bytes, r.fp, r.bp, -1, d_bitmap, d_start, d_end, stream));
        }
        if (done_rows == a.n_rows) return NEEDLE_OK;
        a.rows += done_rows * a.stride_bytes; // the last n_rows % 128 rows
        a.n_rows -= done_rows;
        a.total_bytes = a.n_rows * a.stride_bytes;
        a.bitmap += done_rows >> 6;
        if (a.start) a.start += done_rows, a.end += done_rows;
    }
#endif
    // The n-gram candidate filter (needle_ngram.hip): the automaton only runs where a hashed 4-byte window of the
    // text can stand ahead of a match.  For programs whose lowering established that this gives the reference's answers
    // (needle_ngram_host.cpp), on containedIn() and on find() whose start is end - length (lengths programs, one-length patterns) or
    // comes from a backward walk (choose_route, route 6).
    if (r.own_filter && !skip_backward) {
        bool launched = false;
        rc = launch_filter(p, op, a, r.fp, r.n_cus, stream, 1, 0, 0xFF, &launched);
        if (rc || launched) return rc;
    }
    HIP_TRY(launch_scan(op, cw, a, r.n_cus, stream));
    return NEEDLE_OK;
}

// The program the PER-LANE find-all kernels walk for this pattern on rows of cw -- find_all_kernel (fixed-stride rows, needle_find_all.hip)
// and packed_find_all_lane_kernel (packed rows, needle_packed_find_all_lane.h) -- and how its matches find their starts: one choice for
// both layouts.  Asked through `get`, which answers with a variant's program header (nullptr: the pattern has none): get_program on a
// device, a host-side lowering for needle_pattern_find_all_packed_route.
struct LaneChoice {
    Variant variant = V_FA_PLAIN; // the forward program
    const ProgHeader *hdr = nullptr;
    bool lmode = false;         // the "lengths" automaton: start = end - pend[end state]
    bool need_backward = false; // starts by indexBackwards on the backward program
    uint32_t defer = 0;         // FindAllArgs::defer
};
static int find_all_lengths_level() {
    static const int v = getenv("NEEDLE_FIND_ALL_LENGTHS") ? atoi(getenv("NEEDLE_FIND_ALL_LENGTHS")) : 1;
    return v;
}
template <class Get>
static int find_all_lane_choice(const needle_pattern *p, bool count_only, Get &&get, LaneChoice *c) {
    *c = LaneChoice();
    c->need_backward = p->t.fixed_len < 0;
    int rc = NEEDLE_OK;
    // start = end - (the match length the automaton's end state remembers): no backward walks at all, when the pattern
    // allows it (needle_lower.h: keyword unions and the like).  NEEDLE_FIND_ALL_LENGTHS=0: off (A/B, tests).
    const int lengths_level = find_all_lengths_level();
    if (c->need_backward && lengths_level != 0 && !count_only) {
        if ((rc = get(V_FA_LENGTHS, &c->hdr))) return rc;
        c->lmode = c->hdr != nullptr;
        c->variant = V_FA_LENGTHS;
        if (!c->lmode && lengths_level > 1 && find_lengths_for(MODE_SPARSE)) {
            // no plain LDS table holds the lengths automaton (a big dictionary): the scan kernels' compressed form of it, if there is
            // one.  Opt-in (NEEDLE_FIND_ALL_LENGTHS=2): measured on C3-sparse (profiles/r04_find_all.md) it is no faster than hot rows +
            // backward walks, 2.05 against 1.98 ms -- the per-lane piece walk is what costs there, not the 0.25 starts per row
            const ProgHeader *sp = nullptr;
            if ((rc = get(V_LENGTHS, &sp))) return rc;
            if (sp && sp->mode == MODE_SPARSE) c->hdr = sp, c->lmode = true, c->variant = V_LENGTHS;
        }
        if (c->lmode) c->need_backward = false;
    }
    if (!c->lmode) {
        c->variant = c->need_backward ? V_FA_BACKMAPS : V_FA_PLAIN;
        if ((rc = get(c->variant, &c->hdr))) return rc;
        if (!c->hdr) return fail(NEEDLE_ERR_UNSUPPORTED, "find_all: the pattern has no program");
    }
    static const bool no_defer = (getenv("NEEDLE_FIND_ALL_DEFER") ? atoi(getenv("NEEDLE_FIND_ALL_DEFER")) : 1) == 0; // A/B, tests
    c->defer = (p->t.fixed_len < 0 && !c->hdr->root_accepting && !no_defer && !c->lmode) ? 1u : 0u;
#ifdef NEEDLE_TUNING // measurement builds only: start = the search cursor (wrong answers; never in the shipping library)
    if (c->defer && debug_no_backward()) c->defer = 2;
#endif
    return NEEDLE_OK;
}
// The choice on the current device: the programs themselves.
struct LaneProgram {
    const DevProgram *fp = nullptr, *bp = nullptr;
    bool lmode = false;
    uint32_t defer = 0;
    int n_cus = 0;
};
static int find_all_lane_program(needle_pattern *p, int cw, bool count_only, LaneProgram *lp) {
    *lp = LaneProgram();
    LaneChoice c;
    int rc = find_all_lane_choice(p, count_only, [&](Variant v, const ProgHeader **h) {
        const DevProgram *dp = nullptr;
        const int r = get_program(p, W_FORWARDS, cw, v, &dp, &lp->n_cus);
        *h = (r == NEEDLE_OK && dp) ? &dp->prog.hdr : nullptr;
        return r;
    }, &c);
    if (rc) return rc;
    if ((rc = get_program(p, W_FORWARDS, cw, c.variant, &lp->fp, &lp->n_cus))) return rc; // (resident by now)
    lp->lmode = c.lmode;
    lp->defer = c.defer;
    if (c.need_backward && (rc = backward_program(p, cw, &lp->bp))) return rc;
    return NEEDLE_OK;
}

// The program the n-gram filter kernel's FIND-ALL form runs on for this pattern on rows of cw (needle_ngram.hip OP_NG_FIND_ALL; packed rows:
// needle_ngram_packed.h) -- one choice for both layouts.  As find() chooses its filter: the 8-bit program find() walks (plain table for a
// pattern of one length, else the lengths form) where it carries a filter, else the filter with its walks out of HBM / L2; UTF-16 rows of a
// pattern on one page of the BMP: that page's byte programs, the text narrowed as it is loaded (utf16_route); on several pages: the WIDE
// filter where find() would take it (choose_route, route 3).  Asked through `get`, which answers with a variant's program at char width
// cw | page << 8 (nullptr: the pattern has none): get_program on a device, a host-side lowering for
// needle_pattern_find_all_packed_filter.  c->prog == nullptr: no filter for this pattern.  NEEDLE_FIND_ALL_FILTER=0: off (A/B, tests).
struct FilterChoice {
    const Program *prog = nullptr;
    Variant variant = V_PLAIN;
    int cw_key = 1;          // the program's char width | page << 8
    int page = 0, sub = 0xFF; // what the launchers are told about UTF-16 rows behind a byte program
};
template <class Get>
static int find_all_filter_choice(const needle_pattern *p, int cw, Get &&get, FilterChoice *c) {
    *c = FilterChoice();
    static const bool fa_filter = (getenv("NEEDLE_FIND_ALL_FILTER") ? atoi(getenv("NEEDLE_FIND_ALL_FILTER")) : 1) != 0;
    if (!fa_filter || ngram_level() <= 0 || !(p->t.fixed_len >= 0 || find_lengths_for(MODE_SPARSE))) return NEEDLE_OK;
    // (UTF-16 rows of a pattern on one page of the BMP: that page's byte programs, the text narrowed as it is loaded -- utf16_route)
    const Utf16Route u16 = cw == 2 ? utf16_route(p) : Utf16Route();
    int rc = NEEDLE_OK;
    const Program *sp = nullptr;
    if (cw == 2 && u16.page < 0) { // several pages of the BMP: the WIDE filter, where find() would take it (choose_route, route 3)
        const Program *op16 = nullptr;
        if ((rc = get(2, p->t.fixed_len < 0 ? V_BACKMAPS : V_PLAIN, &op16))) return rc;
        if (op16 && wide_filter_wanted(op16->hdr.mode)) {
            c->cw_key = 2, c->variant = V_FILTER_WIDE;
            if ((rc = get(c->cw_key, c->variant, &sp))) return rc;
        }
    } else {
        c->cw_key = 1 | ((cw == 2 ? u16.page : 0) << 8);
        c->variant = p->t.fixed_len >= 0 ? V_PLAIN : V_LENGTHS;
        if ((rc = get(c->cw_key, c->variant, &sp))) return rc;
        if (!(sp && sp->ng.p.on)) { // an automaton that fits the LDS in no form: the filter with its walks out of HBM / L2
            c->variant = V_FILTER_HBM;
            if ((rc = get(c->cw_key, c->variant, &sp))) return rc;
        }
    }
    if (sp && sp->ng.p.on) c->prog = sp;
    c->page = u16.page > 0 ? u16.page : 0, c->sub = cw == 2 ? u16.sub : 0xFF;
    return NEEDLE_OK;
}
// The choice on the current device: the resident program (nullptr: no filter).
static int find_all_filter_program(needle_pattern *p, int cw, FilterChoice *c, const DevProgram **sp, int *n_cus) {
    *sp = nullptr;
    int rc = find_all_filter_choice(p, cw, [&](int cw_key, Variant v, const Program **pr) {
        const DevProgram *dp = nullptr;
        const int r = get_program(p, W_FORWARDS, cw_key, v, &dp, n_cus);
        *pr = (r == NEEDLE_OK && dp) ? &dp->prog : nullptr;
        return r;
    }, c);
    if (rc || !c->prog) return rc;
    if ((rc = get_program(p, W_FORWARDS, c->cw_key, c->variant, sp, n_cus))) return rc; // (resident by now)
    if (*sp && !(*sp)->d_ng) *sp = nullptr;
    return NEEDLE_OK;
}

// The "more" flag of a one-pass find-all launch: a zeroed scratch word the kernel sets when some row has a match beyond its last slot.
// launch(d_more) enqueues the kernel (and what belongs behind it); the flag is read back -- the call's only synchronisation -- only when the
// caller asked whether its slots sufficed (more != nullptr).  d_more[1] is a second zeroed word for a flag of the launch's own (the packed
// kernel's "a row is too long"), read back with the first into *second when the caller asked for it.
template <class Launch>
static int with_more_flag(hipStream_t stream, int *more, const char *what, Launch &&launch, int *second = nullptr) {
    int32_t *d_more = nullptr;
    HIP_TRY(scratch_malloc((void **)&d_more, 16, stream));
    hipError_t e = hipMemsetAsync(d_more, 0, 8, stream);
    if (e == hipSuccess) e = launch(d_more);
    int32_t h[2] = {0, 0};
    if (e == hipSuccess && (more || second)) {
        e = hipMemcpyAsync(h, d_more, 8, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
    }
    (void)scratch_free(d_more, stream);
    if (e != hipSuccess) return hip_fail(e, what);
    if (more) *more = h[0] != 0;
    if (second) *second = h[1] != 0;
    return NEEDLE_OK;
}

// The find-all transducer program of a pattern for rows of cw: the lengths transducer, else -- for a pattern without bounded match lengths
// -- the RUN transducer (`[0-9]+`, `[a-z]{3}[a-z]*`: starts from a per-lane run-start register), or *tp = nullptr.  The order of
// needle_pattern_find_all_transducer.  lengths_on / runs_on: the caller's switches.
static int find_all_transducer_program(needle_pattern *p, int cw, bool lengths_on, bool runs_on, const DevProgram **tp, int *n_cus) {
    *tp = nullptr;
    int rc = NEEDLE_OK;
    if (lengths_on && (rc = get_program(p, W_FORWARDS, cw, V_FA_TRANSDUCER, tp, n_cus))) return rc;
    if (!*tp && runs_on && p->t.fixed_len < 0) rc = get_program(p, W_FORWARDS, cw, V_FA_RUNS, tp, n_cus);
    return rc;
}

int needle::check_packed(const needle_packed_view *v) {
    if (!v) return fail(NEEDLE_ERR_INVALID, "packed view is NULL");
    if (v->char_width != 1 && v->char_width != 2) return fail(NEEDLE_ERR_INVALID, "char_width must be 1 or 2");
    if (!v->offsets) return fail(NEEDLE_ERR_INVALID, "offsets is NULL");
    return NEEDLE_OK;
}

static int check_packed_dev(const needle_pattern *p, const needle_packed_view *v) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    return NEEDLE_OK;
}

// Packed device batches scanned as they lie (needle_packed.h): no conversion to fixed-stride rows, no host synchronisation.  The route --
// the program, and whether the n-gram candidate filter (needle_ngram_packed.h) runs in front of it -- is choose_route's, as for fixed-stride
// rows: one lowering serves both layouts, with the same flood watch, the same counters and the same needle_pattern_set_prefilter pin.
// What is this layout's own is listed there.  NEEDLE_PREFILTER_PACKED=0: packed rows never take the filter (A/B).
// find() only: d_from = per-row cursors (needle_find_next_packed_dev); d_packed = the result as one dword per row, or one uint16 with
// packed8 (needle_find_packed{16,8}_packed_dev: start / end are not used), d_overflow = optional flag of rows that escaped that form.
static int run_packed_dev(const needle_pattern *cp, int op, const needle_packed_view *v, uint64_t *d_bitmap, int32_t *d_start,
                          int32_t *d_end, void *stream_, const int32_t *d_from = nullptr, uint32_t *d_packed = nullptr, bool packed8 = false,
                          int32_t *d_overflow = nullptr) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    int rc = check_packed_dev(p, v);
    if (rc) return rc;
    if (!d_bitmap) return fail(NEEDLE_ERR_INVALID, "bitmap is NULL");
    if (op == OP_FIND && !d_packed && (!d_start || !d_end)) return fail(NEEDLE_ERR_INVALID, "start/end is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const int cw = (int)v->char_width;
    const ScanOut out{d_bitmap, d_start, d_end, d_packed, packed8};
    const int32_t fixed_len = op == OP_FIND ? p->t.fixed_len : -1;
    static const bool pf_packed_on = (getenv("NEEDLE_PREFILTER_PACKED") ? atoi(getenv("NEEDLE_PREFILTER_PACKED")) : 1) != 0;
    RouteCaps caps;
    caps.filter = pf_packed_on && !d_from;
    caps.unbounded_find = false; // (the packed filter kernel has no backward walk)
    // The packed filter tail: no shape gate -- the kernel is right for any amount of text -- but the modes it is instantiated for (the ones a
    // filter is ever built on), a match length its slot key can hold (16 bits) and its LDS footprint; then the flood watch, LAST.
    auto try_filter = [&](const Route &c, bool *launched) -> int {
        *launched = false;
        const DevProgram *tp = c.fp;
        const uint32_t m = tp->prog.hdr.mode;
        if (m != MODE_TABLE8 && m != MODE_TABLE16 && m != MODE_SPARSE && m != MODE_GLOBAL) return NEEDLE_OK;
        if (op == OP_FIND && p->t.fixed_len > 65535) return NEEDLE_OK;
        if (!ngram_packed_lds_bytes(tp->prog.hdr, tp->prog.ng.p) || !ngram_watch_allows(p, tp)) return NEEDLE_OK;
        const ScanArgs sa = scan_args(v, tp, nullptr, fixed_len, out);
        HIP_TRY(launch_ngram_packed(op, sa, v->offsets, d_overflow, tp->prog.ng.p, tp->d_ng, tp->d_ng_stats, c.n_cus, stream, cw, c.page, c.sub));
        HIP_TRY(ngram_watch_after_launch(tp, stream));
        *launched = true;
        return NEEDLE_OK;
    };
    Route r;
    rc = choose_route(p, op, cw, caps, try_filter, [](Route *, bool *) { return (int)NEEDLE_OK; }, &r);
    if (rc || r.kind != Route::SCAN) return rc;
    if (r.own_filter) {
        bool launched = false;
        rc = try_filter(r, &launched);
        if (rc || launched) return rc;
    }
    PackedArgs a;
    memset(&a, 0, sizeof(a));
    a.s = scan_args(v, r.fp, r.bp, fixed_len, out);
    a.s.from = d_from;
    a.offsets = v->offsets;
    a.overflow = d_packed ? d_overflow : nullptr;
    HIP_TRY(launch_packed(op, cw, a, r.n_cus, stream));
    return NEEDLE_OK;
}

// ------------------------------------------------------------------------------------------------
// Every match of every row of a packed batch (needle_*_packed_dev of find-all; needle_packed_find_all.h)
// ------------------------------------------------------------------------------------------------
// The one answer to "does this program take the packed find-all kernel on rows of char_width": a find-all transducer whose program
// and the windows of at least the smallest shape fit the LDS.  The routing below and needle_pattern_find_all_transducer (what the
// tests read) both ask it.
static bool packed_find_all_takes(const ProgHeader &h, int char_width) {
    int waves = 0, chb = 0;
    return h.ft_on && packed_find_all_shape(h.lds_bytes, char_width, &waves, &chb);
}

// The transducer program the packed find-all kernel walks for this pattern and char width (find_all_transducer_program; the packed
// entries honour none of the fixed-stride entries' switches), or *tp = nullptr: the pattern goes by conversion.
static int packed_find_all_program(needle_pattern *p, int cw, const DevProgram **tp, int *n_cus) {
    const int rc = find_all_transducer_program(p, cw, true, true, tp, n_cus);
    if (rc) return rc;
    if (*tp && !packed_find_all_takes((*tp)->prog.hdr, cw)) *tp = nullptr;
    return NEEDLE_OK;
}

// One launch of the packed find-all kernel.  more / too_long (optional, host): read back after one synchronisation of the stream.
static int packed_find_all_launch(const needle_packed_view *v, const DevProgram *tp, int n_cus, uint32_t *d_counts, const uint64_t *d_offsets,
                                  int32_t *d_start, int32_t *d_end, uint32_t slots, uint32_t *d_blocks, bool count_only, int *more, int *too_long,
                                  hipStream_t stream) {
    PackedFindAllArgs a;
    memset(&a, 0, sizeof(a));
    a.f.s = scan_args(v, tp, nullptr, -1, ScanOut());
    a.f.counts = d_counts;
    a.f.offsets = d_offsets;
    a.f.starts = d_start;
    a.f.ends = d_end;
    a.f.slots = slots;
    a.f.packed = d_blocks;
    a.f.kshift = d_blocks ? 6u : 0u;
    a.f.count_only = count_only ? 1u : 0u;
    a.row_offsets = v->offsets;
    return with_more_flag(stream, more, "find_all (packed kernel)", [&](int32_t *d_more) {
        a.f.more = d_more;
        a.too_long = d_blocks ? d_more + 1 : nullptr;
        return launch_packed_find_all((int)v->char_width, a, n_cus, stream);
    }, too_long);
}

// The one answer to "does this per-lane find-all program take the packed per-lane kernel on rows of char_width"
// (needle_packed_find_all_lane.h): a packed-function or LDS-table program whose image and the windows of at least the smallest shape
// fit the LDS.  Hot-rows, HBM-table and compressed programs go by conversion.  NEEDLE_PACKED_FIND_ALL_LANE=0: off (A/B, tests: the
// conversion route).  The routing below and needle_pattern_find_all_packed_route both ask it.
static bool packed_find_all_lane_takes(const ProgHeader &h, int char_width) {
    static const bool lane_on = (getenv("NEEDLE_PACKED_FIND_ALL_LANE") ? atoi(getenv("NEEDLE_PACKED_FIND_ALL_LANE")) : 1) != 0;
    int waves = 0, chb = 0;
    return lane_on && packed_find_all_lane_mode(h.mode) && packed_find_all_lane_shape(h.lds_bytes, char_width, &waves, &chb);
}

// Patterns without a transducer whose per-lane program the packed per-lane kernel takes: one stream-ordered launch on the packed text,
// no offsets read-back, no chunks.  *taken = false: the pattern goes by conversion.
static int packed_find_all_lane(needle_pattern *p, const needle_packed_view *v, uint32_t *d_counts, const uint64_t *d_offsets, int32_t *d_start,
                                int32_t *d_end, bool count_only, int *more, hipStream_t stream, bool *taken) {
    *taken = false;
    const int cw = (int)v->char_width;
    LaneProgram lp;
    int rc = find_all_lane_program(p, cw, count_only, &lp);
    if (rc) return rc;
    if (!packed_find_all_lane_takes(lp.fp->prog.hdr, cw)) return NEEDLE_OK;
    *taken = true;
    PackedFindAllArgs a;
    memset(&a, 0, sizeof(a));
    a.f.s = scan_args(v, lp.fp, lp.bp, p->t.fixed_len, ScanOut());
    a.f.counts = d_counts;
    a.f.offsets = d_offsets;
    a.f.starts = d_start;
    a.f.ends = d_end;
    a.f.count_only = count_only ? 1u : 0u;
    a.f.lmode = lp.lmode ? 1u : 0u;
    a.f.defer = lp.defer;
    a.row_offsets = v->offsets;
    return with_more_flag(stream, more, "find_all (packed per-lane kernel)", [&](int32_t *d_more) {
        a.f.more = d_more;
        return launch_packed_find_all_lane(cw, a, lp.n_cus, stream);
    });
}

// Patterns without a packed find-all program: the offsets are read back ONCE (a synchronisation of the stream), consecutive rows are
// converted chunk by chunk -- each chunk at its own stride, its padded bytes within 4x its text + 64 KiB -- by needle_rows_from_packed_dev
// and run through the fixed-stride entry.  Per-row counts and absolute CSR offsets need no merge step.
static int packed_find_all_by_conversion(needle_pattern *p, const needle_packed_view *v, uint32_t *d_counts, const uint64_t *d_offsets,
                                         int32_t *d_start, int32_t *d_end, int *more, hipStream_t stream) {
    const uint64_t n = v->n_rows, cw = v->char_width;
    std::vector<uint64_t> off((size_t)n + 1);
    HIP_TRY(hipMemcpyAsync(off.data(), v->offsets, (n + 1) * 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    struct Chunk {
        uint64_t r0, r1, stride_bytes;
    };
    std::vector<Chunk> chunks;
    uint64_t biggest = 0;
    auto stride_of = [&](uint64_t len) { return std::max<uint64_t>(16, (len * cw + 15) & ~(uint64_t)15); };
    for (uint64_t r0 = 0; r0 < n;) {
        uint64_t r1 = r0, longest = 0;
        while (r1 < n) {
            if (off[r1 + 1] < off[r1]) return fail(NEEDLE_ERR_INVALID, "offsets must be non-decreasing");
            const uint64_t l = std::max<uint64_t>(longest, off[r1 + 1] - off[r1]);
            if (stride_of(l) >= (1ull << 26)) return fail(NEEDLE_ERR_UNSUPPORTED, "rows of 64 MiB or more: not on the packed find-all entries");
            if (r1 > r0 && (r1 + 1 - r0) * stride_of(l) > 4 * (off[r1 + 1] - off[r0]) * cw + (64u << 10)) break;
            longest = l;
            ++r1;
        }
        chunks.push_back({r0, r1, stride_of(longest)});
        biggest = std::max<uint64_t>(biggest, (r1 - r0) * (stride_of(longest) + 4));
        r0 = r1;
    }
    uint8_t *tmp = nullptr; // rows | lengths of the biggest chunk (reused: every chunk runs on the same stream)
    HIP_TRY(scratch_malloc((void **)&tmp, biggest + 256, stream));
    auto done = [&](int code) {
        (void)scratch_free(tmp, stream);
        return code;
    };
    if (more) *more = 0;
    for (const Chunk &c : chunks) {
        const uint64_t nr = c.r1 - c.r0;
        uint32_t *d_len = (uint32_t *)(tmp + ((nr * c.stride_bytes + 255) & ~(uint64_t)255));
        needle_packed_view sub = *v;
        sub.offsets = v->offsets + c.r0;
        sub.n_rows = nr;
        int rc = needle_rows_from_packed_dev(&sub, tmp, c.stride_bytes / cw, d_len, nullptr, stream);
        if (rc) return done(rc);
        needle_batch_view bv;
        memset(&bv, 0, sizeof(bv));
        bv.rows = tmp;
        bv.char_width = v->char_width;
        bv.n_rows = nr;
        bv.row_stride = c.stride_bytes / cw;
        bv.lengths = d_len;
        int m = 0;
        rc = d_counts ? needle_count_matches_dev(p, &bv, d_counts + c.r0, stream)
                      : needle_find_all_csr_dev(p, &bv, d_offsets + c.r0, d_start, d_end, more ? &m : nullptr, stream);
        if (rc) return done(rc);
        if (more && m) *more = 1;
    }
    return done(NEEDLE_OK);
}

// Big dictionaries -- no transducer, a program the per-lane kernel does not take (compressed, hot rows, HBM table) -- behind the n-gram
// candidate filter's find-all form on the packed text itself (needle_ngram_packed.h): one stream-ordered launch, no offsets read-back, no
// chunks, rows of any length.  The filter program is the fixed-stride rows' (find_all_filter_choice); what is this layout's own:
//   NEEDLE_PREFILTER_PACKED=0 (no filter in front of packed rows at all) and NEEDLE_FIND_ALL_FILTER_PACKED=0 (this route only; A/B, tests),
//   no shape gate -- the kernel is right for any amount of text -- but the modes it is instantiated for, a one-length pattern of at most
//   65 535 chars (the candidate entry's fields) and its own LDS footprint.
// The two predicates below are what the routing and needle_pattern_find_all_packed_filter both ask.
static bool packed_find_all_filter_on() {
    static const bool on = (getenv("NEEDLE_PREFILTER_PACKED") ? atoi(getenv("NEEDLE_PREFILTER_PACKED")) : 1) != 0 &&
                           (getenv("NEEDLE_FIND_ALL_FILTER_PACKED") ? atoi(getenv("NEEDLE_FIND_ALL_FILTER_PACKED")) : 1) != 0;
    return on;
}
static bool packed_find_all_filter_takes(const needle_pattern *p, const Program &pr) {
    const uint32_t m = pr.hdr.mode;
    if (m != MODE_TABLE8 && m != MODE_TABLE16 && m != MODE_SPARSE && m != MODE_GLOBAL) return false;
    if (p->t.fixed_len > 65535) return false;
    return pr.ng.p.on && ngram_packed_find_all_lds_bytes(pr.hdr, pr.ng.p) != 0;
}
// *taken = false: the batch goes by conversion (no filter program, or the flood watch / the pin declined this call).
static int packed_find_all_filter(needle_pattern *p, const needle_packed_view *v, uint32_t *d_counts, const uint64_t *d_offsets, int32_t *d_start,
                                  int32_t *d_end, bool count_only, int *more, hipStream_t stream, bool *taken) {
    *taken = false;
    if (!packed_find_all_filter_on()) return NEEDLE_OK;
    const int cw = (int)v->char_width;
    FilterChoice fc;
    const DevProgram *sp = nullptr;
    int cus = 0;
    int rc = find_all_filter_program(p, cw, &fc, &sp, &cus);
    if (rc) return rc;
    if (!sp || !packed_find_all_filter_takes(p, sp->prog) || !ngram_watch_allows(p, sp)) return NEEDLE_OK; // (the flood watch LAST: it counts the call)
    *taken = true;
    const ScanArgs a = scan_args(v, sp, nullptr, p->t.fixed_len, ScanOut());
    return with_more_flag(stream, more, "find_all (packed filter kernel)", [&](int32_t *d_more) {
        hipError_t e = launch_ngram_packed_find_all(a, v->offsets, sp->prog.ng.p, sp->d_ng, sp->d_ng_stats, d_counts, d_start, d_end, d_more, d_offsets, count_only,
                                                    cus, stream, cw, fc.page, fc.sub);
        if (e == hipSuccess) e = ngram_watch_after_launch(sp, stream);
        return e;
    });
}

// The packed find-all entries' route: the transducer kernel, else the per-lane kernel, else the filter kernel, else conversion.
static int packed_find_all_route(needle_pattern *p, const needle_packed_view *v, uint32_t *d_counts, const uint64_t *d_offsets, int32_t *d_start,
                                 int32_t *d_end, bool count_only, int *more, hipStream_t stream) {
    const DevProgram *tp = nullptr;
    int n_cus = 0;
    int rc = packed_find_all_program(p, (int)v->char_width, &tp, &n_cus);
    if (rc) return rc;
    if (tp) return packed_find_all_launch(v, tp, n_cus, d_counts, d_offsets, d_start, d_end, 0, nullptr, count_only, more, nullptr, stream);
    bool taken = false;
    rc = packed_find_all_lane(p, v, d_counts, d_offsets, d_start, d_end, count_only, more, stream, &taken);
    if (rc || taken) return rc;
    rc = packed_find_all_filter(p, v, d_counts, d_offsets, d_start, d_end, count_only, more, stream, &taken);
    if (rc || taken) return rc;
    return packed_find_all_by_conversion(p, v, d_counts, d_offsets, d_start, d_end, more, stream);
}

extern "C" {

int needle_count_matches_packed_dev(const needle_pattern *cp, const needle_packed_view *v, uint32_t *d_counts, void *stream_) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    int rc = check_packed_dev(p, v);
    if (rc) return rc;
    if (!d_counts) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    return packed_find_all_route(p, v, d_counts, nullptr, nullptr, nullptr, true, nullptr, (hipStream_t)stream_);
}

int needle_find_all_csr_packed_dev(const needle_pattern *cp, const needle_packed_view *v, const uint64_t *d_offsets, int32_t *d_start,
                                   int32_t *d_end, int *more, void *stream_) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    int rc = check_packed_dev(p, v);
    if (rc) return rc;
    if (!d_offsets || !d_start || !d_end) return fail(NEEDLE_ERR_INVALID, "offsets / output buffer is NULL");
    if (more) *more = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    return packed_find_all_route(p, v, nullptr, d_offsets, d_start, d_end, false, more, (hipStream_t)stream_);
}

// The splice (needle_replace.hip): pure functions of (text, match list, replacement) -- no pattern, no route.  The checks of the packed
// device entries, then the kernels' arguments; n_rows == 0 has returned before this is called.
static int replace_args(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_start, const int32_t *d_end, uint32_t repl_len,
                        ReplaceArgs *a) {
    int rc = check_packed(v);
    if (rc) return rc;
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    if (!d_match_offsets) return fail(NEEDLE_ERR_INVALID, "match offsets is NULL");
    if (repl_len > NEEDLE_REPLACE_MAX_UNITS) return fail(NEEDLE_ERR_INVALID, "replacement longer than NEEDLE_REPLACE_MAX_UNITS code units");
    memset(a, 0, sizeof(*a));
    a->data = (const uint8_t *)v->data;
    a->in_off = v->offsets;
    a->n_rows = v->n_rows;
    a->cw = v->char_width;
    a->repl_len = repl_len;
    a->match_off = d_match_offsets;
    a->start = d_start;
    a->end = d_end;
    return NEEDLE_OK;
}

int needle_replace_all_lengths_packed_dev(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_start,
                                          const int32_t *d_end, uint32_t repl_len, uint64_t *d_out_lengths, void *stream_) {
    ReplaceArgs a;
    int rc = replace_args(v, d_match_offsets, d_start, d_end, repl_len, &a);
    if (rc) return rc;
    if (!d_out_lengths) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    a.out_len = d_out_lengths;
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_TRY(launch_replace_lengths(a, cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

int needle_replace_all_fill_packed_dev(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_start,
                                       const int32_t *d_end, const void *repl, uint32_t repl_len, const uint64_t *d_out_offsets,
                                       void *d_out_data, void *stream_) {
    ReplaceArgs a;
    int rc = replace_args(v, d_match_offsets, d_start, d_end, repl_len, &a);
    if (rc) return rc;
    if (!d_out_offsets || !d_out_data) return fail(NEEDLE_ERR_INVALID, "output offsets / buffer is NULL");
    if (((uintptr_t)d_out_data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "output data must be 4-byte aligned");
    if (repl_len && !repl) return fail(NEEDLE_ERR_INVALID, "replacement is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    a.out_off = d_out_offsets;
    a.out = (uint8_t *)d_out_data;
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const uint32_t bytes = repl_len * v->char_width;
    uint8_t *d_repl = nullptr; // (whole 16 bytes: the kernel stages it with 16-byte loads)
    if (bytes) HIP_TRY(scratch_malloc((void **)&d_repl, (bytes + 15u) & ~15u, stream));
    hipError_t e = bytes ? launch_replace_put(repl, bytes, d_repl, stream) : hipSuccess;
    a.repl = d_repl;
    if (e == hipSuccess) e = launch_replace_fill(a, cus, stream);
    if (d_repl) (void)scratch_free(d_repl, stream);
    return e == hipSuccess ? NEEDLE_OK : hip_fail(e, "needle_replace_all_fill_packed_dev");
}

// The splice with a replacement per match (needle_replace_each.hip): the checks of replace_args, then the table's and the choices'.
// `repl` is checked by the fill entry alone (the lengths entry has none).
static int replace_each_args(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_start, const int32_t *d_end,
                             const void *d_choice, int choice_form, const uint32_t *repl_offsets, uint32_t n_repl, ReplaceEachArgs *a) {
    ReplaceArgs plain;
    int rc = replace_args(v, d_match_offsets, d_start, d_end, 0, &plain);
    if (rc) return rc;
    if (choice_form != NEEDLE_CHOICE_INDEX && choice_form != NEEDLE_CHOICE_LOWEST_BIT)
        return fail(NEEDLE_ERR_INVALID, "choice_form is neither NEEDLE_CHOICE_INDEX nor NEEDLE_CHOICE_LOWEST_BIT");
    if (!repl_offsets) return fail(NEEDLE_ERR_INVALID, "replacement offsets is NULL");
    if (n_repl < 1 || n_repl > NEEDLE_REPLACE_MAX_CHOICES) return fail(NEEDLE_ERR_INVALID, "1 .. NEEDLE_REPLACE_MAX_CHOICES replacements");
    if (repl_offsets[0] != 0) return fail(NEEDLE_ERR_INVALID, "replacement offsets must start at 0");
    for (uint32_t i = 0; i < n_repl; ++i)
        if (repl_offsets[i + 1] < repl_offsets[i]) return fail(NEEDLE_ERR_INVALID, "replacement offsets decrease");
    if (repl_offsets[n_repl] > NEEDLE_REPLACE_MAX_UNITS)
        return fail(NEEDLE_ERR_INVALID, "replacement table longer than NEEDLE_REPLACE_MAX_UNITS code units");
    memset(a, 0, sizeof(*a));
    a->data = plain.data;
    a->in_off = plain.in_off;
    a->n_rows = plain.n_rows;
    a->cw = plain.cw;
    a->n_repl = n_repl;
    a->choice_form = (uint32_t)choice_form;
    a->table_units = repl_offsets[n_repl];
    a->match_off = d_match_offsets;
    a->start = d_start;
    a->end = d_end;
    a->choice = (const uint32_t *)d_choice;
    return NEEDLE_OK;
}

// The table on the device, in stream order: its offsets (kReplaceEachOffsetBytes, zeros behind n_repl + 1) and, with_units, its code
// units behind them, through kernel arguments as the plain replacement goes (launch_replace_put): the caller's arrays are free on return.
static hipError_t replace_each_table(const void *repl, const uint32_t *repl_offsets, uint32_t n_repl, uint32_t cw, bool with_units, uint8_t **d_table,
                                     hipStream_t stream) {
    const uint32_t unit_bytes = with_units ? repl_offsets[n_repl] * cw : 0u;
    const uint32_t bytes = kReplaceEachOffsetBytes + ((unit_bytes + 15u) & ~15u);
    std::vector<uint8_t> host(bytes, 0);
    memcpy(host.data(), repl_offsets, (size_t)(n_repl + 1) * 4);
    if (unit_bytes) memcpy(host.data() + kReplaceEachOffsetBytes, repl, unit_bytes);
    hipError_t e = scratch_malloc((void **)d_table, bytes, stream);
    if (e != hipSuccess) return e;
    return launch_replace_put(host.data(), bytes, *d_table, stream);
}

int needle_replace_each_lengths_packed_dev(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_start,
                                           const int32_t *d_end, const void *d_choice, int choice_form, const uint32_t *repl_offsets,
                                           uint32_t n_repl, uint64_t *d_out_lengths, void *stream_) {
    ReplaceEachArgs a;
    int rc = replace_each_args(v, d_match_offsets, d_start, d_end, d_choice, choice_form, repl_offsets, n_repl, &a);
    if (rc) return rc;
    if (!d_out_lengths) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    a.out_len = d_out_lengths;
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    uint8_t *d_table = nullptr;
    hipError_t e = replace_each_table(nullptr, repl_offsets, n_repl, v->char_width, false, &d_table, stream);
    a.table = d_table;
    if (e == hipSuccess) e = launch_replace_each_lengths(a, cus, stream);
    if (d_table) (void)scratch_free(d_table, stream);
    return e == hipSuccess ? NEEDLE_OK : hip_fail(e, "needle_replace_each_lengths_packed_dev");
}

int needle_replace_each_fill_packed_dev(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_start,
                                        const int32_t *d_end, const void *d_choice, int choice_form, const void *repl,
                                        const uint32_t *repl_offsets, uint32_t n_repl, const uint64_t *d_out_offsets, void *d_out_data,
                                        void *stream_) {
    ReplaceEachArgs a;
    int rc = replace_each_args(v, d_match_offsets, d_start, d_end, d_choice, choice_form, repl_offsets, n_repl, &a);
    if (rc) return rc;
    if (!d_out_offsets || !d_out_data) return fail(NEEDLE_ERR_INVALID, "output offsets / buffer is NULL");
    if (((uintptr_t)d_out_data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "output data must be 4-byte aligned");
    if (repl_offsets[n_repl] && !repl) return fail(NEEDLE_ERR_INVALID, "replacement table is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    hipStream_t stream = (hipStream_t)stream_;
    a.out_off = d_out_offsets;
    a.out = (uint8_t *)d_out_data;
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    uint8_t *d_table = nullptr;
    hipError_t e = replace_each_table(repl, repl_offsets, n_repl, v->char_width, true, &d_table, stream);
    a.table = d_table;
    if (e == hipSuccess) e = launch_replace_each_fill(a, cus, stream);
    if (d_table) (void)scratch_free(d_table, stream);
    return e == hipSuccess ? NEEDLE_OK : hip_fail(e, "needle_replace_each_fill_packed_dev");
}

// A replacement template into its canonical form (needle_template.h): host code, no device.
int needle_template_parse(const uint16_t *tmpl, size_t n_units, uint32_t n_groups, int32_t *groups, uint32_t groups_cap, uint32_t *lit_offsets,
                          uint32_t lit_offsets_cap, uint16_t *lits, uint32_t lits_cap, uint32_t *n_refs, uint32_t *n_lit_units) {
    if (!tmpl && n_units) return fail(NEEDLE_ERR_INVALID, "template is NULL");
    if ((!groups && groups_cap) || (!lit_offsets && lit_offsets_cap) || (!lits && lits_cap))
        return fail(NEEDLE_ERR_INVALID, "a NULL output has capacity 0");
    TemplateForm f;
    std::string err;
    if (!template_parse(tmpl, n_units, n_groups, &f, &err)) return fail(NEEDLE_ERR_INVALID, err);
    if (n_refs) *n_refs = (uint32_t)f.groups.size();
    if (n_lit_units) *n_lit_units = (uint32_t)f.lits.size();
    if ((groups && groups_cap < f.groups.size()) || (lit_offsets && lit_offsets_cap < f.lit_offsets.size()) || (lits && lits_cap < f.lits.size()))
        return fail(NEEDLE_ERR_INVALID, "an output's capacity is below the parsed template's size (call with NULL outputs to size it)");
    if (groups && !f.groups.empty()) memcpy(groups, f.groups.data(), f.groups.size() * sizeof(int32_t));
    if (lit_offsets) memcpy(lit_offsets, f.lit_offsets.data(), f.lit_offsets.size() * sizeof(uint32_t));
    if (lits && !f.lits.empty()) memcpy(lits, f.lits.data(), f.lits.size() * sizeof(uint16_t));
    return NEEDLE_OK;
}

// The splice with a template of literals and group references (needle_replace_groups.hip): the checks of replace_args, then the
// planes' and the template's; *table is what the put kernel takes to the device -- the head (the references' groups, a replaced
// match's pieces in output order) and, with_lits, the literals' units behind it.
static int replace_groups_args(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_group_start, const int32_t *d_group_end,
                               uint64_t plane_stride, uint32_t n_planes, const needle_template *t, bool with_lits, ReplaceGroupsArgs *a,
                               std::vector<uint8_t> *table) {
    ReplaceArgs plain;
    int rc = replace_args(v, d_match_offsets, d_group_start, d_group_end, 0, &plain);
    if (rc) return rc;
    if (n_planes == 0) return fail(NEEDLE_ERR_INVALID, "n_planes is 0: plane 0 is the match itself");
    if (!t) return fail(NEEDLE_ERR_INVALID, "template is NULL");
    if (!t->lit_offsets) return fail(NEEDLE_ERR_INVALID, "template literal offsets is NULL");
    if (t->n_refs > NEEDLE_TEMPLATE_MAX_REFS) return fail(NEEDLE_ERR_INVALID, "more than NEEDLE_TEMPLATE_MAX_REFS group references");
    if (t->n_refs && !t->groups) return fail(NEEDLE_ERR_INVALID, "template groups is NULL");
    const uint32_t K = t->n_refs;
    for (uint32_t k = 0; k < K; ++k)
        if (t->groups[k] < 0 || (uint32_t)t->groups[k] >= n_planes)
            return fail(NEEDLE_ERR_INVALID, "template reference " + std::to_string(k) + " names group " + std::to_string(t->groups[k]) + ": outside 0 .. n_planes - 1");
    if (t->lit_offsets[0] != 0) return fail(NEEDLE_ERR_INVALID, "template literal offsets must start at 0");
    for (uint32_t i = 0; i <= K; ++i)
        if (t->lit_offsets[i + 1] < t->lit_offsets[i]) return fail(NEEDLE_ERR_INVALID, "template literal offsets decrease");
    const uint32_t units = t->lit_offsets[K + 1];
    if (units > NEEDLE_REPLACE_MAX_UNITS) return fail(NEEDLE_ERR_INVALID, "template literals longer than NEEDLE_REPLACE_MAX_UNITS code units");
    if (with_lits && units && !t->lits) return fail(NEEDLE_ERR_INVALID, "template literals is NULL");
    const uint32_t cw = plain.cw, unit_bytes = with_lits ? units * cw : 0u;
    table->assign(kGroupsHeadBytes + ((unit_bytes + 15u) & ~15u), 0);
    uint32_t *head = (uint32_t *)table->data();
    uint32_t pieces = 0;
    for (uint32_t i = 0; i <= K; ++i) {
        const uint32_t lo = t->lit_offsets[i], len = t->lit_offsets[i + 1] - lo;
        if (len) head[kGroupsPieceWord0 + pieces++] = (lo * cw) | ((len * cw) << 14); // (an empty literal is no piece)
        if (i < K) {
            head[i] = (uint32_t)t->groups[i];
            head[kGroupsPieceWord0 + pieces++] = kGroupsRef | (uint32_t)t->groups[i];
        }
    }
    if (unit_bytes) memcpy(table->data() + kGroupsHeadBytes, t->lits, unit_bytes);
    memset(a, 0, sizeof(*a));
    a->data = plain.data;
    a->in_off = plain.in_off;
    a->n_rows = plain.n_rows;
    a->cw = cw;
    a->n_refs = K;
    a->lit_units = units;
    a->pieces = pieces + 1u; // (and the gap behind the match)
    a->chunk = kGroupsTableEntries / a->pieces;
    a->inv_pieces = (65536u + a->pieces - 1u) / a->pieces;
    a->match_off = d_match_offsets;
    a->gstart = d_group_start;
    a->gend = d_group_end;
    a->plane_stride = plane_stride;
    return NEEDLE_OK;
}

static int replace_groups_run(ReplaceGroupsArgs &a, const std::vector<uint8_t> &table, bool fill, hipStream_t stream, const char *what) {
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    uint8_t *d_table = nullptr;
    hipError_t e = scratch_malloc((void **)&d_table, table.size(), stream);
    if (e == hipSuccess) e = launch_replace_put(table.data(), (uint32_t)table.size(), d_table, stream);
    a.table = d_table;
    if (e == hipSuccess) e = fill ? launch_replace_groups_fill(a, cus, stream) : launch_replace_groups_lengths(a, cus, stream);
    if (d_table) (void)scratch_free(d_table, stream);
    return e == hipSuccess ? NEEDLE_OK : hip_fail(e, what);
}

int needle_replace_groups_lengths_packed_dev(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_group_start,
                                             const int32_t *d_group_end, uint64_t plane_stride, uint32_t n_planes, const needle_template *tmpl,
                                             uint64_t *d_out_lengths, void *stream_) {
    ReplaceGroupsArgs a;
    std::vector<uint8_t> table;
    int rc = replace_groups_args(v, d_match_offsets, d_group_start, d_group_end, plane_stride, n_planes, tmpl, false, &a, &table);
    if (rc) return rc;
    if (!d_out_lengths) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    a.out_len = d_out_lengths;
    return replace_groups_run(a, table, false, (hipStream_t)stream_, "needle_replace_groups_lengths_packed_dev");
}

int needle_replace_groups_fill_packed_dev(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_group_start,
                                          const int32_t *d_group_end, uint64_t plane_stride, uint32_t n_planes, const needle_template *tmpl,
                                          const uint64_t *d_out_offsets, void *d_out_data, void *stream_) {
    ReplaceGroupsArgs a;
    std::vector<uint8_t> table;
    int rc = replace_groups_args(v, d_match_offsets, d_group_start, d_group_end, plane_stride, n_planes, tmpl, true, &a, &table);
    if (rc) return rc;
    if (!d_out_offsets || !d_out_data) return fail(NEEDLE_ERR_INVALID, "output offsets / buffer is NULL");
    if (((uintptr_t)d_out_data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "output data must be 4-byte aligned");
    if (v->n_rows == 0) return NEEDLE_OK;
    a.out_off = d_out_offsets;
    a.out = (uint8_t *)d_out_data;
    return replace_groups_run(a, table, true, (hipStream_t)stream_, "needle_replace_groups_fill_packed_dev");
}

// Spans of packed rows as a new packed batch (needle_gather.hip): pure functions of (text, span list) -- no pattern, no route.  The checks
// the three entries share, then the kernels' arguments; n_rows == 0 has returned before the CU count is asked for.
static int gather_args(const needle_packed_view *v, const uint64_t *d_span_offsets, const int32_t *d_start, const int32_t *d_end, GatherArgs *a) {
    int rc = check_packed(v);
    if (rc) return rc;
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    if (!d_span_offsets) return fail(NEEDLE_ERR_INVALID, "span offsets is NULL");
    if ((d_start == nullptr) != (d_end == nullptr)) return fail(NEEDLE_ERR_INVALID, "start / end: one of them is NULL");
    memset(a, 0, sizeof(*a));
    a->data = (const uint8_t *)v->data;
    a->in_off = v->offsets;
    a->n_rows = v->n_rows;
    a->cw = v->char_width;
    a->span_off = d_span_offsets;
    a->start = d_start;
    a->end = d_end;
    return NEEDLE_OK;
}
static int gather_cus(int *cus) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    return NEEDLE_OK;
}

// (d_start / d_end may be NULL when the list is empty, which only the device knows: the kernels then dereference neither)
int needle_gather_spans_lengths_packed_dev(const needle_packed_view *v, const uint64_t *d_span_offsets, const int32_t *d_start,
                                           const int32_t *d_end, uint64_t *d_out_lengths, void *stream_) {
    GatherArgs a;
    int rc = gather_args(v, d_span_offsets, d_start, d_end, &a), cus = 0;
    if (rc) return rc;
    if (d_start && !d_out_lengths) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (v->n_rows == 0 || !d_start) return NEEDLE_OK;
    if ((rc = gather_cus(&cus))) return rc;
    a.out_len = d_out_lengths;
    HIP_TRY(launch_gather_lengths(a, cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

int needle_gather_spans_fill_packed_dev(const needle_packed_view *v, const uint64_t *d_span_offsets, const int32_t *d_start,
                                        const int32_t *d_end, const uint64_t *d_out_offsets, void *d_out_data, void *stream_) {
    GatherArgs a;
    int rc = gather_args(v, d_span_offsets, d_start, d_end, &a), cus = 0;
    if (rc) return rc;
    if (!d_out_offsets || !d_out_data) return fail(NEEDLE_ERR_INVALID, "output offsets / buffer is NULL");
    if (((uintptr_t)d_out_data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "output data must be 4-byte aligned");
    if (v->n_rows == 0 || !d_start) return NEEDLE_OK;
    if ((rc = gather_cus(&cus))) return rc;
    a.out_off = d_out_offsets;
    a.out = (uint8_t *)d_out_data;
    HIP_TRY(launch_gather_fill(a, cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

int needle_split_spans_packed_dev(const needle_packed_view *v, const uint64_t *d_match_offsets, const int32_t *d_start, const int32_t *d_end,
                                  uint64_t *d_piece_offsets, int32_t *d_piece_start, int32_t *d_piece_end, void *stream_) {
    GatherArgs a;
    int rc = gather_args(v, d_match_offsets, d_start, d_end, &a), cus = 0;
    if (rc) return rc;
    if (!d_piece_offsets || !d_piece_start || !d_piece_end) return fail(NEEDLE_ERR_INVALID, "piece offsets / output buffer is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    if ((rc = gather_cus(&cus))) return rc;
    a.piece_off = d_piece_offsets;
    a.piece_start = d_piece_start;
    a.piece_end = d_piece_end;
    HIP_TRY(launch_split_spans(a, cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

uint32_t needle_gather_chunk_spans(void) { return gather_chunk_spans(); }

// Equal spans of a list put into groups (needle_group.hip): a pure function of (text, span list) in the caller's workspace.  Every check
// runs before any device call; the table and the status are cleared on the stream, then the three kernels follow in stream order.
uint64_t needle_group_spans_work_bytes(uint64_t max_spans) { return group_layout(std::min<uint64_t>(max_spans, kGroupMaxSpans)).total; }

int needle_group_spans_packed_dev(const needle_packed_view *v, const uint64_t *d_span_offsets, const int32_t *d_start, const int32_t *d_end,
                                  uint64_t max_spans, uint32_t hash_bits, void *d_work, uint64_t work_bytes, uint64_t *d_first,
                                  uint32_t *d_count, uint32_t *d_status, void *stream_) {
    int rc = check_packed(v), cus = 0;
    if (rc) return rc;
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    if (!d_span_offsets) return fail(NEEDLE_ERR_INVALID, "span offsets is NULL");
    if ((d_start == nullptr) != (d_end == nullptr)) return fail(NEEDLE_ERR_INVALID, "start / end: one of them is NULL");
    if (!d_start && max_spans != 0) return fail(NEEDLE_ERR_INVALID, "start / end may be NULL only with max_spans == 0");
    if (max_spans > kGroupMaxSpans) return fail(NEEDLE_ERR_INVALID, "max_spans is above 2^32 - 2");
    if (hash_bits > 64) return fail(NEEDLE_ERR_INVALID, "hash_bits is above 64");
    if (!d_first || !d_count) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (!d_status) return fail(NEEDLE_ERR_INVALID, "status is NULL");
    if (!d_work) return fail(NEEDLE_ERR_INVALID, "workspace is NULL");
    if (((uintptr_t)d_work) % 16 != 0) return fail(NEEDLE_ERR_INVALID, "workspace must be 16-byte aligned");
    const GroupLayout lay = group_layout(max_spans);
    if (work_bytes < lay.total) return fail(NEEDLE_ERR_INVALID, "workspace is smaller than needle_group_spans_work_bytes(max_spans)");
    hipStream_t stream = (hipStream_t)stream_;
    if (v->n_rows == 0) {
        HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t), stream));
        return NEEDLE_OK;
    }
    if ((rc = gather_cus(&cus))) return rc;
    uint8_t *w = (uint8_t *)d_work;
    GroupArgs a;
    memset(&a, 0, sizeof(a));
    a.data = (const uint8_t *)v->data;
    a.in_off = v->offsets;
    a.n_rows = v->n_rows;
    a.cw = v->char_width;
    a.span_off = d_span_offsets;
    a.start = d_start;
    a.end = d_end;
    a.max_spans = max_spans;
    a.hash_mask = group_hash_mask(hash_bits);
    a.slots = lay.slots;
    a.w_addr = (uint64_t *)(w + lay.addr);
    a.w_hash = (uint64_t *)(w + lay.hash);
    a.w_slot = (uint64_t *)(w + lay.slot);
    a.w_len = (uint32_t *)(w + lay.len);
    a.w_word = (uint32_t *)(w + lay.word);
    a.w_count = (uint32_t *)(w + lay.count);
    a.first = d_first;
    a.count = d_count;
    a.status = d_status;
    HIP_TRY(hipMemsetAsync(d_status, 0, sizeof(uint32_t), stream));
    HIP_TRY(hipMemsetAsync(w + lay.clear_at, 0, lay.clear_bytes, stream));
    HIP_TRY(launch_group_spans(a, cus, stream));
    return NEEDLE_OK;
}

// The UTF-8 front door (needle_utf8.hip): pure functions of the text (and a position list) -- no pattern, no route.  The checks all
// three entries share, then the kernels' arguments and the device's CU count (n_rows == 0: not reached).
static int utf8_view_check(const needle_packed_view *v) {
    if (!v) return fail(NEEDLE_ERR_INVALID, "packed view is NULL");
    if (v->char_width != 1) return fail(NEEDLE_ERR_INVALID, "UTF-8 rows are a packed view of char_width 1");
    if (!v->offsets) return fail(NEEDLE_ERR_INVALID, "offsets is NULL");
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    return NEEDLE_OK;
}
static int utf8_args(const needle_packed_view *v, Utf8Args *a, int *cus) {
    memset(a, 0, sizeof(*a));
    a->data = (const uint8_t *)v->data;
    a->in_off = v->offsets;
    a->n_rows = v->n_rows;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev));
    return NEEDLE_OK;
}

int needle_utf16_lengths_from_utf8_packed_dev(const needle_packed_view *v, uint64_t *d_out_lengths, uint64_t *d_non_ascii, uint64_t *d_malformed,
                                              void *stream_) {
    int rc = utf8_view_check(v);
    if (rc) return rc;
    if (!d_out_lengths) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    Utf8Args a;
    int cus = 0;
    if ((rc = utf8_args(v, &a, &cus))) return rc;
    a.out_len = d_out_lengths;
    a.non_ascii = d_non_ascii;
    a.malformed = d_malformed;
    HIP_TRY(launch_utf8_lengths(a, cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

int needle_utf16_from_utf8_packed_dev(const needle_packed_view *v, const uint64_t *d_out_offsets, uint16_t *d_out_data, void *stream_) {
    int rc = utf8_view_check(v);
    if (rc) return rc;
    if (!d_out_offsets || !d_out_data) return fail(NEEDLE_ERR_INVALID, "output offsets / buffer is NULL");
    if (((uintptr_t)d_out_data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "output data must be 4-byte aligned");
    if (v->n_rows == 0) return NEEDLE_OK;
    Utf8Args a;
    int cus = 0;
    if ((rc = utf8_args(v, &a, &cus))) return rc;
    a.out_off = d_out_offsets;
    a.out = d_out_data;
    HIP_TRY(launch_utf8_fill(a, cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

// (d_unit_pos / d_byte_pos may be NULL when the list is empty, which only the device knows: the kernel then dereferences neither)
int needle_utf8_positions_packed_dev(const needle_packed_view *v, const uint64_t *d_list_offsets, const int32_t *d_unit_pos, int32_t *d_byte_pos,
                                     void *stream_) {
    int rc = utf8_view_check(v);
    if (rc) return rc;
    if (!d_list_offsets) return fail(NEEDLE_ERR_INVALID, "list offsets is NULL");
    if ((d_unit_pos == nullptr) != (d_byte_pos == nullptr)) return fail(NEEDLE_ERR_INVALID, "unit positions / byte positions: one of them is NULL");
    if (v->n_rows == 0 || !d_unit_pos) return NEEDLE_OK;
    Utf8Args a;
    int cus = 0;
    if ((rc = utf8_args(v, &a, &cus))) return rc;
    a.list_off = d_list_offsets;
    a.unit_pos = d_unit_pos;
    a.byte_pos = d_byte_pos;
    HIP_TRY(launch_utf8_positions(a, cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

uint32_t needle_utf8_window_bytes(void) { return utf8_window_bytes(); }

// Documents cut at their line terminators (needle_lines.hip): pure functions of the text -- no pattern, no route.  The checks both entries
// share, then the kernels' arguments; an empty batch has returned before the CU count is asked for.
static int lines_args(const needle_packed_view *v, uint64_t data_units, uint32_t flags, LinesArgs *a) {
    int rc = check_packed(v);
    if (rc) return rc;
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    if (flags & ~NEEDLE_LINES_KEEP_ENDS) return fail(NEEDLE_ERR_INVALID, "unknown flag bits");
    memset(a, 0, sizeof(*a));
    a->data = (const uint8_t *)v->data;
    a->in_off = v->offsets;
    a->n_rows = v->n_rows;
    a->cw = v->char_width;
    a->data_units = data_units;
    a->tiles = needle_lines_tiles(data_units, v->char_width);
    return NEEDLE_OK;
}

uint32_t needle_lines_tile_units(uint32_t char_width) { return lines_tile_units(char_width); }

uint64_t needle_lines_tiles(uint64_t data_units, uint32_t char_width) {
    const uint64_t t = lines_tile_units(char_width);
    return t ? data_units / t + (data_units % t != 0) : 0;
}

int needle_lines_count_packed_dev(const needle_packed_view *v, uint64_t data_units, uint32_t flags, uint64_t *d_tile_lines, uint64_t *d_tile_units,
                                  void *stream_) {
    LinesArgs a;
    int rc = lines_args(v, data_units, flags, &a), cus = 0;
    if (rc) return rc;
    if (!d_tile_lines) return fail(NEEDLE_ERR_INVALID, "tile lines is NULL");
    if (!(flags & NEEDLE_LINES_KEEP_ENDS) && !d_tile_units) return fail(NEEDLE_ERR_INVALID, "tile units is NULL without NEEDLE_LINES_KEEP_ENDS");
    if (v->n_rows == 0 || data_units == 0) return NEEDLE_OK;
    if ((rc = gather_cus(&cus))) return rc;
    a.tile_lines = d_tile_lines;
    a.tile_units = (flags & NEEDLE_LINES_KEEP_ENDS) ? nullptr : d_tile_units;
    HIP_TRY(launch_lines_count(a, cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

int needle_lines_fill_packed_dev(const needle_packed_view *v, uint64_t data_units, uint32_t flags, const uint64_t *d_tile_line_base,
                                 const uint64_t *d_tile_unit_base, uint64_t *d_out_offsets, void *d_out_data, uint64_t *d_doc_line_offsets,
                                 void *stream_) {
    LinesArgs a;
    int rc = lines_args(v, data_units, flags, &a), cus = 0;
    if (rc) return rc;
    const bool keep = (flags & NEEDLE_LINES_KEEP_ENDS) != 0;
    if (!d_tile_line_base || !d_out_offsets) return fail(NEEDLE_ERR_INVALID, "tile line base / output offsets is NULL");
    if (!keep && (!d_tile_unit_base || !d_out_data)) return fail(NEEDLE_ERR_INVALID, "tile unit base / output buffer is NULL without NEEDLE_LINES_KEEP_ENDS");
    if (!keep && ((uintptr_t)d_out_data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "output data must be 4-byte aligned");
    if (v->n_rows == 0 || data_units == 0) return NEEDLE_OK;
    if ((rc = gather_cus(&cus))) return rc;
    a.line_base = d_tile_line_base;
    a.unit_base = keep ? nullptr : d_tile_unit_base;
    a.out_off = d_out_offsets;
    a.out = keep ? nullptr : (uint8_t *)d_out_data;
    a.doc_lines = d_doc_line_offsets;
    HIP_TRY(launch_lines_fill(a, keep, cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

int needle_find_all_compact16_packed_dev(const needle_pattern *cp, const needle_packed_view *v, uint32_t max_per_row, uint64_t *d_offsets,
                                         uint32_t *d_start_end16, uint64_t cap, uint64_t *d_total, int *more, void *stream_) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    int rc = check_packed_dev(p, v);
    if (rc) return rc;
    if (!d_offsets || !d_total || (cap && !d_start_end16)) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (max_per_row == 0 || max_per_row > 4096) return fail(NEEDLE_ERR_INVALID, "max_per_row must be 1 .. 4096");
    if (more) *more = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    const DevProgram *tp = nullptr;
    int n_cus = 0;
    rc = packed_find_all_program(p, (int)v->char_width, &tp, &n_cus);
    if (rc) return rc;
    if (!tp)
        return fail(NEEDLE_ERR_UNSUPPORTED, "needle_find_all_compact16_packed_dev: the pattern has no find-all transducer for these rows (use "
                                            "needle_count_matches_packed_dev + needle_find_all_csr_packed_dev)");
    hipStream_t stream = (hipStream_t)stream_;
    int too_long = 0;
    rc = compact_blocked16(v->n_rows, max_per_row, d_offsets, d_start_end16, cap, d_total, stream, [&](uint32_t *counts, uint32_t *blocks) {
        return packed_find_all_launch(v, tp, n_cus, counts, nullptr, nullptr, nullptr, max_per_row, blocks, false, more, more ? &too_long : nullptr, stream);
    });
    if (rc) return rc;
    if (too_long) return fail(NEEDLE_ERR_UNSUPPORTED, "needle_find_all_compact16_packed_dev: rows of at most 65 535 chars (a longer row's matches were not filed)");
    return NEEDLE_OK;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
extern "C" {

int needle_matches_packed_dev(const needle_pattern *p, const needle_packed_view *v, uint64_t *bm, void *s) {
    return run_packed_dev(p, OP_MATCHES, v, bm, nullptr, nullptr, s);
}
int needle_contained_in_packed_dev(const needle_pattern *p, const needle_packed_view *v, uint64_t *bm, void *s) {
    return run_packed_dev(p, OP_CONTAINED_IN, v, bm, nullptr, nullptr, s);
}
int needle_find_packed_dev(const needle_pattern *p, const needle_packed_view *v, uint64_t *bm, int32_t *st, int32_t *en, void *s) {
    return run_packed_dev(p, OP_FIND, v, bm, st, en, s);
}
int needle_find_next_packed_dev(const needle_pattern *p, const needle_packed_view *v, const int32_t *cur, uint64_t *bm, int32_t *st,
                                int32_t *en, void *s) {
    if (!cur) return fail(NEEDLE_ERR_INVALID, "cursor is NULL");
    return run_packed_dev(p, OP_FIND, v, bm, st, en, s, cur);
}
int needle_find_packed16_packed_dev(const needle_pattern *p, const needle_packed_view *v, uint64_t *bm, uint32_t *start_end16,
                                    int32_t *overflow, void *s) {
    if (!start_end16) return fail(NEEDLE_ERR_INVALID, "start_end16 is NULL");
    return run_packed_dev(p, OP_FIND, v, bm, nullptr, nullptr, s, nullptr, start_end16, false, overflow);
}
int needle_find_packed8_packed_dev(const needle_pattern *p, const needle_packed_view *v, uint64_t *bm, uint16_t *start_len8,
                                   int32_t *overflow, void *s) {
    if (!start_len8) return fail(NEEDLE_ERR_INVALID, "start_len8 is NULL");
    return run_packed_dev(p, OP_FIND, v, bm, nullptr, nullptr, s, nullptr, (uint32_t *)start_len8, true, overflow);
}

int needle_rows_from_packed_dev(const needle_packed_view *v, void *d_rows, uint64_t row_stride, uint32_t *d_lengths,
                                int32_t *d_overflow, void *stream) {
    int rc = check_packed(v);
    if (rc) return rc;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!d_rows || !d_lengths) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    const uint64_t stride_bytes = row_stride * v->char_width;
    if (stride_bytes == 0 || stride_bytes % 16 != 0)
        return fail(NEEDLE_ERR_INVALID, "row_stride * char_width must be a non-zero multiple of 16 bytes");
    if (((uintptr_t)d_rows) % 16 != 0) return fail(NEEDLE_ERR_INVALID, "d_rows must be 16-byte aligned");
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    HIP_TRY(launch_unpack(v->data, v->offsets, v->n_rows, v->char_width, d_rows, stride_bytes, d_lengths, d_overflow,
                          cus, (hipStream_t)stream));
    return NEEDLE_OK;
}

const char *needle_version(void) { return "needle_hip 0.1 (gfx950)"; }
const char *needle_last_error(void) { return g_err.c_str(); }

int needle_trim_scratch(size_t keep_bytes) {
    const hipError_t e = needle::scratch_trim(keep_bytes);
    return e == hipSuccess ? NEEDLE_OK : hip_fail(e, "hipMemPoolTrimTo");
}
int needle_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int needle_compile(const uint16_t *regex, size_t n, int flags, needle_pattern **out) {
    if (!out) return fail(NEEDLE_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!regex && n) return fail(NEEDLE_ERR_INVALID, "regex is NULL"); // Objects.requireNonNull, RegexParser.java:87
    if (flags & ~NEEDLE_ALL_FLAGS) return fail(NEEDLE_ERR_INVALID, "unknown flag bits"); // CompilerOptions.java:9-16
    needle_pattern *p = new needle_pattern();
    std::string err;
    int rc = compile_regex(std::u16string((const char16_t *)regex, n), flags, p->t, err);
    if (rc != NEEDLE_OK) {
        delete p;
        return fail(rc, err);
    }
    if (!validate_tables(p->t, err)) {
        delete p;
        return fail(NEEDLE_ERR_COMPILE, err);
    }
    p->has_regex = true;
    p->regex.assign((const char16_t *)regex, n);
    p->regex_flags = flags;
    *out = p;
    return NEEDLE_OK;
}

static int take_dfa(const needle_dfa_desc &d, int stride, RefDfa &o, std::string &err) {
    if (d.n_states < 1 || d.n_states > 16383) { err = "n_states out of range (1..16383)"; return NEEDLE_ERR_COMPILE; }
    if (!d.accepting) { err = "accepting is NULL"; return NEEDLE_ERR_INVALID; }
    o.n_states = d.n_states;
    o.max_char = d.max_char;
    o.accepting.resize(d.n_states);
    for (int i = 0; i < d.n_states; ++i) o.accepting[i] = d.accepting[i] ? 1 : 0;
    if (d.table) {
        o.table.assign(d.table, d.table + (size_t)d.n_states * stride);
    } else if (d.table_string) {
        if (!decode_table_string(d.table_string, d.n_states, stride, o.table, err)) return NEEDLE_ERR_INVALID;
    } else {
        err = "neither table nor table_string given";
        return NEEDLE_ERR_INVALID;
    }
    return NEEDLE_OK;
}

int needle_pattern_from_tables(const needle_table_desc *desc, needle_pattern **out) {
    if (!out) return fail(NEEDLE_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!desc || !desc->class_map) return fail(NEEDLE_ERR_INVALID, "desc / class_map is NULL");
    if (desc->stride < 1 || desc->stride > 255) return fail(NEEDLE_ERR_INVALID, "stride out of range");
    needle_pattern *p = new needle_pattern();
    p->t.class_map.assign(desc->class_map, desc->class_map + 65536);
    p->t.stride = desc->stride;
    p->t.fixed_len = desc->fixed_len < 0 ? -1 : desc->fixed_len;
    const needle_dfa_desc *ds[4] = {&desc->matches, &desc->contained_in, &desc->forwards, &desc->backwards};
    std::string err;
    for (int w = 0; w < 4; ++w) {
        int rc = take_dfa(*ds[w], desc->stride, p->t.dfa[w], err);
        if (rc) {
            delete p;
            return fail(rc, err);
        }
    }
    if (!validate_tables(p->t, err)) {
        delete p;
        return fail(NEEDLE_ERR_INVALID, err);
    }
    *out = p;
    return NEEDLE_OK;
}

void needle_pattern_destroy(needle_pattern *p) { delete p; }

int needle_pattern_get_info(const needle_pattern *p, needle_pattern_info *o) {
    if (!p || !o) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    memset(o, 0, sizeof(*o));
    o->stride = p->t.stride;
    o->fixed_len = p->t.fixed_len;
    o->min_len = p->t.min_len;
    o->max_len = p->t.max_len;
    for (int w = 0; w < 4; ++w) {
        o->n_states[w] = p->t.dfa[w].n_states;
        o->max_char[w] = p->t.dfa[w].max_char;
        o->kernel_mode[w] = (int)lower(p->t, (Which)w, 1, max_prog_lds(), false).hdr.mode;
    }
    return NEEDLE_OK;
}

int needle_pattern_program_info(const needle_pattern *p, int which, int char_width, int with_backward, needle_program_info *o) {
    if (!p || !o) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    if (which < 0 || which > 2 || (char_width != 1 && char_width != 2)) return fail(NEEDLE_ERR_INVALID, "which / char_width out of range");
    memset(o, 0, sizeof(*o));
    const bool backward = with_backward != 0 && which == W_FORWARDS && p->t.fixed_len < 0;
    Program pr = lower(p->t, (Which)which, char_width, max_prog_lds(), false, backward);
    if (backward && find_lengths_for(pr.hdr.mode)) { // (choose_route, route 5)
        if (const MatchLengths *ml = pattern_ml(p)) {
            Program lp = lower_match_lengths(p->t, *ml, char_width, max_prog_lds(), false);
            if (!lp.blob.empty() && takes_lengths_form(pr.hdr.mode, lp.hdr.mode)) pr = std::move(lp), o->lengths_form = 1;
        }
    }
    o->mode = (int32_t)pr.hdr.mode;
    o->n_states = (int32_t)pr.hdr.n_states;
    o->lds_bytes = (int32_t)pr.hdr.lds_bytes;
    o->blob_bytes = (int32_t)pr.blob.size();
    int waves = 0, chb = 0, in_f = 0;
    if (shape_for_program(pr.hdr, char_width, &waves, &chb, &in_f)) o->waves = waves, o->tile_bytes = chb;
    o->dense_rows = (int32_t)pr.hdr.sp_dense;
    o->records = (int32_t)pr.hdr.sp_records;
    o->chains = (int32_t)pr.hdr.sp_chains;
    if (pr.hdr.mode == MODE_HYBRID) o->hot_rows = (int32_t)(pr.hdr.hot_bytes / (pr.hdr.n_cols * 2u));
    o->window = (int32_t)pr.hdr.win_on;
    if (pr.hdr.win_on) {
        const uint32_t e = pr.hdr.mode == MODE_SPARSE ? 4u : (pr.hdr.mode == MODE_TABLE16 || pr.hdr.mode == MODE_HYBRID) ? 2u : 1u;
        o->window_lo = (int32_t)(pr.hdr.win_lo_e / e);
        o->window_hi = (int32_t)(pr.hdr.win_hi_e / e);
    }
    return NEEDLE_OK;
}

// The n-gram candidate filter (needle_ngram_host.h) of the program containedIn() (which = 1) / find() (which = 2) runs on 8-bit
// rows, as choose_route chooses it: whether there is one, its parameters, why not, and (bitmap != NULL) the bitmap itself.
static int prefilter_info_uncached(const needle_pattern *p, int which, needle_prefilter_info *o, std::vector<uint32_t> *bitmap_out, bool wide,
                                   uint32_t *m1b, uint32_t *m2b) {
    memset(o, 0, sizeof(*o));
    *m1b = *m2b = 0;
    const bool backward = which == W_FORWARDS && p->t.fixed_len < 0;
    Program pr;
    bool usable = which == W_CONTAINED_IN || p->t.fixed_len >= 0;
    if (wide) { // (as run_dev / find_all_one_pass build it; whether a batch takes it also depends on the ordinary UTF-16 program's mode)
        const MatchLengths *ml = backward ? pattern_ml(p) : nullptr;
        if (p->t.class_map.size() == 65536 && (!backward || ml)) pr = lower_filter_wide(p->t, (Which)which, ml), usable = true;
        else memset(&pr.hdr, 0, sizeof(pr.hdr)), memset(&pr.ng.p, 0, sizeof(pr.ng.p)), pr.hdr.mode = MODE_GLOBAL;
    } else
    pr = lower(p->t, (Which)which, 1, max_prog_lds(), false, backward);
    if (!wide && backward && find_lengths_for(pr.hdr.mode)) {
        if (const MatchLengths *ml = pattern_ml(p)) {
            Program lp = lower_match_lengths(p->t, *ml, 1, max_prog_lds(), false);
            if (!lp.blob.empty() && takes_lengths_form(pr.hdr.mode, lp.hdr.mode)) pr = std::move(lp), usable = true;
        }
    }
    if (!wide && (pr.hdr.mode == MODE_HYBRID || pr.hdr.mode == MODE_GLOBAL) && ngram_level() > 0) {
        // an automaton that fits the LDS in no form: the filter program walks its table out of HBM / L2 (lower_filter_hbm)
        const MatchLengths *ml = backward ? pattern_ml(p) : nullptr;
        if (!backward || ml) {
            Program hp = lower_filter_hbm(p->t, (Which)which, ml);
            if (!hp.blob.empty() && hp.hdr.mode == MODE_GLOBAL) pr = std::move(hp), usable = true;
        } else if (prefilter_unbounded_on()) { // no bounded match lengths: the forward search automaton + backward walks (V_FILTER_UNBOUNDED)
            Program hp = lower_filter_hbm(p->t, (Which)which, nullptr, true);
            if (!hp.blob.empty() && hp.hdr.mode == MODE_GLOBAL) pr = std::move(hp), usable = true;
        }
    }
    // (find() of a pattern without bounded match lengths: behind the filter of its ordinary LDS-resident program, starts by backward walks)
    if (!wide && !usable && backward && prefilter_unbounded_on() && pr.hdr.mode != MODE_GLOBAL && pr.hdr.mode != MODE_HYBRID) usable = true;
    const NgramFilter &f = pr.ng;
    o->mode = (int32_t)pr.hdr.mode;
    if (!usable) {
        snprintf(o->why, sizeof(o->why), "find() needs its backward walk for this pattern");
        return NEEDLE_OK;
    }
    o->on = (int32_t)(f.p.on && ngram_lds_bytes(pr.hdr, f.p) ? 1 : 0);
    o->stride = (int32_t)f.p.stride;
    o->warm = (int32_t)f.p.warm;
    o->min_len = (int32_t)f.p.min_len;
    o->n_windows = (int32_t)f.p.n_grams;
    o->bitmap_bytes = (int32_t)f.p.bm_bytes;
    o->m1 = f.p.m1, o->m2 = f.p.m2, o->addr_shift = f.p.addr_shift, o->addr_mask = f.p.addr_mask;
    *m1b = f.p.m1b, *m2b = f.p.m2b;
    o->on2 = (int32_t)(o->on ? f.p.on2 : 0); // (2: two-sided, NgramParams::on2)
    if (o->on2) o->n_windows2 = (int32_t)f.p.n_grams2, o->bitmap2_bytes = (int32_t)f.p.bm2_bytes, o->m3 = f.p.m3, o->addr_mask2 = f.p.addr_mask2;
    snprintf(o->why, sizeof(o->why), "%s", f.p.on ? "" : (f.why.empty() ? (ngram_level() > 0 ? "not a mode the filter is built for" : "NEEDLE_PREFILTER=0") : f.why.c_str()));
    if (f.p.on) {
        *bitmap_out = f.bitmap;
        if (o->on2) bitmap_out->insert(bitmap_out->end(), f.bitmap2.begin(), f.bitmap2.end()); // (the second level's right behind)
    }
    return NEEDLE_OK;
}

// wide: the filter of UTF-16 rows of a pattern on several pages of the BMP (lower_filter_wide).  At most cap_words bitmap words are written.
int needle_pattern_prefilter_info2(const needle_pattern *cp, int which, int wide, needle_prefilter_info2 *o, uint32_t *bitmap, size_t cap_words) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p || !o) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    if (which != W_CONTAINED_IN && which != W_FORWARDS) return fail(NEEDLE_ERR_INVALID, "which must be 1 (contained_in) or 2 (forwards)");
    std::lock_guard<std::mutex> lk(p->pf_mu);
    needle_pattern::PrefilterCache &c = p->pf_cache[(wide ? 4 : 0) + which];
    if (!c.have) {
        const int rc = prefilter_info_uncached(p, which, &c.info, &c.bitmap, wide != 0, &c.m1b, &c.m2b);
        if (rc) return rc;
        c.have = true;
    }
    memset(o, 0, sizeof(*o));
    o->base = c.info;
    o->wide = wide ? 1 : 0;
    o->m1b = c.m1b, o->m2b = c.m2b;
    if (bitmap && c.info.on) memcpy(bitmap, c.bitmap.data(), std::min(cap_words, c.bitmap.size()) * 4);
    return NEEDLE_OK;
}

// (the original contract: the FIRST level's bitmap_bytes / 4 words only -- the second level's come through needle_pattern_prefilter_info2,
// which takes the caller's capacity)
int needle_pattern_prefilter_info(const needle_pattern *cp, int which, needle_prefilter_info *o, uint32_t *bitmap) {
    if (!o) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    needle_prefilter_info2 i2;
    int rc = needle_pattern_prefilter_info2(cp, which, 0, &i2, nullptr, 0);
    if (rc) return rc;
    *o = i2.base;
    if (bitmap && o->on) rc = needle_pattern_prefilter_info2(cp, which, 0, &i2, bitmap, (size_t)o->bitmap_bytes / 4);
    return rc;
}

int needle_pattern_set_prefilter(needle_pattern *p, int mode) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    if (mode < 0 || mode > 2) return fail(NEEDLE_ERR_INVALID, "mode must be NEEDLE_PREFILTER_AUTO (0), _ON (1) or _OFF (2)");
    p->pf_mode.store(mode);
    return NEEDLE_OK;
}

int needle_pattern_utf16_route(const needle_pattern *p, int32_t *page, int32_t *sub) {
    if (!p || !page || !sub) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    const Utf16Route r = utf16_route(p);
    *page = r.page, *sub = r.page >= 0 ? r.sub : 0;
    return NEEDLE_OK;
}

// What the flood watch of this pattern's filter program(s) for `which` on the CURRENT device knows (no device needed to ask; all zero
// before the first scan).  Several programs may carry a filter (plain / lengths / HBM-table forms): the one that ran last is reported.
int needle_pattern_prefilter_state(const needle_pattern *cp, int which, needle_prefilter_state *o) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p || !o) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    if (which != W_CONTAINED_IN && which != W_FORWARDS) return fail(NEEDLE_ERR_INVALID, "which must be 1 (contained_in) or 2 (forwards)");
    memset(o, 0, sizeof(*o));
    o->mode = p->pf_mode.load();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return NEEDLE_OK; // (no device: nothing has run)
    std::lock_guard<std::mutex> lk(p->mu);
    uint64_t best = 0;
    for (auto &kv : p->cache) {
        if (std::get<0>(kv.first) != dev || std::get<1>(kv.first) != which || !kv.second.d_ng) continue;
        const DevProgram &dp = kv.second;
        std::lock_guard<std::mutex> lk2(dp.ng_mu);
        o->has_filter = 1;
        const uint64_t used = dp.ng_launches + dp.ng_suspended_calls;
        if (used < best) continue;
        best = used;
        o->suspended_calls_left = dp.ng_suspend;
        o->backoff = dp.ng_backoff;
        o->last_candidates_per_kib = dp.ng_last_rate;
        o->filter_launches = dp.ng_launches;
        o->suspended_calls = dp.ng_suspended_calls;
    }
    return NEEDLE_OK;
}

// The find-all "lengths" automaton (needle_lower.h), for inspection and CPU-side tests: 1 in *available when the pattern
// allows it.  table: n_states * (stride + 1) int16 (reference layout + one column for chars beyond *max_char, -1 = dead);
// accepting, pend: n_states bytes each.
int needle_pattern_match_lengths(const needle_pattern *cp, int32_t *available, int32_t *n_states, int32_t *n_dead, int32_t *max_char,
                                 int16_t *table, uint8_t *accepting, uint8_t *pend) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p || !available) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    *available = pattern_ml(p) ? 1 : 0;
    if (!*available) return NEEDLE_OK;
    if (n_states) *n_states = p->ml.dfa.n_states;
    if (n_dead) *n_dead = p->ml.n_dead;
    if (max_char) *max_char = p->ml.dfa.max_char;
    if (table) {
        const int N = p->t.stride;
        for (int s = 0; s < p->ml.dfa.n_states; ++s) {
            memcpy(table + (size_t)s * (N + 1), &p->ml.dfa.table[(size_t)s * N], (size_t)N * 2);
            table[(size_t)s * (N + 1) + N] = p->ml.over[s];
        }
    }
    if (accepting) memcpy(accepting, p->ml.dfa.accepting.data(), p->ml.dfa.accepting.size());
    if (pend) memcpy(pend, p->ml.pend.data(), p->ml.pend.size());
    return NEEDLE_OK;
}

// The find-all transducer's device program (needle_lower.h), for inspection and CPU-side tests that walk the blob the way the kernel
// does.  info[0..11] = n_states, n_cols, pad_col, start, win_on, win_lo_e, win_hi_e, off_table, ft_codes_off, lds_bytes, n_pages, 0.
int needle_pattern_find_all_transducer(const needle_pattern *cp, int char_width, int32_t *available, int32_t *info, void *blob, size_t cap,
                                       size_t *needed) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p || !available || (char_width != 1 && char_width != 2)) return fail(NEEDLE_ERR_INVALID, "bad argument");
    *available = 0;
    const MatchLengths *ml = pattern_ml(p);
    Program pr;
    memset(&pr.hdr, 0, sizeof(pr.hdr));
    if (ml) pr = lower_find_all_transducer(p->t, *ml, char_width, max_prog_lds());
    // (no transducer on the lengths automaton: the RUN transducer, if the pattern is one of runs -- info[11] = 2)
    if ((pr.blob.empty() || !pr.hdr.ft_on) && p->t.fixed_len < 0) pr = lower_find_all_runs(p->t, char_width, max_prog_lds());
    if (pr.blob.empty() || !packed_find_all_takes(pr.hdr, char_width)) return NEEDLE_OK; // (ft_on, and a packed find-all shape fits)
    *available = 1;
    if (info) {
        const ProgHeader &h = pr.hdr;
        const uint32_t v[12] = {h.n_states, h.n_cols, h.pad_col, h.start, h.win_on, h.win_lo_e, h.win_hi_e, h.off_table, h.ft_codes_off, h.lds_bytes, h.n_pages, h.ft_on};
        for (int i = 0; i < 12; ++i) info[i] = (int32_t)v[i];
    }
    if (needed) *needed = pr.blob.size();
    if (blob && cap >= pr.blob.size()) memcpy(blob, pr.blob.data(), pr.blob.size());
    return NEEDLE_OK;
}

// Which route needle_count_matches_packed_dev (count_only) / needle_find_all_csr_packed_dev take for this pattern on rows of char_width:
// 0 neither the transducer nor the per-lane kernel (the filter kernel where needle_pattern_find_all_packed_filter says so, else
// conversion), 1 the transducer kernel, 2 the per-lane kernel.  Answers without a device: the programs are lowered on the host, the
// questions are the entries' own (packed_find_all_takes by way of needle_pattern_find_all_transducer, find_all_lane_choice,
// packed_find_all_lane_takes).
int needle_pattern_find_all_packed_route(const needle_pattern *cp, int char_width, int count_only, int32_t *route) {
    if (!cp || !route || (char_width != 1 && char_width != 2) || (count_only != 0 && count_only != 1)) return fail(NEEDLE_ERR_INVALID, "bad argument");
    *route = 0;
    int32_t transducer = 0;
    int rc = needle_pattern_find_all_transducer(cp, char_width, &transducer, nullptr, nullptr, 0, nullptr);
    if (rc) return rc;
    if (transducer) {
        *route = 1;
        return NEEDLE_OK;
    }
    Program pr; // the one program the choice settles on (asked for last)
    LaneChoice c;
    rc = find_all_lane_choice(cp, count_only != 0, [&](Variant v, const ProgHeader **h) {
        *h = nullptr;
        if (v == V_FA_LENGTHS || v == V_LENGTHS) { // (as get_program lowers them)
            const MatchLengths *ml = pattern_ml(cp);
            if (!ml) return (int)NEEDLE_OK;
            pr = lower_match_lengths(cp->t, *ml, char_width, max_prog_lds(), v == V_FA_LENGTHS);
        } else {
            pr = lower(cp->t, W_FORWARDS, char_width, max_prog_lds(), false, v == V_FA_BACKMAPS, true);
        }
        if (!pr.blob.empty()) *h = &pr.hdr;
        return (int)NEEDLE_OK;
    }, &c);
    if (rc) return rc;
    if (packed_find_all_lane_takes(*c.hdr, char_width)) *route = 2;
    return NEEDLE_OK;
}

// Whether the packed find-all entries take the FILTER kernel for this pattern on rows of char_width (needle_ngram_packed.h): neither the
// transducer nor the per-lane kernel takes it (needle_pattern_find_all_packed_route says 0) and the filter's find-all form has a program
// for it.  Answers without a device, with the routing's own predicates (packed_find_all_filter_on, find_all_filter_choice on host-side
// lowerings, packed_find_all_filter_takes); the flood watch and the needle_pattern_set_prefilter pin are runtime state and left aside.
int needle_pattern_find_all_packed_filter(const needle_pattern *cp, int char_width, int count_only, int32_t *available) {
    if (!cp || !available || (char_width != 1 && char_width != 2) || (count_only != 0 && count_only != 1)) return fail(NEEDLE_ERR_INVALID, "bad argument");
    *available = 0;
    int32_t route = 0;
    int rc = needle_pattern_find_all_packed_route(cp, char_width, count_only, &route);
    if (rc || route != 0 || !packed_find_all_filter_on()) return rc;
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    std::vector<std::unique_ptr<Program>> lowered; // (the choice holds pointers into it)
    FilterChoice fc;
    rc = find_all_filter_choice(cp, char_width, [&](int cw_key, Variant v, const Program **pr) {
        *pr = nullptr;
        const bool wants_ml = variant_wants_ml(cp, W_FORWARDS, v);
        const MatchLengths *ml = wants_ml ? pattern_ml(cp) : nullptr; // (before p->mu: see ml_mu)
        std::lock_guard<std::mutex> lk(p->mu);
        const RefTables *tt = tables_for_page(p, cw_key >> 8, &ml);
        std::unique_ptr<Program> out(new Program());
        if (lower_variant(*tt, W_FORWARDS, cw_key & 0xFF, v, wants_ml, ml, out.get())) {
            *pr = out.get();
            lowered.push_back(std::move(out));
        }
        return (int)NEEDLE_OK;
    }, &fc);
    if (rc) return rc;
    if (fc.prog && packed_find_all_filter_takes(cp, *fc.prog)) *available = 1;
    return NEEDLE_OK;
}

int needle_pattern_get_class_map(const needle_pattern *p, uint8_t *cm) {
    if (!p || !cm) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    memcpy(cm, p->t.class_map.data(), 65536);
    return NEEDLE_OK;
}

int needle_pattern_get_table(const needle_pattern *p, int which, int16_t *table, uint8_t *accepting) {
    if (!p || which < 0 || which > 3) return fail(NEEDLE_ERR_INVALID, "bad argument");
    const RefDfa &d = p->t.dfa[which];
    if (table) memcpy(table, d.table.data(), d.table.size() * 2);
    if (accepting) memcpy(accepting, d.accepting.data(), d.accepting.size());
    return NEEDLE_OK;
}

// ---- precompiled-pattern blob ("NDLT" v1)
static void put_i32(std::vector<uint8_t> &b, int32_t v) {
    for (int i = 0; i < 4; ++i) b.push_back((uint8_t)((uint32_t)v >> (8 * i)));
}
static bool get_i32(const uint8_t *&p, const uint8_t *end, int32_t &v) {
    if (end - p < 4) return false;
    v = (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
    p += 4;
    return true;
}

int needle_pattern_serialize(const needle_pattern *p, void *buf, size_t cap, size_t *needed) {
    if (!p || !needed) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    std::vector<uint8_t> b;
    const char magic[4] = {'N', 'D', 'L', 'T'};
    b.insert(b.end(), magic, magic + 4);
    put_i32(b, 1);
    put_i32(b, p->t.stride);
    put_i32(b, p->t.fixed_len);
    put_i32(b, p->t.min_len);
    put_i32(b, p->t.max_len);
    for (int w = 0; w < 4; ++w) {
        put_i32(b, p->t.dfa[w].n_states);
        put_i32(b, p->t.dfa[w].max_char);
    }
    b.insert(b.end(), p->t.class_map.begin(), p->t.class_map.end());
    for (int w = 0; w < 4; ++w) {
        for (int16_t v : p->t.dfa[w].table) {
            b.push_back((uint8_t)((uint16_t)v & 255));
            b.push_back((uint8_t)((uint16_t)v >> 8));
        }
        b.insert(b.end(), p->t.dfa[w].accepting.begin(), p->t.dfa[w].accepting.end());
    }
    *needed = b.size();
    if (cap == 0) return NEEDLE_OK;
    if (!buf || cap < b.size()) return fail(NEEDLE_ERR_INVALID, "buffer too small");
    memcpy(buf, b.data(), b.size());
    return NEEDLE_OK;
}

int needle_pattern_deserialize(const void *buf, size_t n, needle_pattern **out) {
    if (!out) return fail(NEEDLE_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!buf) return fail(NEEDLE_ERR_INVALID, "buf is NULL");
    const uint8_t *q = (const uint8_t *)buf, *end = q + n;
    if (n < 8 || memcmp(q, "NDLT", 4) != 0) return fail(NEEDLE_ERR_INVALID, "not a needle table blob");
    q += 4;
    int32_t ver = 0;
    needle_pattern *p = new needle_pattern();
    bool ok = get_i32(q, end, ver) && ver == 1 && get_i32(q, end, p->t.stride) && get_i32(q, end, p->t.fixed_len) &&
              get_i32(q, end, p->t.min_len) && get_i32(q, end, p->t.max_len);
    for (int w = 0; ok && w < 4; ++w) ok = get_i32(q, end, p->t.dfa[w].n_states) && get_i32(q, end, p->t.dfa[w].max_char);
    ok = ok && p->t.stride >= 1 && p->t.stride <= 255 && (size_t)(end - q) >= 65536;
    if (ok) {
        p->t.class_map.assign(q, q + 65536);
        q += 65536;
    }
    for (int w = 0; ok && w < 4; ++w) {
        RefDfa &d = p->t.dfa[w];
        ok = d.n_states >= 1 && d.n_states <= 16383;
        const size_t cells = ok ? (size_t)d.n_states * p->t.stride : 0;
        ok = ok && (size_t)(end - q) >= cells * 2 + (size_t)d.n_states;
        if (!ok) break;
        d.table.resize(cells);
        for (size_t i = 0; i < cells; ++i) d.table[i] = (int16_t)((uint16_t)q[2 * i] | ((uint16_t)q[2 * i + 1] << 8));
        q += cells * 2;
        d.accepting.assign(q, q + d.n_states);
        q += d.n_states;
    }
    std::string err = "truncated or malformed table blob";
    if (!ok || q != end || !validate_tables(p->t, err)) {
        delete p;
        return fail(NEEDLE_ERR_INVALID, err);
    }
    *out = p;
    return NEEDLE_OK;
}

int needle_matches_dev(const needle_pattern *p, const needle_batch_view *v, uint64_t *bm, void *s) {
    return run_dev(p, OP_MATCHES, v, bm, nullptr, nullptr, s);
}
int needle_contained_in_dev(const needle_pattern *p, const needle_batch_view *v, uint64_t *bm, void *s) {
    return run_dev(p, OP_CONTAINED_IN, v, bm, nullptr, nullptr, s);
}
int needle_find_dev(const needle_pattern *p, const needle_batch_view *v, uint64_t *bm, int32_t *st, int32_t *en, void *s) {
    return run_dev(p, OP_FIND, v, bm, st, en, s);
}
// find() with a row's start / end as one dword (start | end << 16, 0xFFFFFFFF = no match), stored by the scan kernel itself:
// 4 result bytes per row instead of 8, no separate pack pass.  Rows of at most 65 534 chars.
int needle_find_packed16_dev(const needle_pattern *p, const needle_batch_view *v, uint64_t *bm, uint32_t *start_end16, void *s) {
    if (v && v->n_rows && !start_end16) return fail(NEEDLE_ERR_INVALID, "start_end16 is NULL");
    if (v && !offsets16_ok(v, 65534u)) return fail(NEEDLE_ERR_UNSUPPORTED, "16-bit offsets: rows of at most 65 534 chars (use needle_find_dev)");
    return run_dev(p, OP_FIND, v, bm, nullptr, nullptr, s, nullptr, nullptr, false, start_end16);
}
// find() with a row's result as ONE uint16 -- start | (end - start) << 8, 0xFFFF = no match, 0xFFFE = the match (0, 256) -- stored by the
// kernels themselves: 2 result bytes per row.  Rows of at most 256 chars.
int needle_find_packed8_dev(const needle_pattern *p, const needle_batch_view *v, uint64_t *bm, uint16_t *start_len8, void *s) {
    if (v && v->n_rows && !start_len8) return fail(NEEDLE_ERR_INVALID, "start_len8 is NULL");
    if (v && (v->lengths ? v->row_stride : v->row_len) > 256u) return fail(NEEDLE_ERR_UNSUPPORTED, "8-bit start / length: rows of at most 256 chars (use needle_find_packed16_dev)");
    return run_dev(p, OP_FIND, v, bm, nullptr, nullptr, s, nullptr, nullptr, false, (uint32_t *)start_len8, true);
}
int needle_find_next_dev(const needle_pattern *p, const needle_batch_view *v, const int32_t *cur, uint64_t *bm, int32_t *st,
                         int32_t *en, void *s) {
    if (!cur) return fail(NEEDLE_ERR_INVALID, "cursor is NULL");
    return run_dev(p, OP_FIND, v, bm, st, en, s, cur);
}
// The round-per-match form: one needle_find_next pass over the batch per round, one stream synchronisation per round.
// Rows of 64 MiB and more (stripe paths only) take it; NEEDLE_FIND_ALL_ROUNDS=1 forces it (tests cross-check the two).
static int find_all_rounds(const needle_pattern *p, const needle_batch_view *v, uint32_t slots, uint32_t *d_counts, int32_t *d_start,
                           int32_t *d_end, int *more, hipStream_t stream) {
    const size_t n = (size_t)v->n_rows, words = (n + 63) / 64;
    int dev = 0, cus = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    uint8_t *tmp = nullptr; // cursor | start | end (int32 each) | bitmap | any-hit flag
    const size_t o_cur = 0, o_s = n * 4, o_e = 2 * n * 4, o_bm = (3 * n * 4 + 15) & ~(size_t)15, o_flag = o_bm + words * 8;
    HIP_TRY(scratch_malloc((void **)&tmp, o_flag + 16, stream));
    auto done = [&](int code) {
        (void)scratch_free(tmp, stream);
        return code;
    };
    if (hipMemsetAsync(tmp + o_cur, 0, n * 4, stream) != hipSuccess) return done(fail(NEEDLE_ERR_DEVICE, "hipMemsetAsync"));
    for (uint32_t k = 0;; ++k) {
        if (hipMemsetAsync(tmp + o_flag, 0, 4, stream) != hipSuccess) return done(fail(NEEDLE_ERR_DEVICE, "hipMemsetAsync"));
        int rc = run_dev(p, OP_FIND, v, (uint64_t *)(tmp + o_bm), (int32_t *)(tmp + o_s), (int32_t *)(tmp + o_e), stream,
                         (const int32_t *)(tmp + o_cur));
        if (rc) return done(rc);
        hipError_t e = launch_find_all_collect(n, slots, k, (const int32_t *)(tmp + o_s), (const int32_t *)(tmp + o_e),
                                               (int32_t *)(tmp + o_cur), d_counts, d_start, d_end, (int32_t *)(tmp + o_flag), cus, stream);
        if (e != hipSuccess) return done(hip_fail(e, "find_all_collect"));
        int32_t any = 0;
        e = hipMemcpyAsync(&any, tmp + o_flag, 4, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return done(hip_fail(e, "find_all round"));
        if (!any) break;          // round k found nothing anywhere: every row is exhausted
        if (k >= slots) {         // a match beyond the last slot exists
            if (more) *more = 1;
            break;
        }
    }
    return done(NEEDLE_OK);
}

// One pass over the batch: every row is fetched once, each lane restarts its search where its last match ended
// (needle_find_all.hip).  Dense slots (offsets == nullptr), compact filing at caller-computed offsets, or counting only.
// The program is chosen by find-all's own rules (not choose_route's: other programs, other switches); the pieces are the shared ones.
static int find_all_one_pass(needle_pattern *p, const needle_batch_view *v, uint32_t slots, uint32_t *d_counts, int32_t *d_start,
                             int32_t *d_end, const uint64_t *d_offsets, bool count_only, int *more, hipStream_t stream,
                             uint32_t *d_packed = nullptr, uint32_t kshift = 0) {
    const int cw = (int)v->char_width;
    const uint64_t stride_bytes = v->row_stride * v->char_width;
    if (stride_bytes >= (1ull << 26)) return fail(NEEDLE_ERR_UNSUPPORTED, "rows of 64 MiB or more: only needle_find_all_dev (round per match) takes them");
    int rc = NEEDLE_OK;
    static const bool lengths_on = find_all_lengths_level() != 0;
    // the find-all outputs, common to the three kernels below (s: the rows and the program, filled by each)
    FindAllArgs fa;
    memset(&fa, 0, sizeof(fa));
    fa.slots = slots;
    fa.kshift = kshift;
    fa.offsets = d_offsets;
    fa.count_only = count_only ? 1u : 0u;
    fa.counts = d_counts;
    fa.starts = d_start;
    fa.ends = d_end;
    fa.packed = d_packed;
    // Dictionaries whose find() runs behind the n-gram candidate filter (needle_ngram.hip): their find-all does too -- the filter
    // kernel's find-all form files every verified candidate and each row sorts its own out against its moving cursor (dense slots,
    // the counting pass and the compact filing alike).  The program: find_all_filter_choice.
    if (count_only || d_offsets || slots) {
        FilterChoice fc;
        const DevProgram *sp = nullptr;
        int cus = 0;
        if ((rc = find_all_filter_program(p, cw, &fc, &sp, &cus))) return rc;
        if (sp && ngram_find_all_lds_bytes(sp->prog.hdr, sp->prog.ng.p)) {
            // (UTF-16 rows: the stride in CHARS -- launch_ngram_find_all with char_width 2)
            const ScanArgs a = scan_args(v, v->row_stride, sp, nullptr, p->t.fixed_len, ScanOut());
            if (ngram_shape_ok(a) && ngram_watch_allows(p, sp))
                return with_more_flag(stream, more, "find_all (filter kernel)", [&](int32_t *d_more) {
                    hipError_t e = launch_ngram_find_all(a, sp->prog.ng.p, sp->d_ng, sp->d_ng_stats, slots, d_counts, d_start, d_end, d_packed, d_more, d_offsets,
                                                         count_only, cus, stream, cw, fc.page, fc.sub, kshift);
                    if (e == hipSuccess) e = ngram_watch_after_launch(sp, stream);
                    return e;
                });
        }
    }
    // Patterns with a find-all transducer (needle_lower.h: bounded match lengths, no match inside a longer live one) are walked in
    // LOCK-STEP: one table lookup per char, every lane at the same char, the restarts folded into the automaton (needle_find_all_ls.hip).
    // NEEDLE_FIND_ALL_LOCKSTEP=0: off (A/B, tests: the per-lane one-pass kernel below).
    static const bool lockstep_on = (getenv("NEEDLE_FIND_ALL_LOCKSTEP") ? atoi(getenv("NEEDLE_FIND_ALL_LOCKSTEP")) : 1) != 0;
    fa.s.stride_bytes = stride_bytes; // (what the launcher's own check looks at: one definition of "the lock-step kernel takes this shape")
    if (lockstep_on && find_all_lockstep_shape_ok(fa)) {
        const DevProgram *tp = nullptr;
        int cus = 0;
        // NEEDLE_FIND_ALL_LENGTHS=0 / NEEDLE_FIND_ALL_RUNS=0: without the lengths / the RUN transducer (A/B, tests)
        static const bool runs_on = (getenv("NEEDLE_FIND_ALL_RUNS") ? atoi(getenv("NEEDLE_FIND_ALL_RUNS")) : 1) != 0;
        if ((rc = find_all_transducer_program(p, cw, lengths_on, runs_on, &tp, &cus))) return rc;
        if (tp) {
            fa.s = scan_args(v, stride_bytes, tp, nullptr, -1, ScanOut());
            return with_more_flag(stream, more, "find_all (lock-step kernel)", [&](int32_t *d_more) {
                fa.more = d_more;
                return launch_find_all_lockstep(cw, fa, cus, stream);
            });
        }
    }
    LaneProgram lp;
    if ((rc = find_all_lane_program(p, cw, count_only, &lp))) return rc;
    fa.s = scan_args(v, stride_bytes, lp.fp, lp.bp, p->t.fixed_len, ScanOut());
    fa.lmode = lp.lmode ? 1u : 0u;
    fa.defer = lp.defer;
    const int n_cus = lp.n_cus;
    return with_more_flag(stream, more, "find_all", [&](int32_t *d_more) {
        fa.more = d_more;
        return launch_find_all(cw, fa, n_cus, stream);
    });
}

int needle_find_all_dev(const needle_pattern *cp, const needle_batch_view *v, uint32_t slots, uint32_t *d_counts, int32_t *d_start,
                        int32_t *d_end, int *more, void *stream_) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_view(v);
    if (rc) return rc;
    if (more) *more = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!d_counts || (slots && (!d_start || !d_end))) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    hipStream_t stream = (hipStream_t)stream_;
    if (find_all_rounds_forced() || v->row_stride * v->char_width >= (1ull << 26)) return find_all_rounds(p, v, slots, d_counts, d_start, d_end, more, stream);
    return find_all_one_pass(p, v, slots, d_counts, d_start, d_end, nullptr, false, more, stream);
}

// needle_find_all_dev with each match as ONE dword (start | end << 16): half the result bytes, one store per match.
int needle_find_all_packed16_dev(const needle_pattern *cp, const needle_batch_view *v, uint32_t slots, uint32_t *d_counts,
                                 uint32_t *d_start_end16, int *more, void *stream_) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_view(v);
    if (rc) return rc;
    if (more) *more = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!d_counts || (slots && !d_start_end16)) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (!offsets16_ok(v, 65535u)) return fail(NEEDLE_ERR_UNSUPPORTED, "16-bit start / end: rows of at most 65535 chars");
    return find_all_one_pass(p, v, slots, d_counts, nullptr, nullptr, nullptr, false, more, (hipStream_t)stream_, d_start_end16);
}

// needle_find_all_packed16_dev with GROUP-BLOCKED slots: match k of row r at d_blocks[((r >> 6) * slots + k) * 64 + (r & 63)].
int needle_find_all_blocked16_dev(const needle_pattern *cp, const needle_batch_view *v, uint32_t slots, uint32_t *d_counts,
                                  uint32_t *d_blocks, int *more, void *stream_) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_view(v);
    if (rc) return rc;
    if (more) *more = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!d_counts || (slots && !d_blocks)) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (!offsets16_ok(v, 65535u)) return fail(NEEDLE_ERR_UNSUPPORTED, "16-bit start / end: rows of at most 65535 chars");
    return find_all_one_pass(p, v, slots, d_counts, nullptr, nullptr, nullptr, false, more, (hipStream_t)stream_, d_blocks, 6u);
}

int needle_count_matches_dev(const needle_pattern *cp, const needle_batch_view *v, uint32_t *d_counts, void *stream_) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_view(v);
    if (rc) return rc;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!d_counts) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    return find_all_one_pass(p, v, 0, d_counts, nullptr, nullptr, nullptr, true, nullptr, (hipStream_t)stream_);
}

int needle_find_all_csr_dev(const needle_pattern *cp, const needle_batch_view *v, const uint64_t *d_offsets, int32_t *d_start, int32_t *d_end,
                            int *more, void *stream_) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_view(v);
    if (rc) return rc;
    if (more) *more = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!d_offsets || !d_start || !d_end) return fail(NEEDLE_ERR_INVALID, "offsets / output buffer is NULL");
    return find_all_one_pass(p, v, 0, nullptr, d_start, d_end, d_offsets, false, more, (hipStream_t)stream_);
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Pattern sets: up to 32 patterns in one pass over a packed batch (needle_set.h: the products and their groups; needle_packed_set.h: the kernel)
// ------------------------------------------------------------------------------------------------
struct needle_pattern_set {
    std::vector<RefTables> members; // copies: the patterns may be destroyed
    SetPlan plan[2][2];             // [op][char_width - 1], built at creation (host only)
    std::string refused[2][2];      // non-empty: why this plan could not be built (UTF-16 plans only: a refused 8-bit plan fails the creation)
    std::mutex mu;
    std::map<std::tuple<int, int, int, int>, uint8_t *> resident; // (device, op, char_width, group) -> the group's program in that device's HBM
    std::map<int, int> cus;                                       // device -> CU count
    ~needle_pattern_set() {
        for (auto &kv : resident)
            if (kv.second) (void)hipFree(kv.second);
    }
};

static const SetPlan *set_plan(const needle_pattern_set *s, int op, int char_width) {
    if (!s || (op != OP_MATCHES && op != OP_CONTAINED_IN) || (char_width != 1 && char_width != 2)) return nullptr;
    return &s->plan[op][char_width - 1];
}
// NEEDLE_ERR_UNSUPPORTED where the set has no plan for this op and char width (arguments as set_plan accepts them).
int needle::set_plan_usable(const needle_pattern_set *s, int op, int char_width) {
    const std::string &why = s->refused[op][char_width - 1];
    return why.empty() ? NEEDLE_OK : fail(NEEDLE_ERR_UNSUPPORTED, why);
}
uint32_t needle::set_pattern_count(const needle_pattern_set *s) { return (uint32_t)s->members.size(); }

// One group's program on the current device, built on first use and cached in the set (as get_program does for patterns).
static int set_program(needle_pattern_set *s, int op, int cw, int group, const uint8_t **d_blob, int *n_cus) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(s->mu);
    if (!s->cus.count(dev)) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        s->cus[dev] = prop.multiProcessorCount;
    }
    *n_cus = s->cus[dev];
    const auto key = std::make_tuple(dev, op, cw, group);
    auto it = s->resident.find(key);
    if (it == s->resident.end()) {
        const Program &pr = s->plan[op][cw - 1].groups[(size_t)group].prog;
        uint8_t *d = nullptr;
        HIP_TRY(hipMalloc((void **)&d, pr.blob.size()));
        if (hipError_t ce = hipMemcpy(d, pr.blob.data(), pr.blob.size(), hipMemcpyHostToDevice); ce != hipSuccess) {
            (void)hipFree(d);
            return hip_fail(ce, "hipMemcpy(pattern set program)");
        }
        it = s->resident.emplace(key, d).first;
    }
    *d_blob = it->second;
    return NEEDLE_OK;
}

// One launch per group on the caller's stream: group 0 stores the masks, later groups read-modify-write them.
static int run_set_packed_dev(const needle_pattern_set *cs, int op, const needle_packed_view *v, uint32_t *d_masks, void *stream_) {
    needle_pattern_set *s = const_cast<needle_pattern_set *>(cs);
    if (!s) return fail(NEEDLE_ERR_INVALID, "pattern set is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (!d_masks) return fail(NEEDLE_ERR_INVALID, "masks is NULL");
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    if (v->n_rows == 0) return NEEDLE_OK;
    const int cw = (int)v->char_width;
    if ((rc = set_plan_usable(s, op, cw))) return rc;
    const SetPlan &plan = s->plan[op][cw - 1];
    for (size_t g = 0; g < plan.groups.size(); ++g) {
        const SetGroup &grp = plan.groups[g];
        const uint8_t *d_blob = nullptr;
        int n_cus = 0;
        if ((rc = set_program(s, op, cw, (int)g, &d_blob, &n_cus))) return rc;
        PackedSetArgs a;
        memset(&a, 0, sizeof(a));
        a.p.s.rows = (const uint8_t *)v->data;
        a.p.s.n_rows = v->n_rows;
        a.p.s.prog = d_blob;
        a.p.s.hdr = grp.prog.hdr;
        a.p.s.fixed_len = -1;
        a.p.offsets = v->offsets;
        a.masks = d_masks;
        a.group_mask = (grp.count >= 32 ? 0xFFFFFFFFu : ((1u << grp.count) - 1u)) << grp.first;
        a.store = g == 0 ? 1u : 0u;
        HIP_TRY(launch_packed_set(op, cw, a, n_cus, (hipStream_t)stream_));
    }
    return NEEDLE_OK;
}

extern "C" {

int needle_pattern_set_create(const needle_pattern *const *patterns, int n_patterns, needle_pattern_set **out) {
    if (!out) return fail(NEEDLE_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (!patterns) return fail(NEEDLE_ERR_INVALID, "patterns is NULL");
    if (n_patterns < 1 || n_patterns > NEEDLE_SET_MAX_PATTERNS) return fail(NEEDLE_ERR_INVALID, "a pattern set holds 1 .. 32 patterns");
    std::unique_ptr<needle_pattern_set> s(new needle_pattern_set);
    for (int i = 0; i < n_patterns; ++i) {
        if (!patterns[i]) return fail(NEEDLE_ERR_INVALID, "pattern " + std::to_string(i) + " of the set is NULL");
        s->members.push_back(patterns[i]->t);
    }
    for (int op = 0; op < 2; ++op)
        for (int cw = 1; cw <= 2; ++cw) {
            int bad = -1;
            if (build_set_plan(s->members, op, cw, max_prog_lds(), &s->plan[op][cw - 1], &bad)) continue;
            const std::string why = "pattern " + std::to_string(bad) + " of the set does not fit the LDS as a plain table (" +
                                    (op == OP_MATCHES ? "matches" : "containedIn") + ", char_width " + std::to_string(cw) +
                                    "): run it alone, behind the n-gram filter";
            // The UTF-16 column maps hold less than the 8-bit one (columns x element size <= 255): a member they refuse alone must not
            // keep a caller of 8-bit rows from the set -- that plan is refused where it is asked for (info, tables, scans of UTF-16 rows).
            if (cw == 1) return fail(NEEDLE_ERR_UNSUPPORTED, why);
            s->refused[op][cw - 1] = why;
        }
    *out = s.release();
    return NEEDLE_OK;
}

void needle_pattern_set_destroy(needle_pattern_set *s) { delete s; }

int needle_pattern_set_info(const needle_pattern_set *s, int op, int char_width, needle_set_info *o) {
    const SetPlan *plan = set_plan(s, op, char_width);
    if (!plan || !o) return fail(NEEDLE_ERR_INVALID, "pattern_set_info: bad argument");
    if (int rc = set_plan_usable(s, op, char_width)) return rc;
    memset(o, 0, sizeof(*o));
    o->n_patterns = (int32_t)s->members.size();
    o->n_groups = (int32_t)plan->groups.size();
    for (size_t g = 0; g < plan->groups.size(); ++g) {
        const SetGroup &grp = plan->groups[g];
        o->first_pattern[g] = grp.first;
        o->pattern_count[g] = grp.count;
        o->n_states[g] = grp.prod.n_states;
        o->n_columns[g] = grp.prod.n_classes + 2;
        o->kernel_mode[g] = (int32_t)grp.prog.hdr.mode;
        o->lds_bytes[g] = (int32_t)grp.prog.hdr.lds_bytes;
    }
    return NEEDLE_OK;
}

int needle_pattern_set_get_tables(const needle_pattern_set *s, int op, int char_width, int group, uint8_t *class_map, int32_t *n_classes,
                                  int32_t *n_states, int32_t *start, int32_t *table, size_t table_cap, uint32_t *masks, size_t masks_cap) {
    const SetPlan *plan = set_plan(s, op, char_width);
    if (!plan) return fail(NEEDLE_ERR_INVALID, "pattern_set_get_tables: bad argument");
    if (int rc = set_plan_usable(s, op, char_width)) return rc;
    if (group < 0 || (size_t)group >= plan->groups.size()) return fail(NEEDLE_ERR_INVALID, "pattern_set_get_tables: bad argument");
    const SetProduct &sp = plan->groups[(size_t)group].prod;
    if (n_classes) *n_classes = sp.n_classes;
    if (n_states) *n_states = sp.n_states;
    if (start) *start = sp.start;
    if (class_map) memcpy(class_map, sp.class_map.data(), 65536);
    if (table) {
        if (table_cap < sp.table.size()) return fail(NEEDLE_ERR_INVALID, "pattern_set_get_tables: table buffer too small");
        memcpy(table, sp.table.data(), sp.table.size() * 4);
    }
    if (masks) {
        if (masks_cap < sp.mask.size()) return fail(NEEDLE_ERR_INVALID, "pattern_set_get_tables: masks buffer too small");
        memcpy(masks, sp.mask.data(), sp.mask.size() * 4);
    }
    return NEEDLE_OK;
}

int needle_set_matches_packed_dev(const needle_pattern_set *s, const needle_packed_view *v, uint32_t *d_masks, void *stream) {
    return run_set_packed_dev(s, OP_MATCHES, v, d_masks, stream);
}
int needle_set_contained_in_packed_dev(const needle_pattern_set *s, const needle_packed_view *v, uint32_t *d_masks, void *stream) {
    return run_set_packed_dev(s, OP_CONTAINED_IN, v, d_masks, stream);
}

// Which members match each span of a CSR span list (needle_set_spans.h): a pure function of (text, list, set).  The checks and the
// group loop of run_set_packed_dev: one launch per group on the caller's stream, group 0 stores, later groups OR.
int needle_set_matches_spans_packed_dev(const needle_pattern_set *cs, const needle_packed_view *v, const uint64_t *d_span_offsets,
                                        const int32_t *d_start, const int32_t *d_end, uint32_t *d_masks, void *stream_) {
    needle_pattern_set *s = const_cast<needle_pattern_set *>(cs);
    if (!s) return fail(NEEDLE_ERR_INVALID, "pattern set is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (!d_span_offsets) return fail(NEEDLE_ERR_INVALID, "span offsets is NULL");
    if (!d_masks) return fail(NEEDLE_ERR_INVALID, "masks is NULL");
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    if (v->n_rows == 0) return NEEDLE_OK;
    const int cw = (int)v->char_width;
    if ((rc = set_plan_usable(s, OP_MATCHES, cw))) return rc;
    const SetPlan &plan = s->plan[OP_MATCHES][cw - 1];
    for (size_t g = 0; g < plan.groups.size(); ++g) {
        const uint8_t *d_blob = nullptr;
        int n_cus = 0;
        if ((rc = set_program(s, OP_MATCHES, cw, (int)g, &d_blob, &n_cus))) return rc;
        SetSpansArgs a;
        memset(&a, 0, sizeof(a));
        a.rows = (const uint8_t *)v->data;
        a.offsets = v->offsets;
        a.n_rows = v->n_rows;
        a.prog = d_blob;
        a.hdr = plan.groups[g].prog.hdr;
        a.span_off = d_span_offsets;
        a.start = d_start;
        a.end = d_end;
        a.masks = d_masks;
        a.store = g == 0 ? 1u : 0u;
        HIP_TRY(launch_set_spans(cw, a, n_cus, (hipStream_t)stream_));
    }
    return NEEDLE_OK;
}

// ------------------------------------------------------------------------------------------------
// Capturing groups (needle_captures.h: the tagged DFA and its LDS program; needle_captures_spans.h: the kernel)
// ------------------------------------------------------------------------------------------------
static const char *const kCapReasonNames[] = {"available", "NEEDLE_CAPTURES_NULLABLE_LOOP", "NEEDLE_CAPTURES_NO_REGEX", "NEEDLE_CAPTURES_TOO_MANY_GROUPS",
                                              "NEEDLE_CAPTURES_TOO_BIG"};

// The pattern's capture tables and the program of `cw`, built on first use (under cap_mu).  *reason: CAP_OK or why there is none.
static int captures_program(needle_pattern *p, int cw, const CapProgram **prog, int *reason, std::string *why) {
    std::lock_guard<std::mutex> lk(p->cap_mu);
    if (!p->cap_built) {
        if (!p->has_regex) {
            p->cap.reason = CAP_NO_REGEX;
            p->cap.n_groups = -1;
            p->cap.why = "the pattern was not made by needle_compile: it has no regex text";
        } else {
            p->cap_rc = build_captures(p->regex, p->regex_flags, p->cap, p->cap_err);
        }
        p->cap_built = true;
    }
    if (p->cap_rc != NEEDLE_OK) return fail(p->cap_rc, p->cap_err);
    *reason = p->cap.reason;
    *why = p->cap.why;
    *prog = nullptr;
    if (p->cap.reason != CAP_OK) return NEEDLE_OK;
    if (!p->cap_lowered[cw - 1]) {
        p->cap_prog[cw - 1] = lower_captures(p->cap, cw);
        p->cap_lowered[cw - 1] = true;
    }
    if (!p->cap_prog[cw - 1].ok) {
        *reason = CAP_TOO_BIG;
        *why = "the capture program and two waves' slot files do not fit the LDS";
        return NEEDLE_OK;
    }
    *prog = &p->cap_prog[cw - 1];
    return NEEDLE_OK;
}

int needle_pattern_captures_info(const needle_pattern *cp, int char_width, needle_captures_info *o) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p || !o) return fail(NEEDLE_ERR_INVALID, "captures_info: NULL argument");
    if (char_width != 1 && char_width != 2) return fail(NEEDLE_ERR_INVALID, "captures_info: char_width must be 1 or 2");
    const CapProgram *prog = nullptr;
    int reason = 0;
    std::string why;
    if (int rc = captures_program(p, char_width, &prog, &reason, &why)) return rc;
    memset(o, 0, sizeof(*o));
    o->available = reason == CAP_OK;
    o->reason = reason;
    o->n_groups = p->cap.n_groups;
    if (reason == CAP_OK) {
        o->n_states = p->cap.n_states;
        o->n_cols = p->cap.n_cols;
        o->max_threads = p->cap.max_threads;
        o->n_slots = p->cap.n_slots;
        o->n_op_lists = p->cap.n_op_lists;
        o->n_ops = (int32_t)(p->cap.ops.size() / 2);
        o->start = p->cap.start;
        o->init_op = p->cap.init_op;
        o->lds_bytes = (int32_t)prog->hdr.lds_bytes;
    }
    return NEEDLE_OK;
}

int needle_pattern_captures_tables(const needle_pattern *cp, int char_width, uint8_t *class_map, int32_t *next, int32_t *op_id, size_t table_cap,
                                   int32_t *op_off, size_t op_off_cap, int32_t *ops, size_t ops_cap, int32_t *fin, size_t fin_cap) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p) return fail(NEEDLE_ERR_INVALID, "captures_tables: pattern is NULL");
    if (char_width != 1 && char_width != 2) return fail(NEEDLE_ERR_INVALID, "captures_tables: char_width must be 1 or 2");
    const CapProgram *prog = nullptr;
    int reason = 0;
    std::string why;
    if (int rc = captures_program(p, char_width, &prog, &reason, &why)) return rc;
    if (reason != CAP_OK) return fail(NEEDLE_ERR_UNSUPPORTED, std::string(kCapReasonNames[reason]) + ": " + why);
    const CapTables &t = p->cap;
    if (class_map) memcpy(class_map, t.class_map.data(), 65536);
    auto put = [](int32_t *dst, size_t cap, const std::vector<int32_t> &src) {
        if (!dst) return true;
        if (cap < src.size()) return false;
        if (!src.empty()) memcpy(dst, src.data(), src.size() * 4);
        return true;
    };
    if (!put(next, table_cap, t.next) || !put(op_id, table_cap, t.op_id)) return fail(NEEDLE_ERR_INVALID, "captures_tables: table buffer too small");
    if (!put(op_off, op_off_cap, t.op_off)) return fail(NEEDLE_ERR_INVALID, "captures_tables: op_off buffer too small");
    if (!put(ops, ops_cap, t.ops)) return fail(NEEDLE_ERR_INVALID, "captures_tables: ops buffer too small");
    if (!put(fin, fin_cap, t.fin)) return fail(NEEDLE_ERR_INVALID, "captures_tables: fin buffer too small");
    return NEEDLE_OK;
}

// The groups of each span of a CSR span list (needle_captures_spans.h): a pure function of (text, list, pattern).
int needle_captures_spans_packed_dev(const needle_pattern *cp, const needle_packed_view *v, const uint64_t *d_span_offsets, const int32_t *d_start,
                                     const int32_t *d_end, int32_t *d_group_start, int32_t *d_group_end, uint64_t plane_stride, void *stream_) {
    needle_pattern *p = const_cast<needle_pattern *>(cp);
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (!d_span_offsets) return fail(NEEDLE_ERR_INVALID, "span offsets is NULL");
    if ((d_start == nullptr) != (d_end == nullptr)) return fail(NEEDLE_ERR_INVALID, "one of start / end is NULL without the other");
    if (d_start && (!d_group_start || !d_group_end)) return fail(NEEDLE_ERR_INVALID, "group planes are NULL with a span list");
    if (((uintptr_t)v->data) % 4 != 0) return fail(NEEDLE_ERR_INVALID, "packed data must be 4-byte aligned");
    const int cw = (int)v->char_width;
    const CapProgram *prog = nullptr;
    int reason = 0;
    std::string why;
    if ((rc = captures_program(p, cw, &prog, &reason, &why))) return rc;
    if (reason != CAP_OK) return fail(NEEDLE_ERR_UNSUPPORTED, std::string(kCapReasonNames[reason]) + ": " + why);
    if (v->n_rows == 0 || !d_start) return NEEDLE_OK; // (no rows, or no spans at all)
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const uint8_t *d_blob = nullptr;
    int n_cus = 0;
    {
        std::lock_guard<std::mutex> lk(p->cap_mu);
        if (!p->cap_cus.count(dev)) {
            hipDeviceProp_t prop;
            HIP_TRY(hipGetDeviceProperties(&prop, dev));
            p->cap_cus[dev] = prop.multiProcessorCount;
        }
        n_cus = p->cap_cus[dev];
        auto it = p->cap_resident.find(std::make_pair(dev, cw));
        if (it == p->cap_resident.end()) {
            uint8_t *d = nullptr;
            HIP_TRY(hipMalloc((void **)&d, prog->blob.size()));
            if (hipError_t ce = hipMemcpy(d, prog->blob.data(), prog->blob.size(), hipMemcpyHostToDevice); ce != hipSuccess) {
                (void)hipFree(d);
                return hip_fail(ce, "hipMemcpy(capture program)");
            }
            it = p->cap_resident.emplace(std::make_pair(dev, cw), d).first;
        }
        d_blob = it->second;
    }
    CapSpansArgs a;
    memset(&a, 0, sizeof(a));
    a.rows = (const uint8_t *)v->data;
    a.offsets = v->offsets;
    a.n_rows = v->n_rows;
    a.prog = d_blob;
    a.hdr = prog->hdr;
    a.span_off = d_span_offsets;
    a.start = d_start;
    a.end = d_end;
    a.gstart = d_group_start;
    a.gend = d_group_end;
    a.plane_stride = plane_stride;
    HIP_TRY(launch_captures_spans(cw, a, n_cus, (hipStream_t)stream_));
    return NEEDLE_OK;
}

} // extern "C"
