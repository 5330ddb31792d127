// The host-buffer layer of the C ABI: the needle_*_host entries and the single-haystack Matcher mirror that is their client.  It knows
// nothing of programs, routes or kernels: a host batch is cut into chunks that keep a bounded amount resident on the device
// (needle_host_plan.h), and every chunk is uploaded, handed to the public _dev entry and its results downloaded.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/needle_hip.h"
#include "needle_device.h"
#include "needle_host_plan.h"
#include "needle_internal.h"

using namespace needle;

static int fail(int code, const std::string &msg) { return set_error(code, msg); }

// NEEDLE_HOST_CHUNK_BYTES: what the host entry points keep resident on the device at a time (tests shrink it).
static uint64_t host_chunk_bytes() {
    static const uint64_t v = getenv("NEEDLE_HOST_CHUNK_BYTES") ? (uint64_t)atoll(getenv("NEEDLE_HOST_CHUNK_BYTES")) : (2ull << 30);
    return v;
}
// NEEDLE_HOST_RESULT_BYTES: the bound on the find-all results the host entry points keep resident on the device at a time (tests shrink it).
static uint64_t host_result_bytes() {
    static const uint64_t v = getenv("NEEDLE_HOST_RESULT_BYTES") ? (uint64_t)atoll(getenv("NEEDLE_HOST_RESULT_BYTES")) : (512ull << 20);
    return v;
}

// A fixed-stride host batch.  Per-row lengths are readable here, so an oversized one is an argument error, not an out-of-bounds read on
// the device (the kernels derive their chunk counts from the lengths and trust len <= row_stride).
static int check_host_view(const needle_batch_view *v) {
    if (!v) return fail(NEEDLE_ERR_INVALID, "batch view is NULL");
    if (v->char_width != 1 && v->char_width != 2) return fail(NEEDLE_ERR_INVALID, "char_width must be 1 or 2");
    if (v->n_rows && !v->rows) return fail(NEEDLE_ERR_INVALID, "rows is NULL");
    if (v->row_len > v->row_stride) return fail(NEEDLE_ERR_INVALID, "row_len > row_stride");
    if (v->lengths)
        for (uint64_t r = 0; r < v->n_rows; ++r)
            if (v->lengths[r] > v->row_stride) return fail(NEEDLE_ERR_INVALID, "lengths[r] > row_stride");
    return NEEDLE_OK;
}

// The offsets of a packed host batch (readable here): non-decreasing, no row beyond `limit` chars (`beyond`: what to say of one that is),
// text behind them.
static int check_packed_rows(const needle_packed_view *v, uint64_t limit, const char *beyond) {
    const uint64_t *off = v->offsets;
    for (uint64_t r = 0, n = v->n_rows; r < n; ++r) {
        if (off[r + 1] < off[r]) return fail(NEEDLE_ERR_INVALID, "offsets must be non-decreasing");
        if (off[r + 1] - off[r] > limit) return fail(NEEDLE_ERR_UNSUPPORTED, beyond);
    }
    if (off[v->n_rows] > off[0] && !v->data) return fail(NEEDLE_ERR_INVALID, "data is NULL");
    return NEEDLE_OK;
}

// The one device buffer of a host chunk: freed on every return path.
struct DevSlab {
    uint8_t *d = nullptr;
    DevSlab() = default;
    DevSlab(const DevSlab &) = delete;
    DevSlab &operator=(const DevSlab &) = delete;
    ~DevSlab() {
        if (d) (void)hipFree(d);
    }
    hipError_t alloc(uint64_t bytes) { return hipMalloc((void **)&d, bytes ? bytes : 16); }
};

// The rows of a host batch on the device, padded to a stride of whole 16 bytes (zero-filled), and their lengths (d_len: not used without
// lengths).  *dv: the batch as a device view.
static hipError_t upload_rows(const needle_batch_view *v, void *d_rows, uint32_t *d_len, needle_batch_view *dv) {
    const uint64_t src_stride = v->row_stride * v->char_width, dst_stride = padded_stride_bytes(v->row_stride, v->char_width);
    hipError_t e = hipSuccess;
    if (dst_stride == src_stride) {
        e = hipMemcpy(d_rows, v->rows, v->n_rows * src_stride, hipMemcpyHostToDevice);
    } else {
        e = hipMemset(d_rows, 0, v->n_rows * dst_stride);
        if (e == hipSuccess && src_stride) e = hipMemcpy2D(d_rows, dst_stride, v->rows, src_stride, src_stride, v->n_rows, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && v->lengths) e = hipMemcpy(d_len, v->lengths, v->n_rows * 4, hipMemcpyHostToDevice);
    *dv = *v;
    dv->rows = d_rows;
    dv->lengths = v->lengths ? d_len : nullptr;
    dv->row_stride = dst_stride / v->char_width;
    return e;
}

// Upload chunk [r0, r1) of a packed host batch: its text to d_data, its offsets rebased to the chunk's first char to d_offsets (the
// caller's own when that is char 0; `local` holds the rebased copy).  *dv: the chunk as a device view.
static hipError_t upload_packed_chunk(const needle_packed_view *v, uint64_t r0, uint64_t r1, uint8_t *d_data, uint64_t *d_offsets,
                                      std::vector<uint64_t> &local, needle_packed_view *dv) {
    const uint64_t nr = r1 - r0, cw = v->char_width, c0 = v->offsets[r0], text = (v->offsets[r1] - c0) * cw;
    const uint64_t *off = v->offsets + r0;
    if (c0) {
        local.resize(nr + 1);
        for (uint64_t r = 0; r <= nr; ++r) local[r] = v->offsets[r0 + r] - c0;
        off = local.data();
    }
    hipError_t e = text ? hipMemcpy(d_data, (const uint8_t *)v->data + c0 * cw, text, hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpy(d_offsets, off, (nr + 1) * 8, hipMemcpyHostToDevice);
    *dv = *v;
    dv->data = d_data;
    dv->offsets = d_offsets;
    dv->n_rows = nr;
    return e;
}

// What a chunk's run() gets: the device buffer, and the download of one of its sections into the caller's memory (a synchronous copy on
// the null stream: it waits for the _dev entry's kernels there).
struct ChunkOut {
    uint8_t *d;
    const char *who;
    int download(void *dst, uint64_t off, uint64_t bytes) const {
        if (!bytes) return NEEDLE_OK;
        const hipError_t e = hipMemcpy(dst, d + off, bytes, hipMemcpyDeviceToHost);
        return e == hipSuccess ? NEEDLE_OK : hip_fail(e, (std::string(who) + " download").c_str());
    }
};

// Rows [r0, r0 + per) of a fixed-stride host batch (or what is left of it) as a batch of their own.
static needle_batch_view fixed_chunk(const needle_batch_view *v, uint64_t r0, uint64_t per) {
    needle_batch_view c = *v;
    c.n_rows = std::min<uint64_t>(per, v->n_rows - r0);
    c.rows = (const uint8_t *)v->rows + r0 * v->row_stride * v->char_width;
    c.lengths = v->lengths ? v->lengths + r0 : nullptr;
    return c;
}

// One chunk of a fixed-stride host batch on the device: ONE buffer of rows | lengths | whatever layout(lay, n) adds for the chunk's n rows
// (it returns the offsets it was given, for the caller's run); the rows uploaded.  *dv: the chunk as a device view.
template <class Layout>
static auto chunk_to_device(const needle_batch_view &c, const char *who, Layout &&layout, DevSlab &dev, needle_batch_view *dv, int *rc) {
    Slab lay;
    const uint64_t o_rows = lay.add(c.n_rows * padded_stride_bytes(c.row_stride, c.char_width)), o_len = lay.add(c.lengths ? c.n_rows * 4 : 0);
    const auto o = layout(lay, c.n_rows);
    hipError_t e = dev.alloc(lay.total());
    if (e == hipSuccess) e = upload_rows(&c, dev.d + o_rows, (uint32_t *)(dev.d + o_len), dv);
    *rc = e == hipSuccess ? NEEDLE_OK : hip_fail(e, (std::string(who) + " upload").c_str());
    return o;
}

// A fixed-stride host batch of any size: consecutive row chunks of at most NEEDLE_HOST_CHUNK_BYTES on the device -- a row costs its padded
// text + per_row bytes there -- that start on 64-row boundaries, so every chunk owns whole bitmap words.  Per chunk: chunk_to_device, then
// run(dv, out, r0, o) calls the _dev entry on the device view and downloads (o: what layout returned).
template <class Layout, class Run>
static int for_fixed_chunks(const needle_batch_view *v, uint64_t per_row, const char *who, Layout &&layout, Run &&run) {
    const uint64_t per = fixed_chunk_rows(padded_stride_bytes(v->row_stride, v->char_width), per_row, host_chunk_bytes());
    for (uint64_t r0 = 0; r0 < v->n_rows; r0 += per) {
        DevSlab dev;
        needle_batch_view dv;
        int rc = NEEDLE_OK;
        const auto o = chunk_to_device(fixed_chunk(v, r0, per), who, layout, dev, &dv, &rc);
        if (rc || (rc = run(dv, ChunkOut{dev.d, who}, r0, o))) return rc;
    }
    return NEEDLE_OK;
}

// A packed host batch (checked: check_packed_rows) of any size: the chunks of packed_chunks(per_row, align) within
// NEEDLE_HOST_CHUNK_BYTES.  ONE device buffer serves every chunk -- data | offsets | whatever layout(lay, nr) adds for a chunk of nr rows
// (it returns the offsets it was given) -- as large as the largest chunk needs; per chunk the text is uploaded with its offsets rebased, and
// run(dv, out, r0, o) calls the _dev entry on the device view and downloads (o: what layout returned for this chunk) -- one chunk after the
// other, no overlap of one chunk's upload with the previous chunk's scan.
template <class Layout, class Run>
static int for_packed_chunks(const needle_packed_view *v, uint64_t per_row, uint64_t align, const char *who, Layout &&layout, Run &&run) {
    const uint64_t cw = v->char_width;
    const std::vector<RowRange> chunks = packed_chunks(v->offsets, v->n_rows, cw, per_row, align, host_chunk_bytes());
    auto lay_out = [&](const RowRange &c, Slab &lay, uint64_t *o_off) {
        lay.add(std::max<uint64_t>((v->offsets[c.second] - v->offsets[c.first]) * cw, 4)); // (the data, at 0)
        *o_off = lay.add((c.second - c.first + 1) * 8);
        return layout(lay, c.second - c.first);
    };
    uint64_t all = 0, o_off = 0;
    for (const RowRange &c : chunks) {
        Slab lay;
        lay_out(c, lay, &o_off);
        all = std::max(all, lay.total());
    }
    DevSlab dev;
    HIP_TRY(dev.alloc(all));
    std::vector<uint64_t> local;
    for (const RowRange &c : chunks) {
        Slab lay;
        const auto o = lay_out(c, lay, &o_off);
        needle_packed_view dv;
        const hipError_t e = upload_packed_chunk(v, c.first, c.second, dev.d, (uint64_t *)(dev.d + o_off), local, &dv);
        if (e != hipSuccess) return hip_fail(e, (std::string(who) + " upload").c_str());
        const int rc = run(dv, ChunkOut{dev.d, who}, c.first, o);
        if (rc) return rc;
    }
    return NEEDLE_OK;
}

// ------------------------------------------------------------------------------------------------
// matches() / containedIn() / find() of fixed-stride host rows
// ------------------------------------------------------------------------------------------------
// Where the results of a scan of n rows lie in a chunk's buffer -- the bitmap, then two arrays of `bytes` each (start / end of find(), or
// its one-array forms: the second array is then not downloaded; bytes = 0: matches() / containedIn()) -- and their download.
struct ScanAt {
    uint64_t bm, s, e;
};
static ScanAt scan_sections(Slab &lay, uint64_t n, uint64_t bytes, bool two = false) {
    const uint64_t bm = lay.add((n + 63) / 64 * 8), s = lay.add(bytes);
    return ScanAt{bm, s, two ? lay.add(bytes) : s};
}
static int download_scan(const ChunkOut &out, const ScanAt &o, uint64_t n, uint64_t bytes, uint64_t *bitmap, void *start, void *end) {
    int rc = out.download(bitmap, o.bm, (n + 63) / 64 * 8);
    if (!rc && bytes) rc = out.download(start, o.s, bytes);
    return !rc && bytes && end ? out.download(end, o.e, bytes) : rc;
}

static int scan_dev(const needle_pattern *p, int op, const needle_batch_view *dv, uint64_t *d_bm, int32_t *d_s, int32_t *d_e, void *stream) {
    return op == OP_FIND ? needle_find_dev(p, dv, d_bm, d_s, d_e, stream)
                         : op == OP_MATCHES ? needle_matches_dev(p, dv, d_bm, stream) : needle_contained_in_dev(p, dv, d_bm, stream);
}

// Small host batches (above all the one-row batches of the Matcher mirror): one grow-only device arena + pinned
// staging buffer + stream per host thread, ONE upload and ONE download per call -- instead of a hipMalloc / hipFree
// pair and several synchronous copies.
namespace {
struct HostArena {
    int dev = -1;
    uint8_t *d = nullptr, *h = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
    ~HostArena() { release(); }
    void release() {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        if (stream) (void)hipStreamDestroy(stream);
        d = h = nullptr;
        stream = nullptr;
        cap = 0;
        dev = -1;
    }
    hipError_t reserve(size_t bytes) {
        int cur = 0;
        hipError_t e = hipGetDevice(&cur);
        if (e != hipSuccess) return e;
        if (cur == dev && bytes <= cap) return hipSuccess;
        release();
        size_t want = 1 << 16;
        while (want < bytes) want <<= 1;
        if ((e = hipMalloc((void **)&d, want)) != hipSuccess) return e;
        if ((e = hipHostMalloc((void **)&h, want, hipHostMallocMapped)) != hipSuccess) return e;
        if ((e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) != hipSuccess) return e;
        cap = want;
        dev = cur;
        return hipSuccess;
    }
};
constexpr size_t kSmallHostBatchBytes = 4u << 20;
constexpr size_t kZeroCopyBytes = 16u << 10;
} // namespace

static int run_host_small(const needle_pattern *p, int op, const needle_batch_view *v, uint64_t dst_stride, uint64_t *bitmap,
                          int32_t *start, int32_t *end) {
    static thread_local HostArena arena;
    const size_t cw = v->char_width, n = (size_t)v->n_rows;
    const size_t src_stride = (size_t)v->row_stride * cw;
    const size_t words = (n + 63) / 64;
    Slab lay; // in: rows | lengths      out: bitmap | start | end
    const size_t o_rows = lay.add(n * dst_stride), o_len = lay.add(v->lengths ? n * 4 : 0);
    const size_t o_bm = lay.add(words * 8), o_s = lay.add(n * 4), o_e = lay.add(n * 4), total = lay.total();
    HIP_TRY(arena.reserve(total));
    if (dst_stride == src_stride) {
        memcpy(arena.h + o_rows, v->rows, n * src_stride);
    } else {
        for (size_t r = 0; r < n; ++r) {
            memcpy(arena.h + o_rows + r * dst_stride, (const uint8_t *)v->rows + r * src_stride, src_stride);
            memset(arena.h + o_rows + r * dst_stride + src_stride, 0, dst_stride - src_stride);
        }
    }
    if (v->lengths) memcpy(arena.h + o_len, v->lengths, n * 4);
    // Tiny batches (one Matcher call): the kernel reads the pinned staging buffer and writes its results there
    // directly over PCIe -- one launch and one wait, no copy commands at all.
    const bool zero_copy = total <= kZeroCopyBytes;
    uint8_t *base = arena.d;
    if (zero_copy) {
        void *mapped = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&mapped, arena.h, 0));
        base = (uint8_t *)mapped;
    } else {
        HIP_TRY(hipMemcpyAsync(arena.d, arena.h, o_bm, hipMemcpyHostToDevice, arena.stream));
    }
    needle_batch_view dv = *v;
    dv.rows = base + o_rows;
    dv.lengths = v->lengths ? (const uint32_t *)(base + o_len) : nullptr;
    dv.row_stride = dst_stride / cw;
    int rc = scan_dev(p, op, &dv, (uint64_t *)(base + o_bm), (int32_t *)(base + o_s), (int32_t *)(base + o_e), arena.stream);
    if (rc) return rc;
    if (!zero_copy) {
        const size_t out_bytes = op == OP_FIND ? total - o_bm : words * 8;
        HIP_TRY(hipMemcpyAsync(arena.h + o_bm, arena.d + o_bm, out_bytes, hipMemcpyDeviceToHost, arena.stream));
    }
    HIP_TRY(hipStreamSynchronize(arena.stream));
    memcpy(bitmap, arena.h + o_bm, words * 8);
    if (op == OP_FIND) {
        memcpy(start, arena.h + o_s, n * 4);
        memcpy(end, arena.h + o_e, n * 4);
    }
    return NEEDLE_OK;
}

// Host-buffer convenience: pad rows to a 16-byte stride, upload, run, download.  Every chunk on its own takes the arena when it is small
// (tests shrink the chunks; the last chunk of a large batch).
static int run_host(const needle_pattern *p, int op, const needle_batch_view *v, uint64_t *bitmap, int32_t *start, int32_t *end) {
    int rc = check_host_view(v);
    if (rc) return rc;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!bitmap) return fail(NEEDLE_ERR_INVALID, "bitmap is NULL");
    if (op == OP_FIND && (!start || !end)) return fail(NEEDLE_ERR_INVALID, "start/end is NULL");
    const uint64_t dst_stride = padded_stride_bytes(v->row_stride, v->char_width), per = fixed_chunk_rows(dst_stride, 0, host_chunk_bytes());
    const uint64_t fb = op == OP_FIND ? 4 : 0; // bytes per row of start / of end
    for (uint64_t r0 = 0; r0 < v->n_rows; r0 += per) {
        const needle_batch_view c = fixed_chunk(v, r0, per);
        uint64_t *bm = bitmap + r0 / 64;
        int32_t *st = start ? start + r0 : nullptr, *en = end ? end + r0 : nullptr;
        if (c.n_rows * dst_stride + c.n_rows * 16 <= kSmallHostBatchBytes) {
            rc = run_host_small(p, op, &c, dst_stride, bm, st, en);
        } else {
            DevSlab dev;
            needle_batch_view dv;
            const ScanAt o = chunk_to_device(c, "needle_*_host", [&](Slab &lay, uint64_t n) { return scan_sections(lay, n, fb * n, true); }, dev, &dv, &rc);
            if (rc || (rc = scan_dev(p, op, &dv, (uint64_t *)(dev.d + o.bm), (int32_t *)(dev.d + o.s), (int32_t *)(dev.d + o.e), nullptr))) return rc;
            HIP_TRY(hipDeviceSynchronize());
            rc = download_scan(ChunkOut{dev.d, "needle_*_host"}, o, c.n_rows, fb * c.n_rows, bm, st, en);
        }
        if (rc) return rc;
    }
    return NEEDLE_OK;
}

// ------------------------------------------------------------------------------------------------
// matches() / containedIn() / find() of packed host rows (the String[] drop-in path), as fixed-stride rows
// ------------------------------------------------------------------------------------------------
// One packed host batch (checked: rows of up to max_len chars) as fixed-stride rows of one stride: chunks of whole 64-row groups within
// NEEDLE_HOST_CHUNK_BYTES -- a row costs its text + its padded row + length + offset (+ start / end) -- uploaded, unpacked on the device,
// scanned, downloaded.
static int run_packed_host_one(const needle_pattern *p, int op, const needle_packed_view *v, uint64_t max_len, uint64_t *bitmap,
                               int32_t *start, int32_t *end) {
    const uint64_t cw = v->char_width, stride_bytes = padded_stride_bytes(max_len, cw), fb = op == OP_FIND ? 4 : 0;
    struct At {
        uint64_t rows, len;
        ScanAt scan;
    };
    return for_packed_chunks(
        v, stride_bytes + 12 + (op == OP_FIND ? 8 : 0), 64, "needle_*_packed_host",
        [&](Slab &lay, uint64_t nr) {
            const uint64_t rows = lay.add(nr * stride_bytes), len = lay.add(nr * 4);
            return At{rows, len, scan_sections(lay, nr, fb * nr, true)};
        },
        [&](const needle_packed_view &dv, const ChunkOut &out, uint64_t r0, const At &o) {
            uint32_t *d_len = (uint32_t *)(out.d + o.len);
            int rc = needle_rows_from_packed_dev(&dv, out.d + o.rows, stride_bytes / cw, d_len, nullptr, nullptr);
            if (rc) return rc;
            const needle_batch_view bv{out.d + o.rows, v->char_width, dv.n_rows, stride_bytes / cw, 0, d_len};
            rc = scan_dev(p, op, &bv, (uint64_t *)(out.d + o.scan.bm), (int32_t *)(out.d + o.scan.s), (int32_t *)(out.d + o.scan.e), nullptr);
            if (rc) return rc;
            HIP_TRY(hipDeviceSynchronize());
            return download_scan(out, o.scan, dv.n_rows, fb * dv.n_rows, bitmap + r0 / 64, start ? start + r0 : nullptr, end ? end + r0 : nullptr);
        });
}

// Packed host batch.  The fixed-stride layout the kernels read pads every row to the longest one: harmless when the
// lengths are alike, ruinous when one 1 MB document sits among a million 40-char strings.  Rows are therefore grouped
// into length classes (needle_host_plan.h) and every class runs as its own batch, so the padded bytes stay below 4x the text.
static int run_packed_host(const needle_pattern *p, int op, const needle_packed_view *v, uint64_t *bitmap, int32_t *start,
                           int32_t *end) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!bitmap) return fail(NEEDLE_ERR_INVALID, "bitmap is NULL");
    if (op == OP_FIND && (!start || !end)) return fail(NEEDLE_ERR_INVALID, "start/end is NULL");
    const uint64_t cw = v->char_width, n = v->n_rows;
    if ((rc = check_packed_rows(v, ~0ull, ""))) return rc;
    uint64_t max_len = 0; // (a pass of its own: without the early returns of the check it is a vector loop)
    for (uint64_t r = 0; r < n; ++r) max_len = std::max<uint64_t>(max_len, v->offsets[r + 1] - v->offsets[r]);
    if (max_len > 0xFFFFFFFFull) return fail(NEEDLE_ERR_INVALID, "row longer than 2^32 - 1 chars");
    const uint64_t total_bytes = v->offsets[n] * cw;
    if (n * padded_stride_bytes(max_len, cw) <= 4 * total_bytes + (64u << 10)) return run_packed_host_one(p, op, v, max_len, bitmap, start, end);
    std::vector<std::vector<uint64_t>> rows_of((size_t)length_class(max_len * cw) + 1);
    for (uint64_t r = 0; r < n; ++r) rows_of[(size_t)length_class((v->offsets[r + 1] - v->offsets[r]) * cw)].push_back(r);
    memset(bitmap, 0, ((n + 63) / 64) * 8);
    std::vector<uint8_t> data;
    std::vector<uint64_t> off, bm;
    std::vector<int32_t> st, en;
    for (const auto &ids : rows_of) {
        if (ids.empty()) continue;
        off.assign(ids.size() + 1, 0);
        uint64_t longest = 0;
        for (size_t i = 0; i < ids.size(); ++i) {
            const uint64_t len = v->offsets[ids[i] + 1] - v->offsets[ids[i]];
            off[i + 1] = off[i] + len;
            longest = std::max(longest, len);
        }
        data.resize((size_t)(off.back() * cw));
        for (size_t i = 0; i < ids.size(); ++i)
            memcpy(data.data() + off[i] * cw, (const uint8_t *)v->data + v->offsets[ids[i]] * cw, (size_t)((off[i + 1] - off[i]) * cw));
        const needle_packed_view sub{data.data(), v->char_width, ids.size(), off.data()};
        bm.assign((ids.size() + 63) / 64, 0);
        if (op == OP_FIND) {
            st.assign(ids.size(), -1);
            en.assign(ids.size(), -1);
        }
        rc = run_packed_host_one(p, op, &sub, longest, bm.data(), st.data(), en.data());
        if (rc) return rc;
        for (size_t i = 0; i < ids.size(); ++i) {
            if ((bm[i >> 6] >> (i & 63)) & 1) bitmap[ids[i] >> 6] |= 1ull << (ids[i] & 63);
            if (op == OP_FIND) {
                start[ids[i]] = st[i];
                end[ids[i]] = en[i];
            }
        }
    }
    return NEEDLE_OK;
}

// needle_find_packed{16,8}_packed_host: the offsets checked on the host (a row beyond the form: NEEDLE_ERR_UNSUPPORTED before any
// device call), then chunks of whole 64-row groups (the bitmap words stay the caller's; text + offset + result per row within the
// budget) scanned by needle_find_packed{16,8}_packed_dev where they lie.
static int run_packed_compact_host(const needle_pattern *p, const needle_packed_view *v, uint64_t *bitmap, void *res, bool packed8) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!bitmap || !res) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    const uint64_t rb = packed8 ? 2 : 4;
    rc = check_packed_rows(v, packed8 ? 256 : 65534,
                           packed8 ? "8-bit start / length: rows of at most 256 chars (use needle_find_packed16_packed_host)"
                                   : "16-bit offsets: rows of at most 65 534 chars (use needle_find_packed_host)");
    if (rc) return rc;
    return for_packed_chunks(
        v, 8 + rb, 64, "find_packed_packed_host", [&](Slab &lay, uint64_t nr) { return scan_sections(lay, nr, nr * rb); },
        [&](const needle_packed_view &dv, const ChunkOut &out, uint64_t r0, const ScanAt &o) {
            const int rc = packed8 ? needle_find_packed8_packed_dev(p, &dv, (uint64_t *)(out.d + o.bm), (uint16_t *)(out.d + o.s), nullptr, nullptr)
                                   : needle_find_packed16_packed_dev(p, &dv, (uint64_t *)(out.d + o.bm), (uint32_t *)(out.d + o.s), nullptr, nullptr);
            return rc ? rc : download_scan(out, o, dv.n_rows, dv.n_rows * rb, bitmap + r0 / 64, (uint8_t *)res + r0 * rb, nullptr);
        });
}

// A packed HOST batch through a pattern set: consecutive-row chunks (offset + mask per row) scanned where they lie by the _dev entry.
static int run_set_packed_host(const needle_pattern_set *s, int op, const needle_packed_view *v, uint32_t *masks) {
    if (!s) return fail(NEEDLE_ERR_INVALID, "pattern set is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (!masks) return fail(NEEDLE_ERR_INVALID, "masks is NULL");
    if (v->n_rows == 0) return NEEDLE_OK;
    if ((rc = set_plan_usable(s, op, (int)v->char_width))) return rc;
    if ((rc = check_packed_rows(v, ~0ull, ""))) return rc;
    return for_packed_chunks(v, 8 + 4, 1, "set_packed_host", [&](Slab &lay, uint64_t nr) { return lay.add(nr * 4); },
                             [&](const needle_packed_view &dv, const ChunkOut &out, uint64_t r0, uint64_t o_res) {
                                 const int rc = op == OP_MATCHES ? needle_set_matches_packed_dev(s, &dv, (uint32_t *)(out.d + o_res), nullptr)
                                                                 : needle_set_contained_in_packed_dev(s, &dv, (uint32_t *)(out.d + o_res), nullptr);
                                 return rc ? rc : out.download(masks + r0, o_res, dv.n_rows * 4);
                             });
}

// ------------------------------------------------------------------------------------------------
// Every match of every row
// ------------------------------------------------------------------------------------------------
// The fill pass of the CSR host entries over rows [r0, r1), whose counts stand summed up in `offsets`.  It runs over sub-ranges of the rows so
// that the results resident on the device stay bounded too (NEEDLE_HOST_RESULT_BYTES): a dense-match batch (a one-char pattern over
// 256-char rows files ~2 KiB per row) would otherwise ask for several times the chunk's row bytes in one allocation.
// fill(a, n, d_csr, d_start, d_end, &more): the layout's fill of rows [a, a + n) at the sub-range's own offsets, uploaded to d_csr.
// masks != nullptr (needle_set_tag_matches_packed_host): a third result array of 4 bytes per match -- tag(a, n, d_csr, d_start, d_end,
// d_masks) fills it behind the fill, and it is downloaded with the other two.
template <class Fill, class Tag>
static int csr_fill_pass(const std::string &who, const uint64_t *offsets, uint64_t r0, uint64_t r1, uint8_t *d_csr, int32_t *start, int32_t *end,
                         Fill &&fill, uint32_t *masks, Tag &&tag) {
    const std::vector<RowRange> ranges = csr_ranges(offsets, r0, r1, std::max<uint64_t>(host_result_bytes() / csr_match_bytes(masks != nullptr), 1));
    uint64_t biggest = 0;
    for (const RowRange &rg : ranges) biggest = std::max<uint64_t>(biggest, offsets[rg.second] - offsets[rg.first]);
    Slab lay;
    const uint64_t o_s = lay.add(biggest * 4), o_e = lay.add(biggest * 4), o_m = lay.add(masks ? biggest * 4 : 0);
    DevSlab dev;
    hipError_t e = dev.alloc(lay.total());
    if (e != hipSuccess) return hip_fail(e, (who + " results").c_str());
    std::vector<uint64_t> local;
    for (const RowRange &rg : ranges) {
        const uint64_t a = rg.first, sn = rg.second - rg.first, m = offsets[rg.second] - offsets[a];
        if (m == 0) continue;
        local.resize(sn + 1);
        for (uint64_t r = 0; r <= sn; ++r) local[r] = offsets[a + r] - offsets[a];
        e = hipMemcpy(d_csr, local.data(), (sn + 1) * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, (who + " offsets").c_str());
        int more = 0;
        int rc = fill(a, sn, (const uint64_t *)d_csr, (int32_t *)(dev.d + o_s), (int32_t *)(dev.d + o_e), &more);
        if (rc) return rc;
        if (more) return fail(NEEDLE_ERR_DEVICE, who + ": count pass and fill pass disagree");
        if (masks && (rc = tag(a, sn, (const uint64_t *)d_csr, (const int32_t *)(dev.d + o_s), (const int32_t *)(dev.d + o_e), (uint32_t *)(dev.d + o_m))))
            return rc;
        e = hipMemcpy(start + offsets[a], dev.d + o_s, m * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(end + offsets[a], dev.d + o_e, m * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && masks) e = hipMemcpy(masks + offsets[a], dev.d + o_m, m * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, (who + " download").c_str());
    }
    return NEEDLE_OK;
}
template <class Fill>
static int csr_fill_pass(const std::string &who, const uint64_t *offsets, uint64_t r0, uint64_t r1, uint8_t *d_csr, int32_t *start, int32_t *end,
                         Fill &&fill) {
    return csr_fill_pass(who, offsets, r0, r1, d_csr, start, end, fill, nullptr,
                         [](uint64_t, uint64_t, const uint64_t *, const int32_t *, const int32_t *, uint32_t *) { return (int)NEEDLE_OK; });
}

// The sections of a CSR chunk: the counts of its n rows, and the offsets of the fill pass's current sub-range.
struct CsrAt {
    uint64_t cnt, csr;
};
static CsrAt csr_sections(Slab &lay, uint64_t n) {
    const uint64_t cnt = lay.add(n * 4);
    return CsrAt{cnt, lay.add((n + 1) * 8)};
}

// The counts of a chunk's rows [r0, r0 + n), downloaded (which synchronises with the count pass), summed up into offsets[r0 + 1 ..].
static int csr_offsets(const ChunkOut &out, uint64_t o_cnt, uint64_t r0, uint64_t n, std::vector<uint32_t> &counts, uint64_t *offsets) {
    counts.resize(n);
    if (int rc = out.download(counts.data(), o_cnt, n * 4)) return rc;
    for (uint64_t r = 0; r < n; ++r) offsets[r0 + r + 1] = offsets[r0 + r] + counts[r];
    return NEEDLE_OK;
}

// start_end16 != nullptr: the one-dword-per-match form (needle_find_all_packed16_dev) -- start / end are not used
static int find_all_host(const needle_pattern *p, const needle_batch_view *v, uint32_t slots, uint32_t *counts, int32_t *start,
                         int32_t *end, int *more, uint32_t *start_end16) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_host_view(v);
    if (rc) return rc;
    if (more) *more = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!counts || (slots && !start_end16 && (!start || !end))) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    // int32 results wanted, rows of at most 65 534 chars (an empty match at index 65 535 would read as an unfiled slot): the one-dword form
    // on the device and over PCIe (half the result bytes both ways), opened into the caller's two arrays here on the host.
    // (NEEDLE_FIND_ALL_ROUNDS: the tests' cross-check of the round-per-match form goes through needle_find_all_dev)
    const bool staged = !start_end16 && slots && !find_all_rounds_forced() && (v->lengths ? v->row_stride : v->row_len) <= 65534u;
    const bool one_dword = start_end16 || staged;
    std::vector<uint32_t> stage;
    struct At {
        uint64_t cnt, s, e;
    };
    return for_fixed_chunks(
        v, 8 + 8ull * slots, "find_all_host",
        [&](Slab &lay, uint64_t n) {
            const uint64_t cnt = lay.add(n * 4), s = lay.add(n * slots * 4);
            return At{cnt, s, one_dword ? s : lay.add(n * slots * 4)};
        },
        [&](const needle_batch_view &dv, const ChunkOut &out, uint64_t r0, const At &o) {
            const uint64_t n = dv.n_rows, slot_bytes = n * slots * 4;
            if (slots) HIP_TRY(hipMemset(out.d + o.s, 0xFF, o.e + slot_bytes - o.s)); // -1 in every slot
            int m = 0;
            int rc = one_dword ? needle_find_all_packed16_dev(p, &dv, slots, (uint32_t *)(out.d + o.cnt), (uint32_t *)(out.d + o.s), &m, nullptr)
                               : needle_find_all_dev(p, &dv, slots, (uint32_t *)(out.d + o.cnt), (int32_t *)(out.d + o.s), (int32_t *)(out.d + o.e), &m, nullptr);
            if (rc || (rc = out.download(counts + r0, o.cnt, n * 4))) return rc;
            if (m && more) *more = 1;
            if (staged) {
                stage.resize((size_t)n * slots);
                if ((rc = out.download(stage.data(), o.s, slot_bytes))) return rc;
                int32_t *so = start + r0 * slots, *eo = end + r0 * slots;
                for (size_t i = 0; i < stage.size(); ++i) {
                    const uint32_t w = stage[i];
                    const bool none = w == 0xFFFFFFFFu; // an unfiled slot (a real match has start <= end, never 0xFFFF | 0xFFFF << 16)
                    so[i] = none ? -1 : (int32_t)(w & 0xFFFFu);
                    eo[i] = none ? -1 : (int32_t)(w >> 16);
                }
                return (int)NEEDLE_OK;
            }
            if (start_end16) return out.download(start_end16 + r0 * slots, o.s, slot_bytes);
            if ((rc = out.download(start + r0 * slots, o.s, slot_bytes))) return rc;
            return out.download(end + r0 * slots, o.e, slot_bytes);
        });
}

extern "C" {

int needle_matches_host(const needle_pattern *p, const needle_batch_view *v, uint64_t *bm) {
    return run_host(p, OP_MATCHES, v, bm, nullptr, nullptr);
}
int needle_contained_in_host(const needle_pattern *p, const needle_batch_view *v, uint64_t *bm) {
    return run_host(p, OP_CONTAINED_IN, v, bm, nullptr, nullptr);
}
int needle_find_host(const needle_pattern *p, const needle_batch_view *v, uint64_t *bm, int32_t *st, int32_t *en) {
    return run_host(p, OP_FIND, v, bm, st, en);
}

int needle_matches_packed_host(const needle_pattern *p, const needle_packed_view *v, uint64_t *bm) {
    return run_packed_host(p, OP_MATCHES, v, bm, nullptr, nullptr);
}
int needle_contained_in_packed_host(const needle_pattern *p, const needle_packed_view *v, uint64_t *bm) {
    return run_packed_host(p, OP_CONTAINED_IN, v, bm, nullptr, nullptr);
}
int needle_find_packed_host(const needle_pattern *p, const needle_packed_view *v, uint64_t *bm, int32_t *st, int32_t *en) {
    return run_packed_host(p, OP_FIND, v, bm, st, en);
}

int needle_find_packed16_packed_host(const needle_pattern *p, const needle_packed_view *v, uint64_t *bitmap, uint32_t *start_end16) {
    return run_packed_compact_host(p, v, bitmap, start_end16, false);
}
int needle_find_packed8_packed_host(const needle_pattern *p, const needle_packed_view *v, uint64_t *bitmap, uint16_t *start_len8) {
    return run_packed_compact_host(p, v, bitmap, start_len8, true);
}

int needle_set_matches_packed_host(const needle_pattern_set *s, const needle_packed_view *v, uint32_t *masks) {
    return run_set_packed_host(s, OP_MATCHES, v, masks);
}
int needle_set_contained_in_packed_host(const needle_pattern_set *s, const needle_packed_view *v, uint32_t *masks) {
    return run_set_packed_host(s, OP_CONTAINED_IN, v, masks);
}

int needle_find_all_host(const needle_pattern *p, const needle_batch_view *v, uint32_t slots, uint32_t *counts, int32_t *start,
                         int32_t *end, int *more) {
    return find_all_host(p, v, slots, counts, start, end, more, nullptr);
}
int needle_find_all_packed16_host(const needle_pattern *p, const needle_batch_view *v, uint32_t slots, uint32_t *counts,
                                  uint32_t *start_end16, int *more) {
    if (slots && !start_end16) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (v && (v->lengths ? v->row_stride : v->row_len) > 65535u) // (the caller's stride, before any padding; lengths[r] <= row_stride is checked below)
        return fail(NEEDLE_ERR_UNSUPPORTED, "16-bit start / end: rows of at most 65535 chars");
    static uint32_t none = 0; // (slots == 0: counting only; a non-null marker keeps the packed form)
    return find_all_host(p, v, slots, counts, nullptr, nullptr, more, start_end16 ? start_end16 : &none);
}

// (like the other host entry points: at most ~2 GiB of rows + results resident on the device at a time)
// Per chunk: upload, count pass, prefix sum on the host (the counts come back anyway), fill pass while the rows are still resident, download.
int needle_find_all_csr_host(const needle_pattern *p, const needle_batch_view *v, uint64_t *offsets, int32_t *start, int32_t *end,
                             uint64_t capacity, uint64_t *total) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_host_view(v);
    if (rc) return rc;
    if (!offsets || !total || (capacity && (!start || !end))) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    offsets[0] = 0;
    *total = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    std::vector<uint32_t> counts;
    rc = for_fixed_chunks(
        v, 16, "find_all_csr_host", csr_sections,
        [&](const needle_batch_view &dv, const ChunkOut &out, uint64_t r0, const CsrAt &o) {
            const uint64_t n = dv.n_rows;
            int rc = needle_count_matches_dev(p, &dv, (uint32_t *)(out.d + o.cnt), nullptr);
            if (rc || (rc = csr_offsets(out, o.cnt, r0, n, counts, offsets))) return rc;
            if (offsets[r0 + n] == offsets[r0] || offsets[r0 + n] > capacity) return (int)NEEDLE_OK; // nothing to file, or the caller's buffers are too small
            return csr_fill_pass("find_all_csr_host", offsets, r0, r0 + n, out.d + o.csr, start, end,
                                 [&](uint64_t a, uint64_t sn, const uint64_t *d_csr, int32_t *d_s, int32_t *d_e, int *more) {
                                     needle_batch_view sv = dv;
                                     sv.rows = (const uint8_t *)dv.rows + (a - r0) * dv.row_stride * dv.char_width;
                                     sv.lengths = dv.lengths ? dv.lengths + (a - r0) : nullptr;
                                     sv.n_rows = sn;
                                     return needle_find_all_csr_dev(p, &sv, d_csr, d_s, d_e, more, nullptr);
                                 });
        });
    if (rc == NEEDLE_OK) *total = offsets[v->n_rows];
    return rc;
}

// The packed batch in host memory: row chunks of at most NEEDLE_HOST_CHUNK_BYTES of text (12 bytes per row: offset + count) are uploaded,
// counted, the prefix sum built here, filled (in sub-ranges of at most NEEDLE_HOST_RESULT_BYTES of results) and downloaded.
// set != NULL (needle_set_tag_matches_packed_host): every match's member mask beside it, tagged on the device while the rows are resident.
static int find_all_csr_packed_host(const char *who, const needle_pattern *p, const needle_packed_view *v, uint64_t *offsets, int32_t *start,
                                    int32_t *end, uint64_t capacity, uint64_t *total, const needle_pattern_set *set, uint32_t *masks) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (!offsets || !total || (capacity && (!start || !end || (set && !masks)))) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    offsets[0] = 0;
    *total = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (set && (rc = set_plan_usable(set, OP_MATCHES, (int)v->char_width))) return rc;
    if ((rc = check_packed_rows(v, ~0ull, ""))) return rc;
    std::vector<uint32_t> counts;
    rc = for_packed_chunks(
        v, 12, 1, who, csr_sections,
        [&](const needle_packed_view &dv, const ChunkOut &out, uint64_t r0, const CsrAt &o) {
            const uint64_t r1 = r0 + dv.n_rows;
            int rc = needle_count_matches_packed_dev(p, &dv, (uint32_t *)(out.d + o.cnt), nullptr);
            if (rc || (rc = csr_offsets(out, o.cnt, r0, dv.n_rows, counts, offsets))) return rc;
            if (offsets[r1] == offsets[r0] || offsets[r1] > capacity) return (int)NEEDLE_OK;
            auto sub = [&](uint64_t a, uint64_t sn) {
                needle_packed_view sv = dv;
                sv.offsets = dv.offsets + (a - r0);
                sv.n_rows = sn;
                return sv;
            };
            return csr_fill_pass(
                who, offsets, r0, r1, out.d + o.csr, start, end,
                [&](uint64_t a, uint64_t sn, const uint64_t *d_csr, int32_t *d_s, int32_t *d_e, int *more) {
                    const needle_packed_view sv = sub(a, sn);
                    return needle_find_all_csr_packed_dev(p, &sv, d_csr, d_s, d_e, more, nullptr);
                },
                set ? masks : nullptr,
                [&](uint64_t a, uint64_t sn, const uint64_t *d_csr, const int32_t *d_s, const int32_t *d_e, uint32_t *d_m) {
                    const needle_packed_view sv = sub(a, sn);
                    return needle_set_matches_spans_packed_dev(set, &sv, d_csr, d_s, d_e, d_m, nullptr);
                });
        });
    if (rc == NEEDLE_OK) *total = offsets[v->n_rows];
    return rc;
}

int needle_find_all_csr_packed_host(const needle_pattern *p, const needle_packed_view *v, uint64_t *offsets, int32_t *start, int32_t *end,
                                    uint64_t capacity, uint64_t *total) {
    return find_all_csr_packed_host("find_all_csr_packed_host", p, v, offsets, start, end, capacity, total, nullptr, nullptr);
}

// Every match of `p` in every row with the mask of the set's members that match it whole (needle_set_matches_spans_packed_dev).
int needle_set_tag_matches_packed_host(const needle_pattern_set *s, const needle_pattern *p, const needle_packed_view *v, uint64_t *offsets,
                                       int32_t *start, int32_t *end, uint32_t *masks, uint64_t capacity, uint64_t *total) {
    if (!s) return fail(NEEDLE_ERR_INVALID, "pattern set is NULL");
    return find_all_csr_packed_host("set_tag_matches_packed_host", p, v, offsets, start, end, capacity, total, s, masks);
}

} // extern "C"

// Replace every match of a packed HOST batch.  Per chunk of rows (36 bytes per row: offset, count, match offset, length, output offset):
// upload, count pass, prefix sum here; then in sub-ranges of at most NEEDLE_HOST_RESULT_BYTES of matches: CSR fill, lengths, prefix sum
// here into the caller's out_offsets; then, while the caller's buffer has room, in sub-ranges of at most NEEDLE_HOST_RESULT_BYTES of
// output text: splice and download.  The offsets handed to the device are rebased to each sub-range.
// set != NULL (needle_set_replace_each_packed_host): repl is a table of set's-pattern-count entries at repl_offsets; every match is tagged
// by the set in the sub-range loop of the CSR fill, and the masks go straight into the each-entries (NEEDLE_CHOICE_LOWEST_BIT).
static int replace_packed_host(const char *who, const needle_pattern *p, const needle_packed_view *v, const void *repl, uint32_t repl_len,
                               const needle_pattern_set *set, const uint32_t *repl_offsets, uint32_t n_repl, uint64_t *out_offsets, void *out_data,
                               uint64_t capacity, uint64_t *total) {
    int rc = 0;
    out_offsets[0] = 0;
    *total = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if ((rc = check_packed_rows(v, ~0ull, ""))) return rc;
    const uint64_t cw = v->char_width;
    struct At {
        uint64_t cnt, moff, len, ooff;
    };
    std::vector<uint32_t> counts;
    std::vector<uint64_t> moff, lens, local;
    bool room = true; // the output so far fits the caller's buffer
    rc = for_packed_chunks(
        v, 8 + 4 + 8 + 8 + 8, 1, who,
        [&](Slab &lay, uint64_t nr) {
            const uint64_t cnt = lay.add(nr * 4), mo = lay.add((nr + 1) * 8), len = lay.add(nr * 8);
            return At{cnt, mo, len, lay.add((nr + 1) * 8)};
        },
        [&](const needle_packed_view &dv, const ChunkOut &out, uint64_t r0, const At &o) {
            const uint64_t nr = dv.n_rows;
            int rc = needle_count_matches_packed_dev(p, &dv, (uint32_t *)(out.d + o.cnt), nullptr);
            moff.assign(nr + 1, 0);
            if (rc || (rc = csr_offsets(out, o.cnt, 0, nr, counts, moff.data()))) return rc;
            uint64_t *d_moff = (uint64_t *)(out.d + o.moff), *d_len = (uint64_t *)(out.d + o.len), *d_ooff = (uint64_t *)(out.d + o.ooff);
            const std::vector<RowRange> ranges = csr_ranges(moff.data(), 0, nr, std::max<uint64_t>(host_result_bytes() / 8, 1));
            uint64_t biggest = 0;
            for (const RowRange &rg : ranges) biggest = std::max<uint64_t>(biggest, moff[rg.second] - moff[rg.first]);
            Slab lay;
            const uint64_t o_s = lay.add(biggest * 4), o_e = lay.add(biggest * 4), o_m = set ? lay.add(biggest * 4) : 0;
            DevSlab list;
            hipError_t e = list.alloc(lay.total());
            if (e != hipSuccess) return hip_fail(e, "replace_all_packed_host matches");
            int32_t *d_s = (int32_t *)(list.d + o_s), *d_e = (int32_t *)(list.d + o_e);
            uint32_t *d_m = (uint32_t *)(list.d + o_m); // (each match's member mask: the choice)
            for (const RowRange &rg : ranges) {
                const uint64_t a = rg.first, sn = rg.second - rg.first;
                local.resize(sn + 1);
                for (uint64_t r = 0; r <= sn; ++r) local[r] = moff[a + r] - moff[a];
                HIP_TRY(hipMemcpy(d_moff, local.data(), (sn + 1) * 8, hipMemcpyHostToDevice));
                needle_packed_view sv = dv;
                sv.offsets = dv.offsets + a;
                sv.n_rows = sn;
                int more = 0;
                if (local[sn] && (rc = needle_find_all_csr_packed_dev(p, &sv, d_moff, d_s, d_e, &more, nullptr))) return rc;
                if (more) return fail(NEEDLE_ERR_DEVICE, "replace_all_packed_host: count pass and fill pass disagree");
                if (set && local[sn] && (rc = needle_set_matches_spans_packed_dev(set, &sv, d_moff, d_s, d_e, d_m, nullptr))) return rc;
                rc = set ? needle_replace_each_lengths_packed_dev(&sv, d_moff, d_s, d_e, d_m, NEEDLE_CHOICE_LOWEST_BIT, repl_offsets, n_repl, d_len, nullptr)
                         : needle_replace_all_lengths_packed_dev(&sv, d_moff, d_s, d_e, repl_len, d_len, nullptr);
                if (rc) return rc;
                lens.resize(sn);
                if ((rc = out.download(lens.data(), o.len, sn * 8))) return rc;
                uint64_t *oo = out_offsets + r0 + a;
                for (uint64_t r = 0; r < sn; ++r) oo[r + 1] = oo[r] + lens[r];
                if (!room || oo[sn] > capacity) {
                    room = false;
                    continue;
                }
                const std::vector<RowRange> pieces = csr_ranges(out_offsets, r0 + a, r0 + a + sn, std::max<uint64_t>(host_result_bytes() / cw, 1));
                uint64_t most = 0;
                for (const RowRange &pc : pieces) most = std::max<uint64_t>(most, out_offsets[pc.second] - out_offsets[pc.first]);
                DevSlab text;
                if ((e = text.alloc(most * cw)) != hipSuccess) return hip_fail(e, "replace_all_packed_host text");
                for (const RowRange &pc : pieces) {
                    const uint64_t x = pc.first - r0, pn = pc.second - pc.first, units = out_offsets[pc.second] - out_offsets[pc.first];
                    if (!units) continue;
                    local.resize(pn + 1);
                    for (uint64_t r = 0; r <= pn; ++r) local[r] = out_offsets[pc.first + r] - out_offsets[pc.first];
                    HIP_TRY(hipMemcpy(d_ooff, local.data(), (pn + 1) * 8, hipMemcpyHostToDevice));
                    needle_packed_view tv = dv;
                    tv.offsets = dv.offsets + x;
                    tv.n_rows = pn;
                    rc = set ? needle_replace_each_fill_packed_dev(&tv, d_moff + (x - a), d_s, d_e, d_m, NEEDLE_CHOICE_LOWEST_BIT, repl, repl_offsets, n_repl,
                                                                   d_ooff, text.d, nullptr)
                             : needle_replace_all_fill_packed_dev(&tv, d_moff + (x - a), d_s, d_e, repl, repl_len, d_ooff, text.d, nullptr);
                    if (rc) return rc;
                    e = hipMemcpy((uint8_t *)out_data + out_offsets[pc.first] * cw, text.d, units * cw, hipMemcpyDeviceToHost);
                    if (e != hipSuccess) return hip_fail(e, "replace_all_packed_host download");
                }
            }
            return (int)NEEDLE_OK;
        });
    if (rc == NEEDLE_OK) *total = out_offsets[v->n_rows];
    return rc;
}
extern "C" {

int needle_replace_all_packed_host(const needle_pattern *p, const needle_packed_view *v, const void *repl, uint32_t repl_len, uint64_t *out_offsets,
                                   void *out_data, uint64_t capacity, uint64_t *total) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (!out_offsets || !total || (capacity && !out_data)) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (repl_len > NEEDLE_REPLACE_MAX_UNITS) return fail(NEEDLE_ERR_INVALID, "replacement longer than NEEDLE_REPLACE_MAX_UNITS code units");
    if (repl_len && !repl) return fail(NEEDLE_ERR_INVALID, "replacement is NULL");
    return replace_packed_host("replace_all_packed_host", p, v, repl, repl_len, nullptr, nullptr, 0, out_offsets, out_data, capacity, total);
}

// Replace each match of `p` by the replacement of the lowest member of `s` that matches it whole; a match no member matches is kept.
int needle_set_replace_each_packed_host(const needle_pattern_set *s, const needle_pattern *p, const needle_packed_view *v, const void *repl,
                                        const uint32_t *repl_offsets, uint32_t n_repl, uint64_t *out_offsets, void *out_data, uint64_t capacity,
                                        uint64_t *total) {
    if (!s) return fail(NEEDLE_ERR_INVALID, "pattern set is NULL");
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (!out_offsets || !total || (capacity && !out_data)) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if (!repl_offsets) return fail(NEEDLE_ERR_INVALID, "replacement offsets is NULL");
    if (n_repl < 1 || n_repl > NEEDLE_REPLACE_MAX_CHOICES) return fail(NEEDLE_ERR_INVALID, "1 .. NEEDLE_REPLACE_MAX_CHOICES replacements");
    if (repl_offsets[0] != 0) return fail(NEEDLE_ERR_INVALID, "replacement offsets must start at 0");
    for (uint32_t i = 0; i < n_repl; ++i)
        if (repl_offsets[i + 1] < repl_offsets[i]) return fail(NEEDLE_ERR_INVALID, "replacement offsets decrease");
    if (repl_offsets[n_repl] > NEEDLE_REPLACE_MAX_UNITS)
        return fail(NEEDLE_ERR_INVALID, "replacement table longer than NEEDLE_REPLACE_MAX_UNITS code units");
    if (repl_offsets[n_repl] && !repl) return fail(NEEDLE_ERR_INVALID, "replacement table is NULL");
    if (n_repl != set_pattern_count(s)) return fail(NEEDLE_ERR_INVALID, "one replacement per member of the set");
    if (v->n_rows && (rc = set_plan_usable(s, OP_MATCHES, (int)v->char_width))) return rc;
    return replace_packed_host("set_replace_each_packed_host", p, v, repl, 0, s, repl_offsets, n_repl, out_offsets, out_data, capacity, total);
}

// Every match (NEEDLE_GATHER_MATCHES) or every piece between the matches (NEEDLE_GATHER_PIECES) of a packed HOST batch as the rows of a
// new packed batch.  Per chunk of rows (20 bytes per row: offset, count, match offset): upload, count pass, prefix sum here; then in
// sub-ranges of at most NEEDLE_HOST_RESULT_BYTES of matches: CSR fill, the split list (pieces), lengths, prefix sum here into the caller's
// out_offsets, and -- while both of the caller's buffers have room -- gather and download.  A sub-range's output is at most its rows' text
// (the matches are disjoint, the pieces their complement): the chunk budget bounds it.
int needle_gather_matches_packed_host(const needle_pattern *p, const needle_packed_view *v, int mode, uint64_t *span_offsets, uint64_t *out_offsets,
                                      uint64_t span_capacity, void *out_data, uint64_t unit_capacity, uint64_t *total_spans, uint64_t *total_units) {
    const char *who = "gather_matches_packed_host";
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_packed(v);
    if (rc) return rc;
    if (mode != NEEDLE_GATHER_MATCHES && mode != NEEDLE_GATHER_PIECES)
        return fail(NEEDLE_ERR_INVALID, "mode is neither NEEDLE_GATHER_MATCHES nor NEEDLE_GATHER_PIECES");
    if (!span_offsets || !total_spans || !total_units || (span_capacity && !out_offsets) || (unit_capacity && !out_data))
        return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    span_offsets[0] = 0;
    if (out_offsets) out_offsets[0] = 0;
    *total_spans = *total_units = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if ((rc = check_packed_rows(v, ~0ull, ""))) return rc;
    const uint64_t cw = v->char_width;
    const bool pieces = mode == NEEDLE_GATHER_PIECES;
    struct At {
        uint64_t cnt, moff;
    };
    std::vector<uint32_t> counts;
    std::vector<uint64_t> moff, lens, local;
    uint64_t spans = 0, units = 0; // the output rows and code units so far
    rc = for_packed_chunks(
        v, 8 + 4 + 8, 1, who,
        [&](Slab &lay, uint64_t nr) {
            const uint64_t cnt = lay.add(nr * 4);
            return At{cnt, lay.add((nr + 1) * 8)};
        },
        [&](const needle_packed_view &dv, const ChunkOut &out, uint64_t r0, const At &o) {
            const uint64_t nr = dv.n_rows;
            int rc = needle_count_matches_packed_dev(p, &dv, (uint32_t *)(out.d + o.cnt), nullptr);
            moff.assign(nr + 1, 0);
            if (rc || (rc = csr_offsets(out, o.cnt, 0, nr, counts, moff.data()))) return rc;
            for (uint64_t r = 0; r < nr; ++r) span_offsets[r0 + r + 1] = span_offsets[r0 + r] + (moff[r + 1] - moff[r]) + (pieces ? 1 : 0);
            uint64_t *d_moff = (uint64_t *)(out.d + o.moff);
            const std::vector<RowRange> ranges = csr_ranges(moff.data(), 0, nr, std::max<uint64_t>(host_result_bytes() / 8, 1));
            uint64_t big_m = 0, big_l = 0, big_r = 0; // the most matches, list entries and rows of a sub-range
            for (const RowRange &rg : ranges) {
                const uint64_t nm = moff[rg.second] - moff[rg.first], sn = rg.second - rg.first;
                big_m = std::max(big_m, nm), big_l = std::max(big_l, pieces ? nm + sn : nm), big_r = std::max(big_r, sn);
            }
            Slab lay;
            const uint64_t o_s = lay.add(big_m * 4), o_e = lay.add(big_m * 4), o_po = lay.add(pieces ? (big_r + 1) * 8 : 0);
            const uint64_t o_ps = lay.add(pieces ? big_l * 4 : 0), o_pe = lay.add(pieces ? big_l * 4 : 0), o_len = lay.add((big_l + 1) * 8);
            DevSlab list;
            hipError_t e = list.alloc(lay.total());
            if (e != hipSuccess) return hip_fail(e, "gather_matches_packed_host lists");
            int32_t *d_s = (int32_t *)(list.d + o_s), *d_e = (int32_t *)(list.d + o_e);
            for (const RowRange &rg : ranges) {
                const uint64_t a = rg.first, sn = rg.second - rg.first, nm = moff[rg.second] - moff[a], nl = pieces ? nm + sn : nm;
                spans += nl;
                if (!nl) continue;
                local.resize(sn + 1);
                for (uint64_t r = 0; r <= sn; ++r) local[r] = moff[a + r] - moff[a];
                HIP_TRY(hipMemcpy(d_moff, local.data(), (sn + 1) * 8, hipMemcpyHostToDevice));
                needle_packed_view sv = dv;
                sv.offsets = dv.offsets + a;
                sv.n_rows = sn;
                int more = 0;
                if (nm && (rc = needle_find_all_csr_packed_dev(p, &sv, d_moff, d_s, d_e, &more, nullptr))) return rc;
                if (more) return fail(NEEDLE_ERR_DEVICE, "gather_matches_packed_host: count pass and fill pass disagree");
                const uint64_t *d_lo = d_moff; // the list that is gathered
                const int32_t *d_ls = d_s, *d_le = d_e;
                if (pieces) {
                    uint64_t *d_po = (uint64_t *)(list.d + o_po);
                    int32_t *d_ps = (int32_t *)(list.d + o_ps), *d_pe = (int32_t *)(list.d + o_pe);
                    if ((rc = needle_split_spans_packed_dev(&sv, d_moff, nm ? d_s : nullptr, nm ? d_e : nullptr, d_po, d_ps, d_pe, nullptr))) return rc;
                    d_lo = d_po, d_ls = d_ps, d_le = d_pe;
                }
                uint64_t *d_len = (uint64_t *)(list.d + o_len);
                if ((rc = needle_gather_spans_lengths_packed_dev(&sv, d_lo, d_ls, d_le, d_len, nullptr))) return rc;
                lens.resize(nl + 1);
                e = hipMemcpy(lens.data(), d_len, nl * 8, hipMemcpyDeviceToHost);
                if (e != hipSuccess) return hip_fail(e, "gather_matches_packed_host lengths");
                uint64_t sum = 0; // lens becomes the sub-range's own exclusive prefix sum
                for (uint64_t m = 0; m < nl; ++m) {
                    const uint64_t l = lens[m];
                    lens[m] = sum;
                    sum += l;
                }
                lens[nl] = sum;
                const uint64_t span0 = spans - nl, unit0 = units;
                units += sum;
                if (spans > span_capacity) continue;
                for (uint64_t m = 1; m <= nl; ++m) out_offsets[span0 + m] = unit0 + lens[m];
                if (units > unit_capacity || !sum) continue;
                DevSlab text;
                if ((e = text.alloc(sum * cw)) != hipSuccess) return hip_fail(e, "gather_matches_packed_host text");
                HIP_TRY(hipMemcpy(d_len, lens.data(), (nl + 1) * 8, hipMemcpyHostToDevice));
                if ((rc = needle_gather_spans_fill_packed_dev(&sv, d_lo, d_ls, d_le, d_len, text.d, nullptr))) return rc;
                e = hipMemcpy((uint8_t *)out_data + unit0 * cw, text.d, sum * cw, hipMemcpyDeviceToHost);
                if (e != hipSuccess) return hip_fail(e, "gather_matches_packed_host download");
            }
            return (int)NEEDLE_OK;
        });
    if (rc == NEEDLE_OK) *total_spans = spans, *total_units = units;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// UTF-8 packed host rows: transcoded on the device, byte positions back
// ------------------------------------------------------------------------------------------------
} // extern "C"

// A packed HOST batch of UTF-8 rows (checked): chunks of whole 64-row groups (every chunk owns whole bitmap words) of at most
// NEEDLE_HOST_CHUNK_BYTES of UTF-8 text + kUtf8RowBytes per row; ONE device buffer (utf8_chunk, as large as the largest chunk needs).  Per
// chunk: upload, lengths, the units and both bitmaps downloaded (which synchronises), the malformed words into the caller's bitmap.  Then
// run(dv8, dv16, out, r0, at): dv8 is the chunk as it lies; dv16 its UTF-16 form -- prefix sum here, fill -- or NULL when no row of the
// chunk holds a byte >= 0x80: Latin-1 and UTF-8 agree on ASCII, the 8-bit entries serve and positions are the identity.
template <class Run>
static int for_utf8_chunks(const needle_packed_view *v, const char *who, uint64_t *malformed, Run &&run) {
    const std::vector<RowRange> chunks = packed_chunks(v->offsets, v->n_rows, 1, kUtf8RowBytes, 64, host_chunk_bytes());
    uint64_t all = 0;
    for (const RowRange &c : chunks) {
        Slab lay;
        utf8_chunk(lay, c.second - c.first, v->offsets[c.second] - v->offsets[c.first]);
        all = std::max(all, lay.total());
    }
    DevSlab dev;
    HIP_TRY(dev.alloc(all));
    std::vector<uint64_t> local, lens, words;
    for (const RowRange &c : chunks) {
        const uint64_t r0 = c.first, nr = c.second - c.first, nw = (nr + 63) / 64;
        Slab lay;
        const Utf8Chunk at = utf8_chunk(lay, nr, v->offsets[c.second] - v->offsets[r0]);
        needle_packed_view dv8;
        const hipError_t e = upload_packed_chunk(v, r0, c.second, dev.d + at.data, (uint64_t *)(dev.d + at.off), local, &dv8);
        if (e != hipSuccess) return hip_fail(e, (std::string(who) + " upload").c_str());
        const ChunkOut out{dev.d, who};
        int rc = needle_utf16_lengths_from_utf8_packed_dev(&dv8, (uint64_t *)(dev.d + at.len), (uint64_t *)(dev.d + at.non_ascii),
                                                           (uint64_t *)(dev.d + at.malformed), nullptr);
        words.resize(nw);
        if (rc || (malformed && (rc = out.download(malformed + r0 / 64, at.malformed, nw * 8))) || (rc = out.download(words.data(), at.non_ascii, nw * 8)))
            return rc;
        bool ascii = true;
        for (uint64_t w : words) ascii = ascii && w == 0;
        needle_packed_view dv16{dev.d + at.u16, 2, nr, (const uint64_t *)(dev.d + at.uoff)};
        if (!ascii) {
            lens.resize(nr + 1);
            if ((rc = out.download(lens.data() + 1, at.len, nr * 8))) return rc;
            lens[0] = 0;
            for (uint64_t r = 1; r <= nr; ++r) lens[r] += lens[r - 1];
            HIP_TRY(hipMemcpy(dev.d + at.uoff, lens.data(), (nr + 1) * 8, hipMemcpyHostToDevice));
            if ((rc = needle_utf16_from_utf8_packed_dev(&dv8, dv16.offsets, (uint16_t *)(dev.d + at.u16), nullptr))) return rc;
        }
        if ((rc = run(dv8, ascii ? nullptr : &dv16, out, r0, at))) return rc;
    }
    return NEEDLE_OK;
}

static int check_utf8_host(const needle_pattern *p, const needle_packed_view *v) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    if (!v) return fail(NEEDLE_ERR_INVALID, "packed view is NULL");
    if (v->char_width != 1) return fail(NEEDLE_ERR_INVALID, "UTF-8 rows are a packed view of char_width 1");
    if (!v->offsets) return fail(NEEDLE_ERR_INVALID, "offsets is NULL");
    return NEEDLE_OK;
}

extern "C" {

int needle_contained_in_utf8_packed_host(const needle_pattern *p, const needle_packed_view *v, uint64_t *bitmap, uint64_t *malformed) {
    int rc = check_utf8_host(p, v);
    if (rc) return rc;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!bitmap) return fail(NEEDLE_ERR_INVALID, "bitmap is NULL");
    if ((rc = check_packed_rows(v, 0x7FFFFFFFull, "rows of at most 2^31 - 1 bytes"))) return rc;
    return for_utf8_chunks(v, "contained_in_utf8_packed_host", malformed,
                           [&](const needle_packed_view &dv8, const needle_packed_view *dv16, const ChunkOut &out, uint64_t r0, const Utf8Chunk &at) {
                               const int rc = needle_contained_in_packed_dev(p, dv16 ? dv16 : &dv8, (uint64_t *)(out.d + at.bitmap), nullptr);
                               return rc ? rc : out.download(bitmap + r0 / 64, at.bitmap, (dv8.n_rows + 63) / 64 * 8);
                           });
}

// (per chunk, behind the transcoding: count pass, prefix sum here, fill pass in sub-ranges of at most NEEDLE_HOST_RESULT_BYTES of results
// -- needle_find_all_csr_packed_host's -- with the positions kernel on start and on end, in place, before the sub-range's download)
int needle_find_all_csr_utf8_packed_host(const needle_pattern *p, const needle_packed_view *v, uint64_t *offsets, int32_t *byte_start,
                                         int32_t *byte_end, uint64_t capacity, uint64_t *total, uint64_t *malformed) {
    const char *who = "find_all_csr_utf8_packed_host";
    int rc = check_utf8_host(p, v);
    if (rc) return rc;
    if (!offsets || !total || (capacity && (!byte_start || !byte_end))) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    offsets[0] = 0;
    *total = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if ((rc = check_packed_rows(v, 0x7FFFFFFFull, "rows of at most 2^31 - 1 bytes"))) return rc;
    std::vector<uint32_t> counts;
    rc = for_utf8_chunks(v, who, malformed, [&](const needle_packed_view &dv8, const needle_packed_view *dv16, const ChunkOut &out, uint64_t r0, const Utf8Chunk &at) {
        const needle_packed_view &tv = dv16 ? *dv16 : dv8; // the text the pattern scans
        const uint64_t r1 = r0 + dv8.n_rows;
        int rc = needle_count_matches_packed_dev(p, &tv, (uint32_t *)(out.d + at.cnt), nullptr);
        if (rc || (rc = csr_offsets(out, at.cnt, r0, dv8.n_rows, counts, offsets))) return rc;
        if (offsets[r1] == offsets[r0] || offsets[r1] > capacity) return (int)NEEDLE_OK;
        return csr_fill_pass(who, offsets, r0, r1, out.d + at.csr, byte_start, byte_end,
                             [&](uint64_t a, uint64_t sn, const uint64_t *d_csr, int32_t *d_s, int32_t *d_e, int *more) {
                                 needle_packed_view sv = tv, s8 = dv8;
                                 sv.offsets = tv.offsets + (a - r0), s8.offsets = dv8.offsets + (a - r0);
                                 sv.n_rows = s8.n_rows = sn;
                                 int rc = needle_find_all_csr_packed_dev(p, &sv, d_csr, d_s, d_e, more, nullptr);
                                 if (rc || !dv16) return rc;
                                 if ((rc = needle_utf8_positions_packed_dev(&s8, d_csr, d_s, d_s, nullptr))) return rc;
                                 return needle_utf8_positions_packed_dev(&s8, d_csr, d_e, d_e, nullptr);
                             });
    });
    if (rc == NEEDLE_OK) *total = offsets[v->n_rows];
    return rc;
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// find() of fixed-stride host rows in its smaller result forms
// ------------------------------------------------------------------------------------------------
// needle_find_packed{16,8}_host: needle_find_host with start / end as ONE dword (elem 4: low half start, high half end, 0xFFFF = no match;
// rows of at most 65 534 chars) or ONE uint16 (elem 2: start | (end - start) << 8 -- pack8 of needle_device.h, stored by the scan kernel
// itself; rows of at most 256 chars) per row: 4 or 2 bytes per row over PCIe instead of 8.
template <class T>
static int find_packed_host(const needle_pattern *p, const needle_batch_view *v, uint64_t *bitmap, T *res, uint32_t limit, const char *beyond,
                            int (*dev_entry)(const needle_pattern *, const needle_batch_view *, uint64_t *, T *, void *)) {
    if (!p) return fail(NEEDLE_ERR_INVALID, "pattern is NULL");
    int rc = check_host_view(v);
    if (rc) return rc;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!bitmap || !res) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if ((v->lengths ? v->row_stride : v->row_len) > limit) return fail(NEEDLE_ERR_UNSUPPORTED, beyond); // the caller's own stride: the upload pads it to 16 bytes
    return for_fixed_chunks(
        v, 0, "find", [&](Slab &lay, uint64_t n) { return scan_sections(lay, n, n * sizeof(T)); },
        [&](const needle_batch_view &dv, const ChunkOut &out, uint64_t r0, const ScanAt &o) {
            const int rc = dev_entry(p, &dv, (uint64_t *)(out.d + o.bm), (T *)(out.d + o.s), nullptr);
            return rc ? rc : download_scan(out, o, dv.n_rows, dv.n_rows * sizeof(T), bitmap + r0 / 64, res + r0, nullptr);
        });
}

extern "C" {

int needle_find_packed16_host(const needle_pattern *p, const needle_batch_view *v, uint64_t *bitmap, uint32_t *start_end16) {
    return find_packed_host(p, v, bitmap, start_end16, 65534u, "16-bit offsets: rows of at most 65 534 chars (use needle_find_host)", needle_find_packed16_dev);
}
int needle_find_packed8_host(const needle_pattern *p, const needle_batch_view *v, uint64_t *bitmap, uint16_t *start_len8) {
    return find_packed_host(p, v, bitmap, start_len8, 256u, "8-bit start / length: rows of at most 256 chars (use needle_find_packed16_host)",
                            needle_find_packed8_dev);
}

// Host batch -> bitmap + the matched rows' records: what crosses PCIe on the way back is 1 bit per row + 8 bytes per
// MATCHED row (needle_find_host: 8 bytes per row).  *n_matched is the total; at most cap records are written.
int needle_find_compact_host(const needle_pattern *p, const needle_batch_view *v, uint64_t *bitmap, needle_match_rec *recs, uint64_t cap,
                             uint64_t *n_matched) {
    if (!p || !n_matched) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    int rc = check_host_view(v);
    if (rc) return rc;
    *n_matched = 0;
    if (v->n_rows == 0) return NEEDLE_OK;
    if (!bitmap || (cap && !recs)) return fail(NEEDLE_ERR_INVALID, "output buffer is NULL");
    if ((v->lengths ? v->row_stride : v->row_len) > 65534u) // the caller's own stride: the upload pads it to 16 bytes
        return fail(NEEDLE_ERR_UNSUPPORTED, "the compact records hold 16-bit offsets: rows of at most 65 534 chars (use needle_find_host)");
    struct At {
        uint64_t bm, n, rec, room; // (room: the records this chunk may still write)
    };
    return for_fixed_chunks(
        v, 0, "compact find",
        [&](Slab &lay, uint64_t n) {
            const uint64_t room = cap > *n_matched ? std::min<uint64_t>(cap - *n_matched, n) : 0, bm = lay.add((n + 63) / 64 * 8), cnt = lay.add(16);
            return At{bm, cnt, lay.add(room * sizeof(needle_match_rec)), room};
        },
        [&](const needle_batch_view &dv, const ChunkOut &out, uint64_t r0, const At &o) {
            int rc = find_compact(p, &dv, (uint64_t *)(out.d + o.bm), (needle_match_rec *)(out.d + o.rec), o.room, (uint64_t *)(out.d + o.n), r0, nullptr);
            uint64_t m = 0;
            if (rc || (rc = out.download(&m, o.n, 8))) return rc; // (synchronises with the kernels on the null stream)
            if ((rc = out.download(bitmap + r0 / 64, o.bm, (dv.n_rows + 63) / 64 * 8))) return rc;
            if ((rc = out.download(recs + *n_matched, o.rec, std::min(m, o.room) * sizeof(needle_match_rec)))) return rc;
            *n_matched += m;
            return (int)NEEDLE_OK;
        });
}

} // extern "C"

// ------------------------------------------------------------------------------------------------
// Matcher mirror: fields as the generated class declares them (DFAClassBuilder.addFields :688-699); the
// constructor leaves them at the JVM default 0 (the generated <init> only stores string and length).
struct needle_matcher {
    const needle_pattern *p;
    std::vector<uint16_t> s;
    int next_start = 0, start = 0, end = 0;
};

static int one_row(const needle_matcher *m, int op, int from, int *matched, int *st, int *en) {
    const size_t n = m->s.size() - (size_t)from;
    needle_batch_view v;
    memset(&v, 0, sizeof(v));
    v.rows = n ? (const void *)(m->s.data() + from) : (const void *)&v; // never read when n == 0
    v.char_width = 2;
    v.n_rows = 1;
    v.row_stride = n;
    v.row_len = (uint32_t)n;
    uint64_t bm = 0;
    int32_t s32 = -1, e32 = -1;
    int rc = run_host(m->p, op, &v, &bm, &s32, &e32);
    if (rc) return rc;
    *matched = (int)(bm & 1);
    if (st) *st = s32;
    if (en) *en = e32;
    return NEEDLE_OK;
}

extern "C" {

int needle_matcher_create(const needle_pattern *p, const uint16_t *s, size_t n, needle_matcher **out) {
    if (!p || !out || (!s && n)) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    needle_matcher *m = new needle_matcher();
    m->p = p;
    m->s.assign(s, s + n);
    *out = m;
    return NEEDLE_OK;
}

void needle_matcher_destroy(needle_matcher *m) { delete m; }

int needle_matcher_matches(needle_matcher *m, int *r) {
    if (!m || !r) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    return one_row(m, OP_MATCHES, 0, r, nullptr, nullptr);
}

int needle_matcher_contained_in(needle_matcher *m, int *r) {
    if (!m || !r) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    return one_row(m, OP_CONTAINED_IN, 0, r, nullptr, nullptr);
}

// find(FROM, TO): DFAClassBuilder.createFindMethodInternal :625-659.  TO is ignored by the generated
// indexForwards (its slot is overwritten with this.length, DFAMethodComponents.java:19-21).
int needle_matcher_find_range(needle_matcher *m, int from, int to, int *r) {
    (void)to;
    if (!m || !r) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    *r = 0;
    if (m->next_start == -1) return NEEDLE_OK; // :629-630
    const int length = (int)m->s.size();
    const MatcherRoots t = matcher_roots(m->p);
    int index;
    int st = 0;
    bool have_start = false;
    if (from < 0) return fail(NEEDLE_ERR_INVALID, "from < 0 (StringIndexOutOfBoundsException in the reference)");
    if (from >= length) {
        // both generated loops are skipped: indexForwards returns its initial lastMatch (:355-356,468)
        index = t.forwards_root_accepts ? 0 : -1;
    } else {
        int matched = 0, s32 = -1, e32 = -1;
        int rc = one_row(m, OP_FIND, from, &matched, &s32, &e32);
        if (rc) return rc;
        if (matched) {
            index = e32 + from;
            st = s32 + from; // the backward walk is bounded by FROM (:651-652) == index 0 of the sub-row
            have_start = true;
        } else {
            index = -1;
        }
    }
    m->end = index;
    m->next_start = index;
    if (index == -1) return NEEDLE_OK;
    if (!have_start) {
        // index came from the literal 0 above; start as the reference computes it with an empty walk
        if (t.fixed_len >= 0) st = index - t.fixed_len;
        else st = t.backwards_root_accepts ? from : 0x7FFFFFFF; // :543-547 with index-1 < FROM
    }
    m->start = st;
    *r = 1;
    return NEEDLE_OK;
}

int needle_matcher_find(needle_matcher *m, int *r) {
    if (!m) return fail(NEEDLE_ERR_INVALID, "NULL argument");
    return needle_matcher_find_range(m, m->next_start, (int)m->s.size(), r); // :616-623
}

int needle_matcher_start(const needle_matcher *m) { return m ? m->start : -1; }
int needle_matcher_end(const needle_matcher *m) { return m ? m->end : -1; }

} // extern "C"
