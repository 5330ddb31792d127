// needle_find_all.hip -- every non-overlapping match of every row in ONE pass over a batch of fixed-stride rows (SURVEY.md s8f-1:
// the reference's repeated Matcher.find(), DFAClassBuilder.java:616-659; DFACompilerTest.java:66-78,671-699).
//
// The round-per-match form (needle_find_next_dev fed its own `end` as the next cursor) reads the whole batch once per
// round: a keyword dictionary over text finds a handful of matches per row and up to a few dozen in the worst row of
// ten million, so the batch crosses the HBM bus dozens of times.  Here a row is fetched once.
//
// Staging: the scan kernel's (needle_scan.h) -- one row per lane, 64-row groups, whole lines HBM -> VGPRs -> XOR-swizzled LDS
// tile, the lowered automaton staged once per workgroup.  The walk is needle_find_all_walk.h's: the rows of a wave stop being at
// the same char after their first match, so every lane keeps its own PIECE index (16-byte piece of its row) and walk_tile
// iterates "each live lane walks its current piece" -- a ds_read_b128 at a per-lane tile address, then find_all_lane_step.  A lane
// that restarts steps back to the piece holding its cursor (from memory, in the rare case it is in the previous tile); lanes
// that reached the tile's end wait there for the others.
//
// Results: dense per-row slots (needle_find_all_dev), or compact filing at caller-computed offsets after a counting
// pass of the same kernel that files nothing (needle_count_matches_dev / needle_find_all_csr_dev).
#include "needle_find_all_walk.h"
#include "needle_launch.h"

namespace needle {

// The fixed-stride rows of find_all_kernel as needle_find_all_walk.h's Rows policy: rows start on a 16-byte block (skip 0); results go
// to two arrays, or to one dword per match (fa.packed), consecutive per row or group-blocked (fa.kshift); text: the lane's tile row.
template <int CW, int CHB>
struct StrideRows {
    const FindAllArgs &fa;
    const uint8_t *const rowp;           // the lane's row in memory
    const uint32_t row_addr, swz16;      // byte b of the lane's tile row is at row_addr + (b ^ swz16)
    const uint32_t tile_b0;              // first row byte of the tile in LDS
    static constexpr uint32_t skip = 0u;
    __device__ __forceinline__ uint64_t at(uint64_t out0, uint32_t k) const { return out0 + ((uint64_t)k << fa.kshift); }
    __device__ __forceinline__ void file_match(uint64_t out0, uint32_t k, int32_t s, int32_t en) const {
        if (fa.packed) fa.packed[at(out0, k)] = (uint32_t)s | ((uint32_t)en << 16);
        else fa.starts[at(out0, k)] = s, fa.ends[at(out0, k)] = en;
    }
    __device__ __forceinline__ void file_end(uint64_t out0, uint32_t k, int32_t en) const {
        if (fa.packed) fa.packed[at(out0, k)] = (uint32_t)en << 16;
        else fa.ends[at(out0, k)] = en;
    }
    __device__ __forceinline__ int32_t read_end(uint64_t out0, uint32_t k) const {
        if (fa.packed) return (int32_t)(__hip_atomic_load(&fa.packed[at(out0, k)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 16);
        return __hip_atomic_load(&fa.ends[at(out0, k)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void file_start(uint64_t out0, uint32_t k, int32_t s, int32_t en) const {
        if (fa.packed) fa.packed[at(out0, k)] = (uint32_t)s | ((uint32_t)en << 16);
        else fa.starts[at(out0, k)] = s;
    }
    __device__ __forceinline__ int32_t backward(bool act, int32_t en, int32_t bound) const {
        return backward_walk<CW, true>(fa.s, act, en, bound, row_addr, tile_b0, (uint32_t)CHB, swz16, rowp);
    }
    // (the owner's skip stays a literal 0: find_all_starts_phase's "- skip" must fold away here as rows.skip does in the lane step)
    __device__ __forceinline__ FindAllOwner owner(uint64_t grp, uint32_t l) const { return {fa.s.rows + ((grp << 6) + l) * fa.s.stride_bytes, 0u}; }
    static __device__ __forceinline__ bool no_text(int32_t) { return false; }
    __device__ __forceinline__ uint32_t slot_addr() const { return row_addr; }
};

// LM: the "lengths" form (fa.lmode) of a program with skip states
template <int CW, int MODE, int CHB, bool LM>
__global__ __launch_bounds__(kWavesPerBlock * 64) void find_all_kernel(const FindAllArgs fa) {
    using G = Geom<CHB>;
    const ScanArgs &a = fa.s;
    constexpr int CPP = 16 / CW; // chars per 16-byte piece
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_waves = blockDim.x >> 6;

    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();
    for (uint32_t i = tid * 16u; i < a.hdr.lds_bytes; i += blockDim.x * 16u)
        *(u32x4 *)(smem + i) = *(const u32x4 *)(a.prog + i);
    __syncthreads();

    FindAllWalk fw;
    find_all_walk_setup<CW, MODE>(a, lane, fw);

    Tile tile;
    {
        const uint32_t base = ((a.hdr.lds_bytes + 15u) & ~15u) + (uint32_t)wave * G::kTileBytes;
        tile.store_addr = base + (uint32_t)(lane / G::kPieces) * CHB + (uint32_t)(lane % G::kPieces) * 16u;
        tile.store_step = G::kRowsPerInstr * CHB;
        tile.row_addr = base + (uint32_t)lane * CHB;
    }
    const uint32_t swz16 = (uint32_t)G::swz(lane) << 4; // byte b of this lane's tile row is at row_addr + (b ^ swz16)

    const uint64_t n_groups = (a.n_rows + 63) >> 6;
    const uint64_t wave_cnt = (uint64_t)gridDim.x * n_waves;
    uint64_t g = (uint64_t)blockIdx.x * n_waves + wave;
    if (g >= n_groups) return;

    // tile fetch: as in scan_kernel (needle_scan.h) -- a fetch unit is one 128-byte line per row: one tile of 128-byte
    // pieces or the two 64-byte tiles of the same lines, requested back to back
    const uint32_t q = (uint32_t)lane >> 4;
    const uint32_t p_in_row = (uint32_t)(lane % G::kPieces);
    const uint32_t row_in_instr = (uint32_t)(lane / G::kPieces);
    const uint32_t o_even = row_in_instr * (uint32_t)a.stride_bytes + 16u * (p_in_row ^ q);
    const uint32_t o_odd = CHB == 128 ? (row_in_instr * (uint32_t)a.stride_bytes + 16u * (p_in_row ^ q ^ 4u)) : o_even;
    const uint64_t load_step = (uint64_t)G::kRowsPerInstr * a.stride_bytes;
    constexpr int NT = (CHB == 64) ? 2 : 1;
    u32x4 R[NT][G::kInstrs];
    auto fetch = [&](uint64_t grp, uint32_t unit) __attribute__((always_inline)) {
        const uint8_t *base = a.rows + (grp << 6) * a.stride_bytes + unit * (NT * CHB);
#pragma unroll
        for (int j = 0; j < G::kInstrs; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) R[t][j] = load_row16<NT == 1>(base + t * CHB + j * load_step + ((j & 1) ? o_odd : o_even));
    };
    auto fetch_clamped = [&](uint64_t grp, uint32_t chunk) __attribute__((always_inline)) {
        const uint32_t last_r = (uint32_t)(a.n_rows - 1 - (grp << 6));
        const uint32_t stride = (uint32_t)a.stride_bytes;
        const uint8_t *gbase = a.rows + (grp << 6) * a.stride_bytes;
#pragma unroll
        for (int j = 0; j < G::kInstrs; ++j) {
            uint32_t r = (uint32_t)(j * G::kRowsPerInstr) + row_in_instr;
            const uint32_t kk = p_in_row ^ (uint32_t)G::swz((int)r);
            r = r < last_r ? r : last_r;
            uint32_t pb = chunk * CHB + kk * 16u;
            if (pb + 16u > stride) pb = stride - 16u;
            R[0][j] = load_row16<false>(gbase + (r * stride + pb));
        }
    };

    // ---- per-group (per-row) state
    uint64_t my_row = 0;
    uint32_t n_chunks = 1;
    bool row_ok = false;
    FindAllRow row = {}; // (row.len: the row's chars)
    row.done = true, row.last = -1;
    const uint8_t *rowp = a.rows;
    auto rows_at = [&](uint32_t tile_b0) __attribute__((always_inline)) { return StrideRows<CW, CHB>{fa, rowp, tile.row_addr, swz16, tile_b0}; };

    auto begin_group = [&](uint64_t grp) __attribute__((always_inline)) {
        my_row = (grp << 6) + lane;
        row_ok = my_row < a.n_rows;
        row.len = 0;
        if (row_ok) row.len = a.lengths ? a.lengths[my_row] : a.row_len;
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(row.len)); // (the tile it is about to stage was requested earlier still)
        const uint32_t max_len = a.lengths ? wave_max(row.len) : a.row_len;
        n_chunks = (max_len * CW + CHB - 1) / CHB;
        if (n_chunks == 0) n_chunks = 1;
        rowp = a.rows + (row_ok ? my_row : 0) * a.stride_bytes;
        row.done = !row_ok;
        row.cursor = 0;
        row.st = fw.start_state;
        row.last = a.hdr.root_accepting ? 0 : -1; // :356 literal 0 (cursor 0: the same whether 0 < length or not)
        row.pi = 0;
        row.count = 0;
        row.out0 = fa.kshift ? (my_row >> 6) * fa.slots * 64u + (my_row & 63u) : my_row * fa.slots;
        row.cap = fa.count_only ? 0xFFFFFFFFu : fa.slots;
        if (fa.offsets) {
            row.out0 = row_ok ? fa.offsets[my_row] : 0;
            row.cap = row_ok ? (uint32_t)(fa.offsets[my_row + 1] - row.out0) : 0u;
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(row.cap)); // (as for len above: no vmcnt wait inside the walk)
        }
    };

    // Walk the tile in LDS (chunk ck of the group's rows) until every live lane is past it.
    auto walk_tile = [&](uint32_t ck) __attribute__((always_inline)) {
        const uint32_t tile_p0 = ck * G::kPieces, tile_p1 = tile_p0 + G::kPieces;
        const auto rows = rows_at(ck * CHB);
        for (;;) {
            const uint32_t p0 = row.pi * CPP;
            const bool beyond = p0 >= row.len; // nothing of the row there (a walk over PAD: the search ends)
            const bool active = !row.done && (row.pi < tile_p1 || beyond);
            if (__ballot(active) == 0ull) break;
            // (straight-line code for all 64 lanes, idle ones included: find_all_lane_step)
            const bool in_lds = active && !beyond && row.pi >= tile_p0;
            u32x4 v = *(const lds_u32x4 *)(uintptr_t)(tile.row_addr + (((in_lds ? row.pi - tile_p0 : 0u) << 4) ^ swz16));
            const bool in_mem = active && !beyond && row.pi < tile_p0;
            if (__ballot(in_mem) != 0ull) { // a restart in the previous tile (rare): waited for HERE, so that the common path
                                            // carries no vmcnt wait (tile prefetch and match stores are in flight)
                if (in_mem) {
                    v = *(const u32x4 *)(rowp + (uint64_t)row.pi * 16u);
                    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v));
                }
            }
            const uint32_t w[4] = {v[0], v[1], v[2], v[3]}; // (a piece beyond the row: whatever is there -- its flags are masked)
            find_all_lane_step<CW, MODE, LM>(fa, fw, rows, w, active, p0, row);
        }
    };
    auto end_group = [&](uint64_t grp) __attribute__((always_inline)) {
        if (row_ok && fa.counts) fa.counts[my_row] = row.count;
        if (fa.defer && !fa.count_only) find_all_starts_phase<CW>(fa, rows_at(0u), lane, grp, row);
    };
    auto stage = [&](auto tc) __attribute__((always_inline)) {
        constexpr int T = decltype(tc)::value;
#pragma unroll
        for (int j = 0; j < G::kInstrs; ++j) store_piece(tile, j, R[T][j]);
    };

    uint64_t last_group = n_groups - 1; // first group handled by the clamped tail below (as in scan_kernel)
    {
        const uint64_t group_bytes = 64 * a.stride_bytes;
        const uint64_t safe = a.total_bytes >= (uint64_t)(NT * CHB) ? (a.total_bytes - NT * CHB) / group_bytes : 0;
        if (safe < last_group) last_group = safe;
    }
    if (g < last_group) {
        fetch(g, 0);
        for (;;) {
            begin_group(g);
            uint32_t ck = 0;
            bool have_next = false; // R holds (or will hold) unit 0 of this wave's next group
            // the registers of a unit are free once its last tile is staged: the next unit -- of this group, or the
            // first one of the wave's next group -- is requested then and arrives while the tile is walked
            auto prefetch = [&]() __attribute__((always_inline)) {
                if (ck + 1 < n_chunks) fetch(g, (ck + 1) / NT);
                else if (g + wave_cnt < last_group) fetch(g + wave_cnt, 0), have_next = true;
            };
            for (;;) {
                stage(std::integral_constant<int, 0>{});
                asm volatile("" ::: "memory");
                if (NT == 1) prefetch();
                asm volatile("" ::: "memory");
                walk_tile(ck);
                ++ck;
                if (ck >= n_chunks || __ballot(!row.done) == 0ull) break;
                if (NT == 2) {
                    stage(std::integral_constant<int, NT - 1>{});
                    asm volatile("" ::: "memory");
                    prefetch();
                    asm volatile("" ::: "memory");
                    walk_tile(ck);
                    ++ck;
                    if (ck >= n_chunks || __ballot(!row.done) == 0ull) break;
                }
            }
            end_group(g);
            g += wave_cnt;
            if (g >= last_group) break;
            if (!have_next) fetch(g, 0);
        }
    }
    for (; g < n_groups; g += wave_cnt) {
        begin_group(g);
        for (uint32_t ck = 0; ck < n_chunks; ++ck) {
            fetch_clamped(g, ck);
            stage(std::integral_constant<int, 0>{});
            walk_tile(ck);
            if (__ballot(!row.done) == 0ull) break;
        }
        end_group(g);
    }
}

// ---- launcher
template <int CW, int MODE, int CHB, bool LM = false>
static hipError_t launch_fa(const FindAllArgs &fa, int grid, int waves, size_t lds, hipStream_t stream) {
    auto k = find_all_kernel<CW, MODE, CHB, LM>;
    static thread_local uint64_t configured = 0;
    if (hipError_t e = allow_full_lds((const void *)k, configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(grid), dim3(waves * 64), lds, stream, fa);
    return hipGetLastError();
}
template <int CW, int MODE>
static hipError_t launch_fa_h(const FindAllArgs &fa, int chb, int grid, int waves, size_t lds, hipStream_t s) {
    if constexpr (MODE == MODE_TABLE8 || MODE == MODE_TABLE16) {
        if (fa.lmode && fa.s.hdr.fa_skip_lo)
            return chb == 128 ? launch_fa<CW, MODE, 128, true>(fa, grid, waves, lds, s) : launch_fa<CW, MODE, 64, true>(fa, grid, waves, lds, s);
    }
    return chb == 128 ? launch_fa<CW, MODE, 128>(fa, grid, waves, lds, s) : launch_fa<CW, MODE, 64>(fa, grid, waves, lds, s);
}
template <int CW>
static hipError_t launch_fa_m(const FindAllArgs &fa, int chb, int grid, int waves, size_t lds, hipStream_t s) {
    switch (fa.s.hdr.mode) {
    case MODE_PACK: return launch_fa_h<CW, MODE_PACK>(fa, chb, grid, waves, lds, s);
    case MODE_TABLE8: return launch_fa_h<CW, MODE_TABLE8>(fa, chb, grid, waves, lds, s);
    case MODE_TABLE16: return launch_fa_h<CW, MODE_TABLE16>(fa, chb, grid, waves, lds, s);
    case MODE_HYBRID: return launch_fa_h<CW, MODE_HYBRID>(fa, chb, grid, waves, lds, s);
    case MODE_GLOBAL: return launch_fa_h<CW, MODE_GLOBAL>(fa, chb, grid, waves, lds, s);
    case MODE_SPARSE: return fa.lmode ? launch_fa_h<CW, MODE_SPARSE>(fa, chb, grid, waves, lds, s) : hipErrorInvalidValue; // (lengths programs only)
    default: return hipErrorInvalidValue; // (pair mode: the caller lowers the automaton without it)
    }
}

// Waves per workgroup x tile (window) bytes per lane of the per-lane find-all kernels, fixed-stride and packed rows alike: the first
// candidate whose tiles fit the 160 KiB of LDS beside the program.  None of them spills (scripts/kernel_resources.py).
static size_t lane_shape_lds(uint32_t prog_lds_bytes, int waves, int chb) { return ((prog_lds_bytes + 15u) & ~15u) + (size_t)waves * 64 * chb; }
static bool lane_shape_fits(uint32_t prog_lds_bytes, int waves, int chb) { return lane_shape_lds(prog_lds_bytes, waves, chb) <= 160u * 1024u; }
bool find_all_lane_shape(uint32_t prog_lds_bytes, int *waves, int *chb) {
    static const int cand[6][2] = {{16, 128}, {12, 128}, {16, 64}, {12, 64}, {8, 64}, {4, 64}};
    for (const auto &c : cand)
        if (lane_shape_fits(prog_lds_bytes, c[0], c[1])) {
            *waves = c[0], *chb = c[1];
            return true;
        }
    return false;
}

// One persistent workgroup per CU; the shape (waves x tile bytes) follows the automaton's LDS footprint.
hipError_t launch_find_all(int char_width, const FindAllArgs &fa, int n_cus, hipStream_t stream) {
    if (fa.s.n_rows == 0) return hipSuccess;
    int waves = 0, chb = 0;
    static const char *force = getenv("NEEDLE_FIND_ALL_SHAPE"); // e.g. "8x128" (tuning experiments only)
    if (force) {
        int w = 0, c = 0;
        if (sscanf(force, "%dx%d", &w, &c) == 2 && (c == 64 || c == 128) && w >= 1 && w <= 16 && lane_shape_fits(fa.s.hdr.lds_bytes, w, c)) waves = w, chb = c;
    }
    if (!waves && !find_all_lane_shape(fa.s.hdr.lds_bytes, &waves, &chb)) return hipErrorInvalidValue;
    const uint64_t n_groups = (fa.s.n_rows + 63) >> 6;
    uint64_t blocks = (n_groups + waves - 1) / waves;
    if (blocks > (uint64_t)n_cus) blocks = (uint64_t)n_cus;
    const size_t lds = lane_shape_lds(fa.s.hdr.lds_bytes, waves, chb);
    return char_width == 1 ? launch_fa_m<1>(fa, chb, (int)blocks, waves, lds, stream) : launch_fa_m<2>(fa, chb, (int)blocks, waves, lds, stream);
}

} // namespace needle
