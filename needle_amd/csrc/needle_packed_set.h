// needle_packed_set.h -- the pattern-set kernel of PACKED row batches: up to 32 patterns answered in one pass, a uint32 mask per row
// (needle_set_matches_packed_dev / needle_set_contained_in_packed_dev), hand-written for gfx950 (CDNA4).  Included by one
// translation unit per char width (needle_packed_set1.hip / needle_packed_set2.hip).
//
// Built on packed_stream / PackedWindow (needle_packed.h) as they are: the same staging, the same "nothing outside the rows' span is
// read", 64 rows per wave.  The program is a product automaton of the set's members (needle_set.h) lowered as a plain LDS table
// (lower_pattern_set): one table lookup per char whatever the number of patterns.  Per lane the state `st` and, for containedIn(),
// the row's mask `m` live across windows in registers.
//
//   matches():      the walk is the per-char code of the single-pattern kernel (walk_piece<OP_MATCHES>); a row is resolved in the
//                   sink (st == 0); its mask is mask[st], read from LDS ONCE, at the row's end.
//   containedIn():  the row's mask is mask[start] | mask[state after every char].  A state with bits is TRANSIENT (the accepting
//                   component returns to its root on the next char), so it has to be noticed per char: the walk keeps
//                   hi = max(hi, st) along the state chain -- one VALU op per char, no LDS read -- and only when hi >= accept_lo
//                   after a 16-byte block is that block walked again from its saved entry state with m |= mask[st] per char.  PRE
//                   and PAD chars are identities of the table: they change neither st nor m (m |= mask[st] of a state whose bits
//                   m holds already).  A row is resolved when m holds every bit of the group.
//
// Results: masks[r] = m (the set's first group) or masks[r] |= m (later groups: one lane per row, launches stream-ordered, no
// atomics) for rows below n_rows.
#pragma once
#include "needle_packed.h"

namespace needle {

// One 16-byte block of one row for containedIn(): w = its four dwords, p0 / rem / skip as walk_piece's.  A lane whose row is decided
// (m holds every bit of the group) is masked out of the block's lookups, as walk_piece masks its finished lanes: the walk is bound by
// LDS cycles, and a row decided in the middle of a window would go on spending them to the window's end.
template <int CW, int MODE, bool GUARD>
__device__ __forceinline__ void set_walk_block(const Walk &wk, const uint32_t (&w)[4], uint32_t p0, uint32_t rem, uint32_t skip, uint32_t accept_lo,
                                               uint32_t mask_off, uint32_t group_mask, uint32_t &st, uint32_t &m) {
    constexpr int CPP = 16 / CW;
    if (NEEDLE_MASK_DONE_LANES && m == group_mask) return;
    uint32_t col[CPP];
    piece_lookups<MODE, CW, GUARD>(wk, w, p0, rem, skip, col);
    const uint32_t st0 = st;
    uint32_t s = st0, hi = 0u;
#pragma unroll
    for (int i = 0; i < CPP; ++i) {
        s = apply<MODE, CW>(wk, s, col[i]);
        hi = s > hi ? s : hi;
    }
    st = s;
    if (hi >= accept_lo) { // (rare: some state of this block has bits -- the mask reads stay off the common path)
        uint32_t t = st0;
#pragma unroll
        for (int i = 0; i < CPP; ++i) {
            t = apply<MODE, CW>(wk, t, col[i]);
            m |= lds_u32(mask_off + t * 4u);
        }
    }
}

template <int OP, int CW, int MODE, int CHB>
__global__ __launch_bounds__(kWavesPerBlock * 64) void packed_set_kernel(const PackedSetArgs sa) {
    static_assert(OP == OP_MATCHES || OP == OP_CONTAINED_IN, "matches() / containedIn() only");
    static_assert(MODE == MODE_TABLE8 || MODE == MODE_TABLE16, "plain table programs only");
    const ScanArgs &a = sa.p.s;
    constexpr uint32_t kWin = 64u * CHB;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_waves = blockDim.x >> 6;

    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem != 0u) __builtin_trap();
    // ---- stage the automaton (column maps, table, masks) in LDS (once per workgroup)
    for (uint32_t i = tid * 16u; i < a.hdr.lds_bytes; i += blockDim.x * 16u)
        *(u32x4 *)(smem + i) = *(const u32x4 *)(a.prog + i);
    __syncthreads();

    // ---- walk constants of a plain table program (no window addressing, compact page map)
    Walk wk;
    constexpr uint32_t ELEM = MODE == MODE_TABLE16 ? 2u : 1u;
    wk.ncols_e = a.hdr.n_cols * ELEM;
    wk.pad_e = a.hdr.pad_col * ELEM;
    wk.pre_e = (a.hdr.pad_col + 1u) * ELEM;
    wk.pad_b = wk.pre_b = 0;
    wk.win_on = 0;
    wk.win_lo = wk.win_hi = 0;
    wk.dead_hi = 0;
    wk.sp_chains = wk.sp_pad_ident = 0;
    wk.flat = 0;
    wk.table_off = a.hdr.off_table;
    wk.lane4 = (uint32_t)(lane & 31) * 4u;
    wk.gtable = nullptr;
    wk.hot_last = 0;
    const uint32_t accept_lo = a.hdr.accept_lo, start_state = a.hdr.start, mask_off = a.hdr.ft_codes_off;
    const uint32_t group_mask = sa.group_mask;

    const PackedWindow<CHB> win(a.hdr.lds_bytes, 0u, wave);
    const uint64_t n_rows = a.n_rows;

    uint64_t rs, re;        // this lane's row as absolute byte addresses [rs, re) (packed_stream)
    uint32_t st, m, skip, rem;
    bool row_ok;
    auto begin_group = [&](uint64_t grp) __attribute__((always_inline)) {
        row_ok = ((grp << 6) + (uint64_t)lane) < n_rows;
        skip = (uint32_t)(rs & 15u) / CW;        // chars of the origin block before the row
        rem = skip + (uint32_t)((re - rs) / CW); // chars from the origin to the row's end
        st = start_state;
        m = 0u;
        if (OP == OP_CONTAINED_IN) m = lds_u32(mask_off + start_state * 4u); // the members whose root accepts
    };
    auto resolved = [&]() __attribute__((always_inline)) { return OP == OP_CONTAINED_IN ? m == group_mask : st == 0u; };
    auto unresolved = [&]() __attribute__((always_inline)) { return !resolved(); };
    auto wanted_from = [&]() __attribute__((always_inline)) { return rs; };

    auto walk_block = [&](const u32x4 c, uint32_t p0, auto guard) __attribute__((always_inline)) {
        constexpr bool G = decltype(guard)::value;
        const uint32_t wv[4] = {c[0], c[1], c[2], c[3]};
        if constexpr (OP == OP_MATCHES) {
            int32_t unused = -1;
            walk_piece<OP_MATCHES, CW, MODE, G>(wk, wv, p0, G ? rem : 0u, G ? skip : 0u, accept_lo, st, unused);
        } else {
            set_walk_block<CW, MODE, G>(wk, wv, p0, G ? rem : 0u, G ? skip : 0u, accept_lo, mask_off, group_mask, st, m);
        }
    };
    // Walk the window at w (its bytes are in LDS): this lane's blocks of [max(rs, w), min(re, w + kWin)) -- first and last one guarded
    auto walk_window = [&](uint64_t w) __attribute__((always_inline)) {
        const uint64_t lo = rs > w ? rs : w;
        const uint64_t hi = re < w + kWin ? re : w + kWin;
        if (lo < hi && !resolved()) {
            const uint32_t kb0 = (uint32_t)(lo - w) >> 4, kb1 = (uint32_t)(hi - 1u - w) >> 4;
            const uint32_t rel = (uint32_t)(w - (rs & ~(uint64_t)15)); // window start - origin (mod 2^32)
            auto p0_of = [&](uint32_t kb) __attribute__((always_inline)) { return (rel + kb * 16u) / CW; };
            {
                const u32x4 c = *(const lds_u32x4 *)(uintptr_t)win.at(kb0 * 16u);
                walk_block(c, p0_of(kb0), std::true_type());
            }
            if (kb1 > kb0) {
                u32x4 v = *(const lds_u32x4 *)(uintptr_t)win.at((kb0 + 1u) * 16u);
                for (uint32_t kb = kb0 + 1u; kb < kb1; ++kb) {
                    const u32x4 c = v;
                    v = *(const lds_u32x4 *)(uintptr_t)win.at((kb + 1u) * 16u); // next block: its latency hides below
                    walk_block(c, p0_of(kb), std::false_type());
                }
                walk_block(v, p0_of(kb1), std::true_type());
            }
        }
    };
    auto finish_rows = [&](uint64_t grp) __attribute__((always_inline)) {
        if (!row_ok) return;
        const uint64_t r = (grp << 6) + (uint64_t)lane;
        uint32_t bits = m;
        if (OP == OP_MATCHES) bits = lds_u32(mask_off + st * 4u); // (the sink's mask is 0)
        if (!sa.store) bits |= sa.masks[r];
        sa.masks[r] = bits;
    };

    packed_stream<CW, CHB>(lane, wave, n_waves, a.rows, sa.p.offsets, n_rows, win, rs, re, begin_group, walk_window, unresolved, wanted_from,
                           finish_rows);
}

template <int OP, int CW, int MODE, int CHB>
static hipError_t launch_packed_set_one(const PackedSetArgs &a, PackedShape sh, hipStream_t stream) {
    auto k = packed_set_kernel<OP, CW, MODE, CHB>;
    static thread_local uint64_t configured = 0;
    if (hipError_t e = allow_full_lds((const void *)k, configured); e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3(sh.grid), dim3(sh.waves * 64), sh.lds, stream, a);
    return hipGetLastError();
}

template <int CW>
static hipError_t launch_packed_set_cw(int op, const PackedSetArgs &a, PackedShape sh, hipStream_t s) {
    const uint32_t mode = a.p.s.hdr.mode;
    if (mode != MODE_TABLE8 && mode != MODE_TABLE16) return hipErrorInvalidValue;
#define NEEDLE_SET_CASE(OP, MODE)                                                                                              \
    if (op == OP && mode == MODE)                                                                                              \
        return sh.chb == 128 ? launch_packed_set_one<OP, CW, MODE, 128>(a, sh, s) : launch_packed_set_one<OP, CW, MODE, 64>(a, sh, s);
    NEEDLE_SET_CASE(OP_MATCHES, MODE_TABLE8)
    NEEDLE_SET_CASE(OP_MATCHES, MODE_TABLE16)
    NEEDLE_SET_CASE(OP_CONTAINED_IN, MODE_TABLE8)
    NEEDLE_SET_CASE(OP_CONTAINED_IN, MODE_TABLE16)
#undef NEEDLE_SET_CASE
    return hipErrorInvalidValue;
}

} // namespace needle
