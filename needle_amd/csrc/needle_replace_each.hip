// needle_replace_each.hip -- replace every match of every row of a PACKED batch by the entry of a replacement TABLE that the match's
// choice names, or keep it, hand-written for gfx950 (CDNA4): the kernels of needle_replace_each_lengths_packed_dev /
// needle_replace_each_fill_packed_dev (include/needle_hip.h).
//
//   The algorithm is needle_replace.hip's, read that file's head first: a wave owns a 64-row group, the group's matches go through a
//   piece table in LDS in chunks (here of kReplaceEachChunk), and the wave sweeps the chunk's output range in steps of 64 lanes x 16 bytes, each
//   lane putting its 16 bytes together piece by piece.  These kernels are a copy of that sweep, instantiated apart, so that the plain
//   kernels keep their registers and their LDS; what differs:
//     a piece has its OWN replacement: R_m bytes at byte off_m of the table, both filed beside O_m and D_m (one dword per piece,
//       off | R << 16).  delta_m = R_m - (e - s) * CW; O stays sorted because O_(m+1) >= O_m + R_m, so the binary search and the advance
//       over the matches that begin at or before x are untouched;
//     "inside the replacement" is rel < R_(jj-1), and its five dwords come from the table at off_(jj-1) + (X - Oprev): at char width 1
//       an entry starts at any byte, so the dword index and the funnel shift are taken from the SUM.  The dwords bring bytes of the
//       neighbouring entries along; the piece mask drops them, as it drops neighbouring text;
//     a KEPT match (a choice outside the table) is no third kind of piece: it is filed with R = 0 and delta = 0, and the gap behind its
//       O reads the input at x - D, which starts with the match's own text;
//     the choice is read with start / end: an int32 index, or a uint32 mask whose lowest set bit is the index (one ctz under a select).
//   The table -- 260 dwords of offsets, then the entries' units -- is staged into LDS once per workgroup; a choice is checked against
//   n_repl before it indexes the offsets, so nothing outside the table is ever read, whatever the choice array holds.
#include <hip/hip_runtime.h>
#include <type_traits>

#include "needle_csr_rows.h"
#include "needle_launch.h"
#include "needle_replace_each.h"

namespace needle {

typedef uint32_t rpe_u32x4 __attribute__((ext_vector_type(4)));
// (needle_replace.hip: loads and stores of text name the GLOBAL address space, so that they are global_* instructions)
#define RPE_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ uint64_t each_clamp(uint64_t x, uint64_t lo, uint64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Match m of row r (group-relative) clamped into its row: *s <= *e <= the row's length, in code units.
__device__ __forceinline__ void each_match(const ReplaceEachArgs &a, const uint64_t *ino, uint64_t m, uint32_t r, uint64_t *s, uint64_t *e) {
    csr_clamp(a.start[m], a.end[m], ino[r + 1] - ino[r], s, e);
}

// The table entry that match m's choice names, or -1: the match is kept.  Defined for every 32-bit value.
__device__ __forceinline__ int each_choice(const ReplaceEachArgs &a, uint64_t m) {
    const uint32_t raw = a.choice[m];
    const int c = a.choice_form ? (raw != 0u ? (int)__builtin_ctz(raw) : -1) : (int)raw;
    return (uint32_t)c < a.n_repl ? c : -1; // (a negative index is a huge unsigned one)
}

// The table's offsets (code units) into LDS: whole 16 bytes, entries behind n_repl are 0 and never read.
__device__ __forceinline__ void each_stage_offsets(const ReplaceEachArgs &a, uint32_t *roff) {
    for (uint32_t i = threadIdx.x * 16u; i < kReplaceEachOffsetBytes; i += kReplaceWaves * 64u * 16u)
        *(rpe_u32x4 *)((uint8_t *)roff + i) = *(const rpe_u32x4 *)(a.table + i);
}

__global__ __launch_bounds__(kReplaceWaves * 64) void replace_each_lengths_kernel(const ReplaceEachArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_roff[kReplaceEachOffsetBytes / 4];
    __shared__ uint64_t s_mo[kReplaceWaves][65], s_ino[kReplaceWaves][65];
    __shared__ unsigned long long s_gone[kReplaceWaves][64], s_come[kReplaceWaves][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave];
    unsigned long long *gone = s_gone[wave], *come = s_come[wave];
    each_stage_offsets(a, s_roff);
    __syncthreads();
    const uint64_t n_groups = (a.n_rows + 63u) >> 6;
    for (uint64_t grp = (uint64_t)blockIdx.x * kReplaceWaves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kReplaceWaves) {
        const uint64_t g0 = grp << 6;
        csr_group_offsets(a.match_off, a.in_off, a.n_rows, g0, lane, mo, ino);
        gone[lane] = 0ull;
        come[lane] = 0ull;
        csr_wave_sync();
        const uint64_t m0 = mo[0], m1 = mo[64];
        for (uint64_t m = m0 + (uint64_t)lane; m < m1; m += 64u) {
            const uint32_t r = csr_row_of(mo, m);
            uint64_t s, e;
            each_match(a, ino, m, r, &s, &e);
            const int c = each_choice(a, m);
            if (c >= 0) { // (a kept match changes nothing)
                atomicAdd(&gone[r], (unsigned long long)(e - s));
                atomicAdd(&come[r], (unsigned long long)(s_roff[c + 1] - s_roff[c]));
            }
        }
        csr_wave_sync();
        if (g0 + (uint64_t)lane < a.n_rows) {
            const uint64_t len = ino[lane + 1] - ino[lane];
            const uint64_t g = gone[lane] < len ? gone[lane] : len;
            a.out_len[g0 + (uint64_t)lane] = len - g + come[lane];
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

// Five waves per SIMD, as the plain fill kernel has with its 94 registers: without the hint the extra piece field costs 98 registers,
// which the hardware rounds to 104 -- four waves.  With it: 90, no scratch.
template <int CW>
__global__ __launch_bounds__(kReplaceWaves * 64) __attribute__((amdgpu_waves_per_eu(5))) void replace_each_fill_kernel(const ReplaceEachArgs a) {
    using T = std::conditional_t<CW == 1, uint8_t, uint16_t>;
    constexpr uint32_t K = kReplaceEachChunk;
    __shared__ __attribute__((aligned(16))) uint8_t s_repl[kReplaceMaxUnits * 2];
    __shared__ __attribute__((aligned(16))) uint32_t s_roff[kReplaceEachOffsetBytes / 4];
    __shared__ uint64_t s_mo[kReplaceWaves][65], s_ino[kReplaceWaves][65];
    __shared__ uint64_t s_O[kReplaceWaves][K + 1]; // O of the chunk's matches; entry nk: the next chunk's first O, or the end of the group
    __shared__ uint64_t s_D[kReplaceWaves][K];     // D behind match k (the gap that follows it)
    __shared__ uint32_t s_R[kReplaceWaves][K + 1]; // match k's replacement: its byte offset in s_repl | its bytes << 16 (kept: 0); entry nk: read, never used
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave], *O = s_O[wave], *Dn = s_D[wave];
    uint32_t *Rn = s_R[wave];

    const uint32_t TB = (a.table_units < kReplaceMaxUnits ? a.table_units : kReplaceMaxUnits) * CW; // the table's bytes
    each_stage_offsets(a, s_roff);
    for (uint32_t i = threadIdx.x * 16u; i < TB; i += kReplaceWaves * 64u * 16u)
        *(rpe_u32x4 *)(s_repl + i) = *(const rpe_u32x4 *)(a.table + kReplaceEachOffsetBytes + i);
    __syncthreads();

    const uint64_t n = a.n_rows, n_groups = (n + 63u) >> 6;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.data, obase = (uint64_t)(uintptr_t)a.out;
    const uint64_t in_first = a.in_off[0], in_last = a.in_off[n], out_first = a.out_off[0], out_last = a.out_off[n];
    for (uint64_t grp = (uint64_t)blockIdx.x * kReplaceWaves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kReplaceWaves) {
        const uint64_t g0 = grp << 6, g1 = g0 + 64u < n ? g0 + 64u : n;
        const uint64_t out_g0 = a.out_off[g0], out_g1 = a.out_off[g1]; // (with the other offsets: one round trip)
        csr_group_offsets(a.match_off, a.in_off, a.n_rows, g0, lane, mo, ino);
        csr_wave_sync();
        // the group's spans as absolute byte addresses, inside the batch's
        const uint64_t in_b = each_clamp(ino[0], in_first, in_last), out_b = each_clamp(out_g0, out_first, out_last);
        const uint64_t inB = dbase + in_b * CW, inE = dbase + each_clamp(ino[64], in_b, in_last) * CW;
        const uint64_t outB = obase + out_b * CW, outE = obase + each_clamp(out_g1, out_b, out_last) * CW;
        const uint64_t m0 = mo[0], m1 = mo[64] > m0 ? mo[64] : m0;
        uint64_t D = outB - inB; // (mod 2^64 throughout)
        uint64_t lo = outB;
        for (uint64_t mb = m0;; mb += K) {
            const uint32_t nk = (uint32_t)(m1 - mb < (uint64_t)K ? m1 - mb : (uint64_t)K);
            const bool last = mb + nk >= m1;
            const uint64_t Dpre = D;
            // ---- the chunk's piece table
            for (uint32_t k0 = 0; k0 < nk; k0 += 64u) {
                const uint32_t k = k0 + (uint32_t)lane;
                uint64_t I = 0;
                long long delta = 0;
                uint32_t rk = 0;
                if (k < nk) {
                    const uint64_t m = mb + k;
                    const uint32_t r = csr_row_of(mo, m);
                    uint64_t s, e;
                    each_match(a, ino, m, r, &s, &e);
                    I = dbase + (ino[r] + s) * CW;
                    const int c = each_choice(a, m);
                    if (c >= 0) {
                        const uint32_t at = s_roff[c] * CW, rb = (s_roff[c + 1] - s_roff[c]) * CW;
                        delta = (long long)rb - (long long)((e - s) * CW);
                        rk = rb ? at | (rb << 16) : 0u;
                    }
                }
                long long incl = delta;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const long long up = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += up;
                }
                const uint64_t Dk = D + (uint64_t)(incl - delta);
                if (k < nk) {
                    O[k] = I + Dk;
                    Dn[k] = Dk + (uint64_t)delta;
                    Rn[k] = rk;
                }
                D += (uint64_t)__shfl(incl, 63, 64);
            }
            if (lane == 0) {
                uint64_t I = inE;
                if (!last) {
                    const uint64_t m = mb + nk;
                    const uint32_t r = csr_row_of(mo, m);
                    uint64_t s, e;
                    each_match(a, ino, m, r, &s, &e);
                    I = dbase + (ino[r] + s) * CW;
                }
                O[nk] = I + D;
            }
            csr_wave_sync();
            const uint64_t hi = last ? outE : each_clamp(O[nk], lo, outE);

            // ---- sweep the chunk's output range [lo, hi): 64 lanes x 16 bytes a step, a lane's 16 bytes piece by piece (needle_replace.hip)
            uint32_t step0 = 0; // the binary search's first step: the largest power of two <= nk (wave-uniform)
            if (nk) step0 = 1u << (31u - (uint32_t)__builtin_clz(nk));
            for (uint64_t X = (lo & ~(uint64_t)15) + (uint64_t)lane * 16u; X < hi; X += 1024u) {
                const uint64_t x0 = X > lo ? X : lo, x1 = X + 16u < hi ? X + 16u : hi;
                if (x0 >= x1) continue; // (an empty range that begins inside a 16-byte block)
                uint32_t jj = 0;        // the chunk's matches with O <= x
                for (uint32_t step = step0; step; step >>= 1)
                    if (jj + step <= nk && O[jj + step - 1u] <= x0) jj += step;
                uint64_t Oprev = jj ? O[jj - 1u] : 0ull, Dcur = jj ? Dn[jj - 1u] : Dpre, Onext = O[jj];
                // (no match in front: no replacement.  The NEXT piece's replacement travels with Onext, so that the advance below hands it over
                // out of a register: "inside the replacement?" is decided at once, as in the plain kernel, not after one more LDS round trip)
                uint32_t Rcur = jj ? Rn[jj - 1u] : 0u, Rnext = Rn[jj];
                uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
                uint64_t x = x0;
                do {
                    while (jj < nk && Onext <= x) { // the matches that begin at or before x (several: touching, empty or kept ones)
                        Oprev = Onext;
                        Dcur = Dn[jj];
                        Rcur = Rnext;
                        ++jj;
                        Onext = O[jj];
                        Rnext = Rn[jj];
                    }
                    const uint64_t rel = x - Oprev, RB = (uint64_t)(Rcur >> 16);
                    uint64_t pe; // the piece at x ends here: always beyond x
                    uint32_t t0, t1, t2, t3, t4, sh;
                    if (rel < RB) { // inside replacement jj - 1: the table's dwords around byte off + (X - Oprev); X - Oprev may be < 0
                        pe = Oprev + RB < x1 ? Oprev + RB : x1;
                        const int64_t r0 = (int64_t)(X - Oprev) + (int64_t)(Rcur & 0xFFFFu);
                        const int64_t d0 = r0 & ~(int64_t)3;
                        sh = (uint32_t)r0 & 3u;
                        auto dword = [&](int i) __attribute__((always_inline)) -> uint32_t {
                            const int64_t at = d0 + 4 * i;
                            return at >= 0 && at < (int64_t)sizeof(s_repl) ? *(const uint32_t *)(s_repl + at) : 0u;
                        };
                        t0 = dword(0), t1 = dword(1), t2 = dword(2), t3 = dword(3), t4 = dword(4);
                    } else { // a gap: the input at (x - Dcur), up to the next match
                        pe = jj < nk && Onext < x1 ? Onext : x1;
                        const uint64_t A = X - Dcur;
                        const uint32_t kb = (uint32_t)A & 15u;
                        const uint64_t P0 = A - kb, P1 = P0 + 16u;
                        rpe_u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
                        // (an aligned block is loaded only when it holds a byte of the group's input span -- the piece's own bytes always do)
                        if (P0 < inE && P1 > inB && P1 > P0) v0 = *(const RPE_GLOBAL rpe_u32x4 *)(uintptr_t)P0;
                        if (kb && P1 < inE && P1 + 16u > inB && P1 + 16u > P1) v1 = *(const RPE_GLOBAL rpe_u32x4 *)(uintptr_t)P1;
                        const bool q2 = (kb & 8u) != 0u, q1 = (kb & 4u) != 0u;
                        uint32_t u0 = v0[0], u1 = v0[1], u2 = v0[2], u3 = v0[3], u4 = v1[0], u5 = v1[1], u6 = v1[2], u7 = v1[3];
                        u0 = q2 ? u2 : u0, u1 = q2 ? u3 : u1, u2 = q2 ? u4 : u2, u3 = q2 ? u5 : u3, u4 = q2 ? u6 : u4, u5 = q2 ? u7 : u5;
                        t0 = q1 ? u1 : u0, t1 = q1 ? u2 : u1, t2 = q1 ? u3 : u2, t3 = q1 ? u4 : u3, t4 = q1 ? u5 : u4;
                        sh = kb & 3u;
                    }
                    const uint32_t f0 = __builtin_amdgcn_alignbyte(t1, t0, sh), f1 = __builtin_amdgcn_alignbyte(t2, t1, sh);
                    const uint32_t f2 = __builtin_amdgcn_alignbyte(t3, t2, sh), f3 = __builtin_amdgcn_alignbyte(t4, t3, sh);
                    // the piece's own bytes [x, pe) of the block: a mask per dword
                    const int bs = (int)(uint32_t)(x - X), be = (int)(uint32_t)(pe - X);
                    auto below = [](int k) __attribute__((always_inline)) -> uint32_t { // the low min(max(k, 0), 4) bytes
                        const int c = k < 0 ? 0 : (k > 4 ? 4 : k);
                        return c == 4 ? 0xFFFFFFFFu : (1u << (8 * c)) - 1u;
                    };
                    const uint32_t m0 = below(be) & ~below(bs), m1 = below(be - 4) & ~below(bs - 4);
                    const uint32_t m2 = below(be - 8) & ~below(bs - 8), m3 = below(be - 12) & ~below(bs - 12);
                    w0 = (w0 & ~m0) | (f0 & m0), w1 = (w1 & ~m1) | (f1 & m1), w2 = (w2 & ~m2) | (f2 & m2), w3 = (w3 & ~m3) | (f3 & m3);
                    x = pe;
                } while (x < x1);
                if (X >= lo && X + 16u <= hi) { // the chunk's own 16 bytes: one store
                    const rpe_u32x4 w = {w0, w1, w2, w3};
                    *(RPE_GLOBAL rpe_u32x4 *)(uintptr_t)X = w;
                } else { // an edge of the chunk's range, shared with another wave or with the caller's memory: the own units only
                    const uint32_t ww[4] = {w0, w1, w2, w3};
#pragma unroll
                    for (uint32_t b = 0; b < 16u; b += CW) {
                        const uint64_t xb = X + b;
                        if (xb >= x0 && xb < x1) *(RPE_GLOBAL T *)(uintptr_t)xb = (T)(ww[b >> 2] >> ((b & 3u) * 8u));
                    }
                }
            }
            lo = hi;
            csr_wave_sync(); // (the next chunk, or the next group, overwrites the tables)
            if (last) break;
        }
    }
}

static int replace_each_grid(uint64_t n_rows, int n_cus) {
    const uint64_t blocks = ((n_rows + 63u) / 64u + kReplaceWaves - 1u) / kReplaceWaves;
    const uint64_t cap = (uint64_t)(n_cus > 0 ? n_cus : 1) * 16u;
    return (int)(blocks < cap ? blocks : cap);
}

hipError_t launch_replace_each_lengths(const ReplaceEachArgs &a, int n_cus, hipStream_t stream) {
    hipLaunchKernelGGL(replace_each_lengths_kernel, dim3(replace_each_grid(a.n_rows, n_cus)), dim3(kReplaceWaves * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_replace_each_fill(const ReplaceEachArgs &a, int n_cus, hipStream_t stream) {
    const dim3 grid(replace_each_grid(a.n_rows, n_cus)), block(kReplaceWaves * 64);
    if (a.cw == 1) hipLaunchKernelGGL(replace_each_fill_kernel<1>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(replace_each_fill_kernel<2>, grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace needle
