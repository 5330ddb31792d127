// needle_replace_groups.hip -- replace every match of every row of a PACKED batch by a TEMPLATE of literals and group references
// ($2-$1), or keep it, hand-written for gfx950 (CDNA4): the kernels of needle_replace_groups_lengths_packed_dev /
// needle_replace_groups_fill_packed_dev (include/needle_hip.h).
//
//   The sweep is needle_gather.hip's, the running D is needle_replace.hip's; read those files' heads first.  A wave owns a 64-row group,
//   whose output is one contiguous run of PIECES; a piece k has a first output byte O_k, ends where piece k + 1 begins, and has one of
//   two sources, filed as D_k and a flag:
//     the input: output byte x is the input at x - D_k.  The gap behind a match (D = the group's first output address minus its first
//       input address, plus what the replaced matches in front have added), and a group's text (D = O_k minus the text's address: it
//       may lie anywhere in its row, the same text may be read twice, D is NOT monotone);
//     the literals in LDS: output byte x is literal byte x - D_k (D = O_k minus the literal's byte offset), at char width 1 at any byte.
//   A replaced match is always P pieces -- its template's group texts and non-empty literals in their order, then the gap behind it --
//   so the chunk's piece table is cut on the host: floor(kGroupsTableEntries / P) matches.  A lane builds one piece: c = its bytes (the
//   gap's lane: minus the match's bytes), one wave prefix sum S over c gives every O = (the match's input address) + D + S_exclusive and
//   the gap's D = D + S_inclusive, which is carried on.  A KEPT match (plane 0 < 0) has no position: its P entries are empty pieces
//   at the O of the piece in front with the gap's D, so the gap simply runs on.  A group the match did not pass is an empty piece.
//   Loads: an aligned 16-byte block is loaded only when it holds a byte of the group's input span; a group text is clamped into its ROW,
//   which lies inside it.  Stores: inside the chunk's range, which is inside the group's output span; edges code unit by code unit.
//   Planes of any value give a defined result; a list whose replaced matches are not monotone gives unspecified text, never an access
//   outside the spans.
// The sweep is a copy, not a shared header, for the reason needle_gather.hip gives: the other kernels' registers and LDS stay as they are.
#include <hip/hip_runtime.h>
#include <type_traits>

#include "needle_csr_rows.h"
#include "needle_launch.h"
#include "needle_replace_groups.h"

namespace needle {

typedef uint32_t rg_u32x4 __attribute__((ext_vector_type(4)));
// (needle_replace.hip: loads and stores of text name the GLOBAL address space, so that they are global_* instructions)
#define RG_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ uint64_t groups_clamp(uint64_t x, uint64_t lo, uint64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// The template's head into LDS: whole 16 bytes.
__device__ __forceinline__ void groups_stage_head(const ReplaceGroupsArgs &a, uint32_t *head) {
    for (uint32_t i = threadIdx.x * 16u; i < kGroupsHeadBytes; i += kReplaceWaves * 64u * 16u)
        *(rg_u32x4 *)((uint8_t *)head + i) = *(const rg_u32x4 *)(a.table + i);
}

__global__ __launch_bounds__(kReplaceWaves * 64) void replace_groups_lengths_kernel(const ReplaceGroupsArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t s_head[kGroupsHeadWords];
    __shared__ uint64_t s_mo[kReplaceWaves][65], s_ino[kReplaceWaves][65];
    __shared__ unsigned long long s_gone[kReplaceWaves][64], s_come[kReplaceWaves][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave];
    unsigned long long *gone = s_gone[wave], *come = s_come[wave];
    groups_stage_head(a, s_head);
    __syncthreads();
    const uint32_t K = a.n_refs < kTemplateMaxRefs ? a.n_refs : kTemplateMaxRefs;
    const uint64_t n_groups = (a.n_rows + 63u) >> 6;
    for (uint64_t grp = (uint64_t)blockIdx.x * kReplaceWaves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kReplaceWaves) {
        const uint64_t g0 = grp << 6;
        csr_group_offsets(a.match_off, a.in_off, a.n_rows, g0, lane, mo, ino);
        gone[lane] = 0ull;
        come[lane] = 0ull;
        csr_wave_sync();
        const uint64_t m0 = mo[0], m1 = mo[64];
        for (uint64_t m = m0 + (uint64_t)lane; m < m1; m += 64u) {
            const int32_t gs0 = a.gstart[m];
            if (gs0 < 0) continue; // (a kept match changes nothing)
            const uint32_t r = csr_row_of(mo, m);
            const uint64_t len = ino[r + 1] - ino[r];
            uint64_t s, e, in = (uint64_t)a.lit_units;
            csr_clamp(gs0, a.gend[m], len, &s, &e);
            for (uint32_t k = 0; k < K; ++k) { // (plane g is contiguous in m: the wave's loads coalesce)
                const uint64_t at = (uint64_t)s_head[k] * a.plane_stride + m;
                const int32_t xs = a.gstart[at];
                if (xs < 0) continue; // a group the match did not pass
                uint64_t x, y;
                csr_clamp(xs, a.gend[at], len, &x, &y);
                in += y - x;
            }
            atomicAdd(&gone[r], (unsigned long long)(e - s));
            atomicAdd(&come[r], (unsigned long long)in);
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

template <int CW>
__global__ __launch_bounds__(kReplaceWaves * 64) void replace_groups_fill_kernel(const ReplaceGroupsArgs a) {
    using T = std::conditional_t<CW == 1, uint8_t, uint16_t>;
    constexpr uint32_t E = kGroupsTableEntries;
    __shared__ __attribute__((aligned(16))) uint8_t s_lits[kReplaceMaxUnits * 2];
    __shared__ __attribute__((aligned(16))) uint32_t s_head[kGroupsHeadWords];
    __shared__ uint64_t s_mo[kReplaceWaves][65], s_ino[kReplaceWaves][65];
    __shared__ uint64_t s_O[kReplaceWaves][E + 1]; // O of the chunk's pieces; entry np: the next chunk's first O, or the end of the group
    __shared__ uint64_t s_D[kReplaceWaves][E];     // D of piece k
    __shared__ uint8_t s_L[kReplaceWaves][E];      // piece k is a literal
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave], *O = s_O[wave], *Dn = s_D[wave];
    uint8_t *Ln = s_L[wave];

    const uint32_t LB = (a.lit_units < kReplaceMaxUnits ? a.lit_units : kReplaceMaxUnits) * CW; // the literals' bytes
    groups_stage_head(a, s_head);
    for (uint32_t i = threadIdx.x * 16u; i < LB; i += kReplaceWaves * 64u * 16u)
        *(rg_u32x4 *)(s_lits + i) = *(const rg_u32x4 *)(a.table + kGroupsHeadBytes + i);
    __syncthreads();

    // (what the host derived from the template, kept inside the piece table whatever it passes)
    const uint32_t P = a.pieces < 1u ? 1u : (a.pieces > kGroupsMaxPieces ? kGroupsMaxPieces : a.pieces);
    const uint32_t CM = a.chunk < 1u ? 1u : (a.chunk > E / P ? E / P : a.chunk);
    const uint64_t n = a.n_rows, n_groups = (n + 63u) >> 6;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.data, obase = (uint64_t)(uintptr_t)a.out;
    const uint64_t in_first = a.in_off[0], in_last = a.in_off[n], out_first = a.out_off[0], out_last = a.out_off[n];
    for (uint64_t grp = (uint64_t)blockIdx.x * kReplaceWaves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kReplaceWaves) {
        const uint64_t g0 = grp << 6, g1 = g0 + 64u < n ? g0 + 64u : n;
        const uint64_t out_g0 = a.out_off[g0], out_g1 = a.out_off[g1]; // (with the other offsets: one round trip)
        csr_group_offsets(a.match_off, a.in_off, a.n_rows, g0, lane, mo, ino);
        csr_wave_sync();
        // the group's spans as absolute byte addresses, inside the batch's
        const uint64_t in_b = groups_clamp(ino[0], in_first, in_last), out_b = groups_clamp(out_g0, out_first, out_last);
        const uint64_t inB = dbase + in_b * CW, inE = dbase + groups_clamp(ino[64], in_b, in_last) * CW;
        const uint64_t outB = obase + out_b * CW, outE = obase + groups_clamp(out_g1, out_b, out_last) * CW;
        const uint64_t m0 = mo[0], m1 = mo[64] > m0 ? mo[64] : m0;
        uint64_t D = outB - inB; // the gaps' running D (mod 2^64 throughout), carried across the chunks
        uint64_t Olast = outB;   // O of the last piece tabled so far: where a kept match's empty pieces stand
        uint64_t lo = outB;
        for (uint64_t mb = m0;; mb += CM) {
            const uint32_t nm = (uint32_t)(m1 - mb < (uint64_t)CM ? m1 - mb : (uint64_t)CM);
            const uint32_t np = nm * P;
            const bool last = mb + nm >= m1;
            const uint64_t Dpre = D;
            // ---- the chunk's piece table: a lane builds one piece
            for (uint32_t k0 = 0; k0 < np; k0 += 64u) {
                const uint32_t k = k0 + (uint32_t)lane;
                long long c = 0;       // the piece's bytes; the gap's lane: minus the match's
                uint64_t I = 0;        // the match's first input byte
                uint64_t src = 0;      // a group text's first input byte, or a literal's byte offset
                uint32_t kind = 0;     // 0 the gap behind the match, or any piece of a kept match; 1 a group text; 2 a literal
                bool replaced = false;
                if (k < np) {
                    const uint32_t mi = (k * a.inv_pieces) >> 16, j = k - mi * P;
                    const uint64_t m = mb + mi;
                    const int32_t gs0 = a.gstart[m];
                    if (gs0 >= 0) {
                        replaced = true;
                        const uint32_t r = csr_row_of(mo, m);
                        const uint64_t len = ino[r + 1] - ino[r], row = dbase + ino[r] * CW;
                        uint64_t s, e;
                        csr_clamp(gs0, a.gend[m], len, &s, &e);
                        I = row + s * CW;
                        if (j + 1u == P) {
                            c = -(long long)((e - s) * CW);
                        } else {
                            const uint32_t t = s_head[kGroupsPieceWord0 + j];
                            if (t & kGroupsRef) {
                                kind = 1;
                                src = row;
                                const uint64_t at = (uint64_t)(t & ~kGroupsRef) * a.plane_stride + m;
                                const int32_t xs = a.gstart[at];
                                if (xs >= 0) { // (a group the match did not pass stays an empty piece)
                                    uint64_t x, y;
                                    csr_clamp(xs, a.gend[at], len, &x, &y);
                                    src = row + x * CW;
                                    c = (long long)((y - x) * CW);
                                }
                            } else {
                                kind = 2;
                                src = (uint64_t)(t & 0x3FFFu);
                                c = (long long)((t >> 14) & 0x3FFFu);
                            }
                        }
                    }
                }
                long long incl = c;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const long long up = __shfl_up(incl, d, 64);
                    if (lane >= d) incl += up;
                }
                uint64_t Ok = I + D + (uint64_t)(incl - c);
                // a piece of a kept match (or no piece at all) stands where the last piece of a replaced match in front of it does
                const uint64_t rm = __ballot(replaced), below = rm & ((1ull << lane) - 1ull);
                const int from = replaced ? lane : (below ? 63 - (int)__builtin_clzll(below) : lane);
                const uint64_t Ofrom = (uint64_t)__shfl((unsigned long long)Ok, from, 64);
                if (!replaced) Ok = below ? Ofrom : Olast;
                if (k < np) {
                    O[k] = Ok;
                    Dn[k] = kind == 0u ? D + (uint64_t)incl : Ok - src;
                    Ln[k] = (uint8_t)(kind == 2u);
                }
                D += (uint64_t)__shfl(incl, 63, 64);
                Olast = (uint64_t)__shfl((unsigned long long)Ok, 63, 64);
            }
            if (lane == 0) {
                uint64_t On = inE + D;
                if (!last) {
                    const uint64_t m = mb + nm;
                    const int32_t gs0 = a.gstart[m];
                    On = Olast;
                    if (gs0 >= 0) {
                        const uint32_t r = csr_row_of(mo, m);
                        uint64_t s, e;
                        csr_clamp(gs0, a.gend[m], ino[r + 1] - ino[r], &s, &e);
                        On = dbase + (ino[r] + s) * CW + D;
                    }
                }
                O[np] = On;
            }
            csr_wave_sync();
            const uint64_t hi = last ? outE : groups_clamp(O[np], lo, outE);

            // ---- sweep the chunk's output range [lo, hi): 64 lanes x 16 bytes a step, a lane's 16 bytes piece by piece (needle_gather.hip)
            uint32_t step0 = 0; // the binary search's first step: the largest power of two <= np (wave-uniform)
            if (np) step0 = 1u << (31u - (uint32_t)__builtin_clz(np));
            for (uint64_t X = (lo & ~(uint64_t)15) + (uint64_t)lane * 16u; X < hi; X += 1024u) {
                const uint64_t x0 = X > lo ? X : lo, x1 = X + 16u < hi ? X + 16u : hi;
                if (x0 >= x1) continue; // (an empty range that begins inside a 16-byte block)
                uint32_t jj = 0;        // the chunk's pieces with O <= x
                for (uint32_t step = step0; step; step >>= 1)
                    if (jj + step <= np && O[jj + step - 1u] <= x0) jj += step;
                // (no piece in front: the gap behind the chunk before, or the text in front of the group's first match)
                uint64_t Dcur = jj ? Dn[jj - 1u] : Dpre, Onext = O[jj];
                uint32_t Lcur = jj ? (uint32_t)Ln[jj - 1u] : 0u;
                uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
                uint64_t x = x0;
                do {
                    while (jj < np && Onext <= x) { // the pieces that begin at or before x (several: empty ones)
                        Dcur = Dn[jj];
                        Lcur = (uint32_t)Ln[jj];
                        ++jj;
                        Onext = O[jj];
                    }
                    const uint64_t pe = jj < np && Onext < x1 ? Onext : x1; // the piece at x ends here: always beyond x
                    const uint64_t A = X - Dcur; // the source of the block's first byte: an input address, or a byte among the literals (may be < 0)
                    uint32_t t0, t1, t2, t3, t4, sh;
                    if (Lcur) { // a literal: the dwords around byte A of the literals; they bring neighbouring literals along, the mask drops them
                        const int64_t r0 = (int64_t)A;
                        const int64_t d0 = r0 & ~(int64_t)3;
                        sh = (uint32_t)r0 & 3u;
                        auto dword = [&](int i) __attribute__((always_inline)) -> uint32_t {
                            const int64_t at = d0 + 4 * i;
                            return at >= 0 && at < (int64_t)sizeof(s_lits) ? *(const uint32_t *)(s_lits + at) : 0u;
                        };
                        t0 = dword(0), t1 = dword(1), t2 = dword(2), t3 = dword(3), t4 = dword(4);
                    } else { // the input: a gap, or a group's text
                        const uint32_t kb = (uint32_t)A & 15u;
                        const uint64_t P0 = A - kb, P1 = P0 + 16u;
                        rg_u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
                        // (an aligned block is loaded only when it holds a byte of the group's input span -- the piece's own bytes always do)
                        if (P0 < inE && P1 > inB && P1 > P0) v0 = *(const RG_GLOBAL rg_u32x4 *)(uintptr_t)P0;
                        if (kb && P1 < inE && P1 + 16u > inB && P1 + 16u > P1) v1 = *(const RG_GLOBAL rg_u32x4 *)(uintptr_t)P1;
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
                    const uint32_t k0 = below(be) & ~below(bs), k1 = below(be - 4) & ~below(bs - 4);
                    const uint32_t k2 = below(be - 8) & ~below(bs - 8), k3 = below(be - 12) & ~below(bs - 12);
                    w0 = (w0 & ~k0) | (f0 & k0), w1 = (w1 & ~k1) | (f1 & k1), w2 = (w2 & ~k2) | (f2 & k2), w3 = (w3 & ~k3) | (f3 & k3);
                    x = pe;
                } while (x < x1);
                if (X >= lo && X + 16u <= hi) { // the chunk's own 16 bytes: one store
                    const rg_u32x4 w = {w0, w1, w2, w3};
                    *(RG_GLOBAL rg_u32x4 *)(uintptr_t)X = w;
                } else { // an edge of the chunk's range, shared with another wave or with the caller's memory: the own units only
                    const uint32_t ww[4] = {w0, w1, w2, w3};
#pragma unroll
                    for (uint32_t b = 0; b < 16u; b += CW) {
                        const uint64_t xb = X + b;
                        if (xb >= x0 && xb < x1) *(RG_GLOBAL T *)(uintptr_t)xb = (T)(ww[b >> 2] >> ((b & 3u) * 8u));
                    }
                }
            }
            lo = hi;
            csr_wave_sync(); // (the next chunk, or the next group, overwrites the tables)
            if (last) break;
        }
    }
}

static int replace_groups_grid(uint64_t n_rows, int n_cus) {
    const uint64_t blocks = ((n_rows + 63u) / 64u + kReplaceWaves - 1u) / kReplaceWaves;
    const uint64_t cap = (uint64_t)(n_cus > 0 ? n_cus : 1) * 16u;
    return (int)(blocks < cap ? blocks : cap);
}

hipError_t launch_replace_groups_lengths(const ReplaceGroupsArgs &a, int n_cus, hipStream_t stream) {
    hipLaunchKernelGGL(replace_groups_lengths_kernel, dim3(replace_groups_grid(a.n_rows, n_cus)), dim3(kReplaceWaves * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_replace_groups_fill(const ReplaceGroupsArgs &a, int n_cus, hipStream_t stream) {
    const dim3 grid(replace_groups_grid(a.n_rows, n_cus)), block(kReplaceWaves * 64);
    if (a.cw == 1) hipLaunchKernelGGL(replace_groups_fill_kernel<1>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(replace_groups_fill_kernel<2>, grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace needle
