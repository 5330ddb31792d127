// needle_replace.hip -- replace every match of every row of a PACKED batch by one literal replacement, hand-written for gfx950 (CDNA4):
// the kernels of needle_replace_all_lengths_packed_dev / needle_replace_all_fill_packed_dev (include/needle_hip.h).
//
//   Rows lie back to back in the input and in the output, so a 64-row group is ONE contiguous text with ONE monotone match list, and a
//   wave owns a group as in the other packed kernels.  Row boundaries do not matter to the copy: they are in out_off already.
//   Everything is done in BYTES at absolute addresses (positions scaled by the char width), one body for both widths.
//     I_m = address of match m's first input byte,  D_m = (group's first output address - its first input address)
//           + sum over the group's earlier matches of (replacement bytes - matched bytes),  O_m = I_m + D_m:
//   replacement m occupies output [O_m, O_m + R), the gap behind it [O_m + R, O_(m+1)) is the input at (x - D_(m+1)), the text in front
//   of the group's first match the input at (x - D_first).  O is sorted because O_(m+1) >= O_m + R.
//   Fill: the group's matches in chunks of kReplaceChunk; a wave prefix sum gives the chunk's O and D (the "piece table", in LDS), D is
//   carried on.  The wave then sweeps the chunk's output range in steps of 64 lanes x 16 bytes on 16-byte aligned OUTPUT addresses; each
//   lane finds its block's first piece by binary search and puts its 16 bytes together PIECE BY PIECE -- a gap of the input or a
//   replacement:
//     a gap is fetched as if it filled the whole block: two aligned 16-byte loads around the (misaligned) source, a dword select and a
//       v_alignbyte funnel shift; a replacement the same way from its dwords in LDS; the piece's own bytes are merged under a byte mask;
//     a block inside one gap -- nearly all of them -- is one round, and the wave makes as many rounds as its block with the most pieces;
//     the 16 bytes are stored at once when all of them are the chunk's own, else code unit by code unit and ONLY the own units:
//       neighbouring groups' spans meet at byte granularity, and the batch's first and last bytes border the caller's memory.
//   Loads: an aligned 16-byte block is loaded only when it holds a byte of the group's input span (the packed kernels' rule), zeros
//   stand in for any other.  A list that is not monotone or leaves its row gives unspecified text, never an access outside the spans.
//   Lengths: a wave reads its group's contiguous range of start / end coalesced, finds each match's row by binary search over the
//   group's 65 match offsets (LDS) and adds e - s to the row's LDS counter.
#include <hip/hip_runtime.h>
#include <cstring>
#include <type_traits>

#include "needle_csr_rows.h"
#include "needle_launch.h"
#include "needle_replace.h"

namespace needle {

typedef uint32_t rp_u32x4 __attribute__((ext_vector_type(4)));
// Text addresses are computed as integers; loads and stores through them name the GLOBAL address space, so that they are global_*
// instructions: flat ones count on the LDS counter too and every piece-table read would wait for the loads in flight.
#define RP_GLOBAL __attribute__((address_space(1)))

// (The wave's hand-over, the group's offsets in LDS, the row search and the clamp are needle_csr_rows.h's, shared with needle_set_spans.h.)
__device__ __forceinline__ uint64_t replace_clamp(uint64_t x, uint64_t lo, uint64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Match m of row r (group-relative) clamped into its row: *s <= *e <= the row's length, in code units.
__device__ __forceinline__ void replace_match(const ReplaceArgs &a, const uint64_t *ino, uint64_t m, uint32_t r, uint64_t *s, uint64_t *e) {
    csr_clamp(a.start[m], a.end[m], ino[r + 1] - ino[r], s, e);
}

__global__ __launch_bounds__(kReplaceWaves * 64) void replace_lengths_kernel(const ReplaceArgs a) {
    __shared__ uint64_t s_mo[kReplaceWaves][65], s_ino[kReplaceWaves][65];
    __shared__ unsigned long long s_sum[kReplaceWaves][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave];
    unsigned long long *sum = s_sum[wave];
    const uint64_t n_groups = (a.n_rows + 63u) >> 6;
    for (uint64_t grp = (uint64_t)blockIdx.x * kReplaceWaves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kReplaceWaves) {
        const uint64_t g0 = grp << 6;
        csr_group_offsets(a.match_off, a.in_off, a.n_rows, g0, lane, mo, ino);
        sum[lane] = 0ull;
        csr_wave_sync();
        const uint64_t m0 = mo[0], m1 = mo[64];
        for (uint64_t m = m0 + (uint64_t)lane; m < m1; m += 64u) {
            const uint32_t r = csr_row_of(mo, m);
            uint64_t s, e;
            replace_match(a, ino, m, r, &s, &e);
            atomicAdd(&sum[r], (unsigned long long)(e - s));
        }
        csr_wave_sync();
        if (g0 + (uint64_t)lane < a.n_rows) {
            const uint64_t len = ino[lane + 1] - ino[lane], c = mo[lane + 1] - mo[lane];
            const uint64_t gone = sum[lane] < len ? sum[lane] : len;
            a.out_len[g0 + (uint64_t)lane] = len - gone + c * (uint64_t)a.repl_len;
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

template <int CW>
__global__ __launch_bounds__(kReplaceWaves * 64) void replace_fill_kernel(const ReplaceArgs a) {
    using T = std::conditional_t<CW == 1, uint8_t, uint16_t>;
    constexpr uint32_t K = kReplaceChunk;
    __shared__ __attribute__((aligned(16))) uint8_t s_repl[kReplaceMaxUnits * 2];
    __shared__ uint64_t s_mo[kReplaceWaves][65], s_ino[kReplaceWaves][65];
    __shared__ uint64_t s_O[kReplaceWaves][K + 1]; // O of the chunk's matches; entry nk: the next chunk's first O, or the end of the group
    __shared__ uint64_t s_D[kReplaceWaves][K];     // D behind match k (the gap that follows it)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave], *O = s_O[wave], *Dn = s_D[wave];

    const uint64_t RB = (uint64_t)a.repl_len * CW; // replacement bytes
    for (uint32_t i = threadIdx.x * 16u; i < (uint32_t)RB; i += kReplaceWaves * 64u * 16u) *(rp_u32x4 *)(s_repl + i) = *(const rp_u32x4 *)(a.repl + i);
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
        const uint64_t in_b = replace_clamp(ino[0], in_first, in_last), out_b = replace_clamp(out_g0, out_first, out_last);
        const uint64_t inB = dbase + in_b * CW, inE = dbase + replace_clamp(ino[64], in_b, in_last) * CW;
        const uint64_t outB = obase + out_b * CW, outE = obase + replace_clamp(out_g1, out_b, out_last) * CW;
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
                if (k < nk) {
                    const uint64_t m = mb + k;
                    const uint32_t r = csr_row_of(mo, m);
                    uint64_t s, e;
                    replace_match(a, ino, m, r, &s, &e);
                    I = dbase + (ino[r] + s) * CW;
                    delta = (long long)RB - (long long)((e - s) * CW);
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
                }
                D += (uint64_t)__shfl(incl, 63, 64);
            }
            if (lane == 0) {
                uint64_t I = inE;
                if (!last) {
                    const uint64_t m = mb + nk;
                    const uint32_t r = csr_row_of(mo, m);
                    uint64_t s, e;
                    replace_match(a, ino, m, r, &s, &e);
                    I = dbase + (ino[r] + s) * CW;
                }
                O[nk] = I + D;
            }
            csr_wave_sync();
            const uint64_t hi = last ? outE : replace_clamp(O[nk], lo, outE);

            // ---- sweep the chunk's output range [lo, hi): 64 lanes x 16 bytes a step.  A lane's 16 bytes are put together piece by piece
            // -- a gap of the input, or a replacement -- each piece fetched as if it filled the whole block (two aligned 16-byte loads
            // around the gap's misaligned source, or the replacement's dwords out of LDS, and a funnel shift) and its own bytes merged
            // under a byte mask.  A block inside one gap -- nearly all of them -- is one round of this; the wave makes as many rounds
            // as its block with the most pieces has.
            uint32_t step0 = 0; // the binary search's first step: the largest power of two <= nk (wave-uniform)
            if (nk) step0 = 1u << (31u - (uint32_t)__builtin_clz(nk));
            for (uint64_t X = (lo & ~(uint64_t)15) + (uint64_t)lane * 16u; X < hi; X += 1024u) {
                const uint64_t x0 = X > lo ? X : lo, x1 = X + 16u < hi ? X + 16u : hi;
                if (x0 >= x1) continue; // (an empty range that begins inside a 16-byte block)
                uint32_t jj = 0;        // the chunk's matches with O <= x
                for (uint32_t step = step0; step; step >>= 1)
                    if (jj + step <= nk && O[jj + step - 1u] <= x0) jj += step;
                uint64_t Oprev = jj ? O[jj - 1u] : 0ull, Dcur = jj ? Dn[jj - 1u] : Dpre, Onext = O[jj];
                bool any = jj != 0u;
                uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
                uint64_t x = x0;
                do {
                    while (jj < nk && Onext <= x) { // the matches that begin at or before x (several: touching or empty ones)
                        Oprev = Onext;
                        Dcur = Dn[jj];
                        ++jj;
                        Onext = O[jj];
                        any = true;
                    }
                    const uint64_t rel = x - Oprev;
                    uint64_t pe; // the piece at x ends here: always beyond x
                    uint32_t t0, t1, t2, t3, t4, sh;
                    if (any && rel < RB) { // inside replacement jj - 1: the dwords of the replacement around byte (X - Oprev), which may be < 0
                        pe = Oprev + RB < x1 ? Oprev + RB : x1;
                        const int64_t r0 = (int64_t)(X - Oprev);
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
                        rp_u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
                        // (an aligned block is loaded only when it holds a byte of the group's input span -- the piece's own bytes always do)
                        if (P0 < inE && P1 > inB && P1 > P0) v0 = *(const RP_GLOBAL rp_u32x4 *)(uintptr_t)P0;
                        if (kb && P1 < inE && P1 + 16u > inB && P1 + 16u > P1) v1 = *(const RP_GLOBAL rp_u32x4 *)(uintptr_t)P1;
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
                    const rp_u32x4 w = {w0, w1, w2, w3};
                    *(RP_GLOBAL rp_u32x4 *)(uintptr_t)X = w;
                } else { // an edge of the chunk's range, shared with another wave or with the caller's memory: the own units only
                    const uint32_t ww[4] = {w0, w1, w2, w3};
#pragma unroll
                    for (uint32_t b = 0; b < 16u; b += CW) {
                        const uint64_t xb = X + b;
                        if (xb >= x0 && xb < x1) *(RP_GLOBAL T *)(uintptr_t)xb = (T)(ww[b >> 2] >> ((b & 3u) * 8u));
                    }
                }
            }
            lo = hi;
            csr_wave_sync(); // (the next chunk, or the next group, overwrites the tables)
            if (last) break;
        }
    }
}

// The replacement out of kernel arguments into device memory: what the host passes is copied when the launch is made, so the caller's
// buffer is free when the entry returns, with no host synchronisation and no staging buffer to keep alive.
__global__ __launch_bounds__(256) void replace_put_kernel(const ReplacePiece piece, uint8_t *dst, uint32_t n) {
    for (uint32_t i = threadIdx.x; i < n; i += 256u) dst[i] = piece.b[i];
}

static int replace_grid(uint64_t n_rows, int n_cus) {
    const uint64_t blocks = ((n_rows + 63u) / 64u + kReplaceWaves - 1u) / kReplaceWaves;
    const uint64_t cap = (uint64_t)(n_cus > 0 ? n_cus : 1) * 16u;
    return (int)(blocks < cap ? blocks : cap);
}

hipError_t launch_replace_put(const void *repl_host, uint32_t bytes, uint8_t *d_repl, hipStream_t stream) {
    for (uint32_t at = 0; at < bytes; at += kReplacePutBytes) {
        ReplacePiece piece;
        const uint32_t n = bytes - at < kReplacePutBytes ? bytes - at : kReplacePutBytes;
        memcpy(piece.b, (const uint8_t *)repl_host + at, n);
        memset(piece.b + n, 0, kReplacePutBytes - n);
        hipLaunchKernelGGL(replace_put_kernel, dim3(1), dim3(256), 0, stream, piece, d_repl + at, n);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_replace_lengths(const ReplaceArgs &a, int n_cus, hipStream_t stream) {
    hipLaunchKernelGGL(replace_lengths_kernel, dim3(replace_grid(a.n_rows, n_cus)), dim3(kReplaceWaves * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_replace_fill(const ReplaceArgs &a, int n_cus, hipStream_t stream) {
    const dim3 grid(replace_grid(a.n_rows, n_cus)), block(kReplaceWaves * 64);
    if (a.cw == 1) hipLaunchKernelGGL(replace_fill_kernel<1>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(replace_fill_kernel<2>, grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace needle
