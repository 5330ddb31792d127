// needle_gather.hip -- gather a CSR list of spans of the rows of a PACKED batch into a new packed batch, hand-written for gfx950 (CDNA4):
// the kernels of needle_gather_spans_lengths_packed_dev / needle_gather_spans_fill_packed_dev / needle_split_spans_packed_dev
// (include/needle_hip.h).  Extract (the matches as rows), split (the text between them) and row selection are this one
// operation on three lists.
//
//   Lengths and split list: a wave owns a 64-row group (grid-stride), the group's 65 list offsets and 65 row offsets in its LDS
//   (needle_csr_rows.h); lanes are list entries, each finds its row by binary search and clamps its span into it.  The group's entries are
//   one contiguous range of the list, read and written coalesced; no atomics.
//   Fill: the spans of a 64-row group occupy ONE contiguous output range [out_off[m0], out_off[m1]), so a wave owns a group here too.
//   Everything is done in BYTES at absolute addresses, one body for both widths.  Per chunk of kGatherChunk spans the "piece table" in LDS:
//     O_k = the span's first output byte (non-decreasing: out_off is a prefix sum),  D_k = O_k - (its clamped source start):
//   output byte x of span k is the input at x - D_k.  The wave sweeps the chunk's OUTPUT range in steps of 64 lanes x one 16-byte
//   aligned block; a lane finds its block's first piece by binary search (the LAST k with O_k <= the block start: empty spans in front cost
//   nothing) and puts its 16 bytes together piece by piece -- each piece fetched as if it filled the whole block: two aligned 16-byte
//   loads around the misaligned source, a dword select and a v_alignbyte funnel shift, its own bytes merged under a byte mask.  The wave
//   makes as many rounds as its block with the most pieces: one for a long span, up to 16 for one-byte spans at char width 1.  A span
//   longer than a step is copied by the whole wave over several steps (needle_gather.h).
//   Stores: 16 bytes at once when all of them are the chunk's own, else code unit by code unit and ONLY the own units: neighbouring
//   groups' ranges meet at byte granularity, and the batch's first and last bytes border the caller's memory.
//   Loads: an aligned 16-byte block is loaded only when it holds a byte of the group's input span (the packed kernels' rule), zeros stand
//   in for any other: only blocks that spans touch are read, the rows are never streamed whole.  An out_off that is no prefix sum of the
//   lengths gives unspecified text, never an access outside the spans: every store is inside [out_off[M0], out_off[M1]).
//
// The sweep is needle_replace.hip's with the replacement branch and the running prefix sum taken out.  It is a copy, not a shared header:
// the replace kernels' register allocation (scripts/kernel_resources.py) moves with every line of their loop body, and this loop is the
// shorter one.
#include <hip/hip_runtime.h>
#include <type_traits>

#include "needle_csr_rows.h"
#include "needle_gather.h"
#include "needle_launch.h"

namespace needle {

typedef uint32_t ga_u32x4 __attribute__((ext_vector_type(4)));
// Text addresses are computed as integers; loads and stores through them name the GLOBAL address space, so that they are global_*
// instructions: flat ones count on the LDS counter too and every piece-table read would wait for the loads in flight.
#define GA_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ uint64_t gather_clamp(uint64_t x, uint64_t lo, uint64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

__global__ __launch_bounds__(kGatherWaves * 64) void gather_lengths_kernel(const GatherArgs a) {
    __shared__ uint64_t s_mo[kGatherWaves][65], s_ino[kGatherWaves][65];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave];
    const uint64_t n_groups = (a.n_rows + 63u) >> 6;
    for (uint64_t grp = (uint64_t)blockIdx.x * kGatherWaves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kGatherWaves) {
        const uint64_t g0 = grp << 6;
        csr_group_offsets(a.span_off, a.in_off, a.n_rows, g0, lane, mo, ino);
        csr_wave_sync();
        const uint64_t m0 = mo[0], m1 = mo[64];
        for (uint64_t m = m0 + (uint64_t)lane; m < m1; m += 64u) {
            const uint32_t r = csr_row_of(mo, m);
            uint64_t s, e;
            csr_clamp(a.start[m], a.end[m], ino[r + 1] - ino[r], &s, &e);
            a.out_len[m] = e - s;
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

// The complement of a match list: row r's c matches give c + 1 pieces at piece_off[r] = (match_off[r] - match_off[0]) + r; the group's
// pieces are one contiguous range of the piece list.  A lane is a piece.
__global__ __launch_bounds__(kGatherWaves * 64) void split_spans_kernel(const GatherArgs a) {
    __shared__ uint64_t s_mo[kGatherWaves][65], s_ino[kGatherWaves][65];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave];
    const uint64_t n = a.n_rows, n_groups = (n + 63u) >> 6;
    const uint64_t M0 = a.span_off[0];
    for (uint64_t grp = (uint64_t)blockIdx.x * kGatherWaves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kGatherWaves) {
        const uint64_t g0 = grp << 6;
        csr_group_offsets(a.span_off, a.in_off, n, g0, lane, mo, ino);
        csr_wave_sync();
        const uint64_t rows = n - g0 < 64u ? n - g0 : 64u;
        const uint64_t m0 = mo[0], m1 = mo[64] > m0 ? mo[64] : m0;
        if ((uint64_t)lane < rows) a.piece_off[g0 + (uint64_t)lane] = (mo[lane] - M0) + g0 + (uint64_t)lane;
        if (lane == 0 && g0 + 64u >= n) a.piece_off[n] = (m1 - M0) + n;
        const uint64_t total = (m1 - m0) + rows, first = (m0 - M0) + g0;
        for (uint64_t j = (uint64_t)lane; j < total; j += 64u) {
            uint32_t r = 0; // the last row whose first piece is at or before j: (mo[r] - m0) + r is increasing in r
#pragma unroll
            for (uint32_t step = 32; step; step >>= 1)
                if ((mo[r + step] - m0) + (uint64_t)(r + step) <= j) r += step;
            const uint64_t k = j - ((mo[r] - m0) + (uint64_t)r), c = mo[r + 1] - mo[r], len = ino[r + 1] - ino[r];
            uint64_t ps = 0, pe = len, s, e;
            if (k != 0) {
                csr_clamp(a.start[mo[r] + k - 1u], a.end[mo[r] + k - 1u], len, &s, &e);
                ps = e;
            }
            if (k != c) {
                csr_clamp(a.start[mo[r] + k], a.end[mo[r] + k], len, &s, &e);
                pe = s;
            }
            if (pe < ps) pe = ps;
            a.piece_start[first + j] = (int32_t)ps;
            a.piece_end[first + j] = (int32_t)pe;
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

template <int CW>
__global__ __launch_bounds__(kGatherWaves * 64) void gather_fill_kernel(const GatherArgs a) {
    using T = std::conditional_t<CW == 1, uint8_t, uint16_t>;
    constexpr uint32_t K = kGatherChunk;
    __shared__ uint64_t s_mo[kGatherWaves][65], s_ino[kGatherWaves][65];
    __shared__ uint64_t s_O[kGatherWaves][K + 1]; // O of the chunk's spans; entry nk: the next chunk's first O, or the end of the group
    __shared__ uint64_t s_D[kGatherWaves][K];     // D of span k: its output address minus its source address
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave], *O = s_O[wave], *Dn = s_D[wave];

    const uint64_t n = a.n_rows, n_groups = (n + 63u) >> 6;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.data, obase = (uint64_t)(uintptr_t)a.out;
    const uint64_t M0 = a.span_off[0], M1 = a.span_off[n] > M0 ? a.span_off[n] : M0;
    const uint64_t in_first = a.in_off[0], in_last = a.in_off[n];
    const uint64_t out_first = a.out_off[M0], out_last = a.out_off[M1] > out_first ? a.out_off[M1] : out_first;
    for (uint64_t grp = (uint64_t)blockIdx.x * kGatherWaves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kGatherWaves) {
        const uint64_t g0 = grp << 6;
        csr_group_offsets(a.span_off, a.in_off, n, g0, lane, mo, ino);
        csr_wave_sync();
        const uint64_t m0 = gather_clamp(mo[0], M0, M1), m1 = gather_clamp(mo[64], m0, M1);
        if (m1 > m0) {
            // the group's spans as absolute byte addresses, inside the batch's
            const uint64_t in_b = gather_clamp(ino[0], in_first, in_last), out_b = gather_clamp(a.out_off[m0], out_first, out_last);
            const uint64_t inB = dbase + in_b * CW, inE = dbase + gather_clamp(ino[64], in_b, in_last) * CW;
            const uint64_t outB = obase + out_b * CW, outE = obase + gather_clamp(a.out_off[m1], out_b, out_last) * CW;
            uint64_t lo = outB;
            for (uint64_t mb = m0; mb < m1; mb += K) {
                const uint32_t nk = (uint32_t)(m1 - mb < (uint64_t)K ? m1 - mb : (uint64_t)K);
                const bool last = mb + nk >= m1;
                // ---- the chunk's piece table
                for (uint32_t k = (uint32_t)lane; k < nk; k += 64u) {
                    const uint64_t m = mb + k;
                    const uint32_t r = csr_row_of(mo, m);
                    uint64_t s, e;
                    csr_clamp(a.start[m], a.end[m], ino[r + 1] - ino[r], &s, &e);
                    const uint64_t Ok = obase + a.out_off[m] * CW;
                    O[k] = Ok;
                    Dn[k] = Ok - (dbase + (ino[r] + s) * CW); // (mod 2^64)
                }
                if (lane == 0) O[nk] = obase + a.out_off[mb + nk] * CW;
                csr_wave_sync();
                const uint64_t hi = last ? outE : gather_clamp(O[nk], lo, outE);

                // ---- sweep the chunk's output range [lo, hi): 64 lanes x 16 bytes a step
                const uint32_t step0 = 1u << (31u - (uint32_t)__builtin_clz(nk)); // the binary search's first step (wave-uniform; nk >= 1)
                for (uint64_t X = (lo & ~(uint64_t)15) + (uint64_t)lane * 16u; X < hi; X += 1024u) {
                    const uint64_t x0 = X > lo ? X : lo, x1 = X + 16u < hi ? X + 16u : hi;
                    if (x0 >= x1) continue; // (an empty range that begins inside a 16-byte block)
                    uint32_t jj = 0;        // the chunk's spans with O <= x
                    for (uint32_t step = step0; step; step >>= 1)
                        if (jj + step <= nk && O[jj + step - 1u] <= x0) jj += step;
                    uint64_t Dcur = jj ? Dn[jj - 1u] : 0ull, Onext = O[jj];
                    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
                    uint64_t x = x0;
                    do {
                        while (jj < nk && Onext <= x) { // the spans that begin at or before x (several: empty ones)
                            Dcur = Dn[jj];
                            ++jj;
                            Onext = O[jj];
                        }
                        const uint64_t pe = jj < nk && Onext < x1 ? Onext : x1; // the piece at x ends here: always beyond x
                        const uint64_t A = X - Dcur;
                        const uint32_t kb = (uint32_t)A & 15u;
                        const uint64_t P0 = A - kb, P1 = P0 + 16u;
                        ga_u32x4 v0 = {0u, 0u, 0u, 0u}, v1 = {0u, 0u, 0u, 0u};
                        // (an aligned block is loaded only when it holds a byte of the group's input span -- the piece's own bytes always do)
                        if (P0 < inE && P1 > inB && P1 > P0) v0 = *(const GA_GLOBAL ga_u32x4 *)(uintptr_t)P0;
                        if (kb && P1 < inE && P1 + 16u > inB && P1 + 16u > P1) v1 = *(const GA_GLOBAL ga_u32x4 *)(uintptr_t)P1;
                        const bool q2 = (kb & 8u) != 0u, q1 = (kb & 4u) != 0u;
                        uint32_t u0 = v0[0], u1 = v0[1], u2 = v0[2], u3 = v0[3], u4 = v1[0], u5 = v1[1], u6 = v1[2], u7 = v1[3];
                        u0 = q2 ? u2 : u0, u1 = q2 ? u3 : u1, u2 = q2 ? u4 : u2, u3 = q2 ? u5 : u3, u4 = q2 ? u6 : u4, u5 = q2 ? u7 : u5;
                        const uint32_t t0 = q1 ? u1 : u0, t1 = q1 ? u2 : u1, t2 = q1 ? u3 : u2, t3 = q1 ? u4 : u3, t4 = q1 ? u5 : u4;
                        const uint32_t sh = kb & 3u;
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
                        const ga_u32x4 w = {w0, w1, w2, w3};
                        *(GA_GLOBAL ga_u32x4 *)(uintptr_t)X = w;
                    } else { // an edge of the chunk's range, shared with another wave or with the caller's memory: the own units only
                        const uint32_t ww[4] = {w0, w1, w2, w3};
#pragma unroll
                        for (uint32_t b = 0; b < 16u; b += CW) {
                            const uint64_t xb = X + b;
                            if (xb >= x0 && xb < x1) *(GA_GLOBAL T *)(uintptr_t)xb = (T)(ww[b >> 2] >> ((b & 3u) * 8u));
                        }
                    }
                }
                lo = hi;
                csr_wave_sync(); // (the next chunk overwrites the tables)
            }
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

static int gather_grid(uint64_t n_rows, int n_cus) {
    const uint64_t blocks = ((n_rows + 63u) / 64u + kGatherWaves - 1u) / kGatherWaves;
    const uint64_t cap = (uint64_t)(n_cus > 0 ? n_cus : 1) * 16u;
    return (int)(blocks < cap ? blocks : cap);
}

hipError_t launch_gather_lengths(const GatherArgs &a, int n_cus, hipStream_t stream) {
    hipLaunchKernelGGL(gather_lengths_kernel, dim3(gather_grid(a.n_rows, n_cus)), dim3(kGatherWaves * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_split_spans(const GatherArgs &a, int n_cus, hipStream_t stream) {
    hipLaunchKernelGGL(split_spans_kernel, dim3(gather_grid(a.n_rows, n_cus)), dim3(kGatherWaves * 64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_gather_fill(const GatherArgs &a, int n_cus, hipStream_t stream) {
    const dim3 grid(gather_grid(a.n_rows, n_cus)), block(kGatherWaves * 64);
    if (a.cw == 1) hipLaunchKernelGGL(gather_fill_kernel<1>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(gather_fill_kernel<2>, grid, block, 0, stream, a);
    return hipGetLastError();
}

uint32_t gather_chunk_spans() { return kGatherChunk; }

} // namespace needle
