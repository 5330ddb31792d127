// needle_group.hip -- equal spans of a CSR list over the rows of a PACKED batch put into groups, hand-written for gfx950 (CDNA4): the
// kernels of needle_group_spans_packed_dev (include/needle_hip.h).  grep -o | sort | uniq -c, GROUP BY regexp_extract,
// COUNT(DISTINCT ..), sort -u without the sort: per span the FIRST span with the same text and the size of its group.
//
//   Three launches on one stream; stream order is the only barrier between them.  No workgroup ever waits on another, and every loop
//   has a bound known at entry (the group's spans, the span's blocks, the table's slots, 64 lanes).
//   The text of a span is read as its CANONICAL 16-byte blocks -- bytes [16 j, 16 j + 16) of the span, whatever the span's alignment:
//   two aligned 16-byte loads around the misaligned source, a dword select and a v_alignbyte funnel shift (needle_gather.hip's), the
//   bytes behind the span's end masked to zero.  Hash and comparison both see canonical blocks only, so the same text at byte offset 3
//   and at byte offset 9 of its blocks hashes and compares alike.  An aligned block is loaded only when it holds a byte of the span
//   (the packed kernels' rule), with global_* loads, one block ahead of the one being used.
//   Pass 1, group_hash_kernel<CW>: gather_lengths_kernel's skeleton -- a wave owns a 64-row group (grid-stride), the group's 65 + 65
//   offsets in its LDS (needle_csr_rows.h), lanes are spans.  Per span i = m - M0 < max_spans: w_addr[i] the absolute byte address of
//   the clamped start, w_len[i] the length in bytes (kGroupAbsent for start < 0 and end < 0), w_hash[i] the hash of (text, length)
//   masked to hash_bits.  i >= max_spans: nothing is written but *status = 1.
//   Pass 2, group_insert_kernel: a lane is a span i (grid-stride over [0, min(M1 - M0, max_spans)), wave-contiguous, ascending with the
//   lane).  From slot hash & (slots - 1) on it visits at most `slots` slots: the word is read; an empty one is claimed with ONE
//   agent-scope compare-and-swap of 0 -> i + 1, and a failed swap hands back the occupant, which is treated like any occupant -- there
//   is no retry; against an occupant r the masked hashes and lengths of pass 1 (an earlier launch: visible) and then the canonical
//   blocks are compared.  Equal: this is the span's slot.  Every representative a slot ever holds carries the same text -- only spans
//   that compared equal lower the word -- so a stale read of the word still names a valid text.  When all lanes of the wave are done,
//   the wave's lanes with the same slot are combined (readlane of the first lane's slot + ballot: at most 64 rounds): the first of
//   them -- the smallest i -- adds their number to the slot's count and lowers the word to i + 1 by an unsigned min unless the word it
//   saw is smaller already.  A probe that runs out of slots sets *status and files kGroupNoSlot.
//   Pass 3, group_finish_kernel: first[m] = M0 + word[slot] - 1, count[m] = count[slot]; absent spans NEEDLE_GROUP_NONE / 0.
//   Exact and deterministic: equality is decided by the text; first is a minimum and count a sum of integers, neither depends on
//   which wave came first.
//   Limit: a span is hashed and compared by ONE lane (set_spans_kernel's limit): a long span runs at one lane's pace.
#include <hip/hip_runtime.h>

#include "needle_csr_rows.h"
#include "needle_group.h"
#include "needle_launch.h"

namespace needle {

typedef uint32_t gr_u32x4 __attribute__((ext_vector_type(4)));
// Text addresses are integers; loads through them name the GLOBAL address space (global_* instructions, not flat ones).
#define GR_GLOBAL __attribute__((address_space(1)))

// The low min(max(k, 0), 4) bytes of a dword.
__device__ __forceinline__ uint32_t group_below(int k) {
    const int c = k < 0 ? 0 : (k > 4 ? 4 : k);
    return c == 4 ? 0xFFFFFFFFu : (1u << (8 * c)) - 1u;
}

// A span's text as canonical 16-byte blocks.  b0: its first aligned block, kb: the span's first byte in it, nblk: aligned blocks that
// hold a byte of the span, ncb: canonical blocks.  cur / nxt: aligned blocks j and j + 1 (zeros where the span has none).
struct GroupReader {
    uint64_t b0;
    uint32_t kb, nblk, ncb, len;
    gr_u32x4 cur, nxt;

    __device__ __forceinline__ gr_u32x4 load(uint32_t k) const {
        gr_u32x4 v = {0u, 0u, 0u, 0u};
        if (k < nblk) v = *(const GR_GLOBAL gr_u32x4 *)(uintptr_t)(b0 + (uint64_t)k * 16u);
        return v;
    }
    __device__ __forceinline__ void open(uint64_t at, uint32_t len_bytes) {
        b0 = at & ~(uint64_t)15;
        kb = (uint32_t)at & 15u;
        len = len_bytes;
        nblk = len_bytes ? (uint32_t)(((uint64_t)kb + len_bytes + 15u) >> 4) : 0u;
        ncb = (uint32_t)(((uint64_t)len_bytes + 15u) >> 4);
        cur = load(0);
        nxt = load(1);
    }
    // Canonical block j (j < ncb; called for j = 0, 1, .. in turn): the bytes behind the span's end are zero.
    __device__ __forceinline__ gr_u32x4 block(uint32_t j) {
        const gr_u32x4 ahead = load(j + 2u); // its latency hides behind this block's work
        const bool q2 = (kb & 8u) != 0u, q1 = (kb & 4u) != 0u;
        uint32_t u0 = cur[0], u1 = cur[1], u2 = cur[2], u3 = cur[3], u4 = nxt[0], u5 = nxt[1], u6 = nxt[2], u7 = nxt[3];
        u0 = q2 ? u2 : u0, u1 = q2 ? u3 : u1, u2 = q2 ? u4 : u2, u3 = q2 ? u5 : u3, u4 = q2 ? u6 : u4, u5 = q2 ? u7 : u5;
        const uint32_t t0 = q1 ? u1 : u0, t1 = q1 ? u2 : u1, t2 = q1 ? u3 : u2, t3 = q1 ? u4 : u3, t4 = q1 ? u5 : u4;
        const uint32_t sh = kb & 3u;
        gr_u32x4 f = {__builtin_amdgcn_alignbyte(t1, t0, sh), __builtin_amdgcn_alignbyte(t2, t1, sh), __builtin_amdgcn_alignbyte(t3, t2, sh),
                      __builtin_amdgcn_alignbyte(t4, t3, sh)};
        if (j + 1u == ncb) { // the last block: its own bytes only
            const int rb = (int)(len - j * 16u); // 1 .. 16
            f[0] &= group_below(rb), f[1] &= group_below(rb - 4), f[2] &= group_below(rb - 8), f[3] &= group_below(rb - 12);
        }
        cur = nxt;
        nxt = ahead;
        return f;
    }
};

__device__ __forceinline__ uint64_t group_mix(uint64_t h, uint32_t lo, uint32_t hi) {
    h = (h ^ ((uint64_t)hi << 32 | lo)) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}

// The hash of (text, length): a fold over the canonical blocks, then murmur3's finalizer.
__device__ __forceinline__ uint64_t group_finalize(uint64_t h, uint32_t len) {
    h ^= len;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 33);
}

template <int CW>
__global__ __launch_bounds__(kGroupWaves * 64) void group_hash_kernel(const GroupArgs a) {
    __shared__ uint64_t s_mo[kGroupWaves][65], s_ino[kGroupWaves][65];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *mo = s_mo[wave], *ino = s_ino[wave];
    const uint64_t n_groups = (a.n_rows + 63u) >> 6;
    const uint64_t dbase = (uint64_t)(uintptr_t)a.data;
    const uint64_t M0 = a.span_off[0];
    for (uint64_t grp = (uint64_t)blockIdx.x * kGroupWaves + (uint64_t)wave; grp < n_groups; grp += (uint64_t)gridDim.x * kGroupWaves) {
        csr_group_offsets(a.span_off, a.in_off, a.n_rows, grp << 6, lane, mo, ino);
        csr_wave_sync();
        const uint64_t m0 = mo[0], m1 = mo[64];
        for (uint64_t mb = m0; mb < m1; mb += 64u) { // (wave-uniform)
            const uint64_t m = mb + (uint64_t)lane, i = m - M0;
            const bool in_list = m < m1, own = in_list && i < a.max_spans;
            if (in_list && !own) __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            GroupReader rd;
            rd.open(0, 0);
            uint64_t as = 0;
            bool absent = false;
            if (own) {
                const int32_t s32 = a.start[m], e32 = a.end[m];
                absent = s32 < 0 && e32 < 0;
                const uint32_t r = csr_row_of(mo, m);
                const uint64_t row = ino[r];
                uint64_t sc, ec;
                csr_clamp(s32, e32, ino[r + 1] - row, &sc, &ec);
                as = dbase + (row + sc) * CW;
                if (!absent) rd.open(as, (uint32_t)((ec - sc) * CW)); // (positions are int32: at most 2^32 - 2 bytes)
            }
            uint64_t h = 0x243F6A8885A308D3ull;
            uint32_t j = 0;
            while (__ballot(j < rd.ncb) != 0ull) { // (the wave goes on to its next 64 spans when all lanes are through)
                if (j < rd.ncb) {
                    const gr_u32x4 f = rd.block(j);
                    h = group_mix(group_mix(h, f[0], f[1]), f[2], f[3]);
                    ++j;
                }
            }
            if (own) {
                a.w_addr[i] = as;
                a.w_len[i] = absent ? kGroupAbsent : rd.len;
                a.w_hash[i] = group_finalize(h, rd.len) & a.hash_mask;
            }
        }
        csr_wave_sync(); // (the next group overwrites the offsets)
    }
}

// Are the texts of `len` bytes at xa and at xb the same?  Canonical block by canonical block.
__device__ __forceinline__ bool group_text_equal(uint64_t xa, uint64_t xb, uint32_t len) {
    if (xa == xb) return true;
    GroupReader ra, rb;
    ra.open(xa, len);
    rb.open(xb, len);
    for (uint32_t j = 0; j < ra.ncb; ++j) {
        const gr_u32x4 fa = ra.block(j), fb = rb.block(j);
        if (((fa[0] ^ fb[0]) | (fa[1] ^ fb[1]) | (fa[2] ^ fb[2]) | (fa[3] ^ fb[3])) != 0u) return false;
    }
    return true;
}

__global__ __launch_bounds__(kGroupWaves * 64) void group_insert_kernel(const GroupArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t M0 = a.span_off[0], M1 = a.span_off[a.n_rows];
    const uint64_t have = M1 > M0 ? M1 - M0 : 0ull, n = have < a.max_spans ? have : a.max_spans;
    const uint64_t smask = a.slots - 1u;
    const uint64_t stride = (uint64_t)gridDim.x * (kGroupWaves * 64);
    // (wave-uniform trip count: base is the wave's first span)
    for (uint64_t base = ((uint64_t)blockIdx.x * (kGroupWaves * 64) + (uint64_t)threadIdx.x) - (uint64_t)lane; base < n; base += stride) {
        const uint64_t i = base + (uint64_t)lane;
        uint32_t len = kGroupAbsent;
        if (i < n) len = a.w_len[i];
        const bool live = len != kGroupAbsent;
        uint64_t h = 0, at = 0;
        if (live) h = a.w_hash[i], at = a.w_addr[i];
        const uint32_t me = (uint32_t)i + 1u;
        uint64_t slot = h & smask, probes = 0;
        uint32_t seen = 0; // the word as this lane saw it when it found its slot
        bool done = !live;
        while (__ballot(!done && probes < a.slots) != 0ull) {
            if (!done && probes < a.slots) {
                uint32_t occ = __hip_atomic_load(&a.w_word[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (occ == 0u) { // empty: the one swap of this visit; a failed one hands back the occupant
                    if (__hip_atomic_compare_exchange_strong(&a.w_word[slot], &occ, me, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                        occ = me;
                }
                const uint64_t r = (uint64_t)occ - 1u; // (occ - 1 < n: only such values are ever stored)
                if (occ == me || (a.w_hash[r] == h && a.w_len[r] == len && group_text_equal(a.w_addr[r], at, len))) {
                    seen = occ;
                    done = true;
                } else {
                    slot = (slot + 1u) & smask;
                    ++probes;
                }
            }
        }
        const bool found = live && done;
        if (live && !done) {
            __hip_atomic_store(a.status, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.w_slot[i] = kGroupNoSlot;
        }
        if (found) a.w_slot[i] = slot;
        // the wave's lanes with the same slot: one add and at most one min for all of them, by the first (the smallest i)
        uint64_t todo = __ballot(found);
        while (todo != 0ull) { // (at most 64 rounds: every round takes its first lane out)
            const int first = __builtin_ctzll(todo);
            const uint32_t s_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)slot, first);
            const uint32_t s_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(slot >> 32), first);
            const uint64_t s = (uint64_t)s_hi << 32 | s_lo;
            const uint64_t same = __ballot(found && slot == s);
            if (lane == first) {
                __hip_atomic_fetch_add(&a.w_count[s], (uint32_t)__builtin_popcountll(same), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (me < seen) __hip_atomic_fetch_min(&a.w_word[s], me, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            todo &= ~same;
        }
    }
}

__global__ __launch_bounds__(kGroupWaves * 64) void group_finish_kernel(const GroupArgs a) {
    const uint64_t M0 = a.span_off[0], M1 = a.span_off[a.n_rows];
    const uint64_t have = M1 > M0 ? M1 - M0 : 0ull, n = have < a.max_spans ? have : a.max_spans;
    const uint64_t stride = (uint64_t)gridDim.x * (kGroupWaves * 64);
    for (uint64_t i = (uint64_t)blockIdx.x * (kGroupWaves * 64) + (uint64_t)threadIdx.x; i < n; i += stride) {
        uint64_t first = ~0ull; // NEEDLE_GROUP_NONE
        uint32_t count = 0;
        if (a.w_len[i] != kGroupAbsent) {
            const uint64_t s = a.w_slot[i];
            if (s < a.slots) {
                first = M0 + (uint64_t)a.w_word[s] - 1u;
                count = a.w_count[s];
            }
        }
        a.first[M0 + i] = first;
        a.count[M0 + i] = count;
    }
}

static int group_grid(uint64_t items, uint64_t per_block, int n_cus) {
    const uint64_t blocks = (items + per_block - 1u) / per_block;
    const uint64_t cap = (uint64_t)(n_cus > 0 ? n_cus : 1) * 16u;
    return (int)(blocks < 1u ? 1u : (blocks < cap ? blocks : cap));
}

hipError_t launch_group_spans(const GroupArgs &a, int n_cus, hipStream_t stream) {
    const dim3 block(kGroupWaves * 64);
    const dim3 rows_grid(group_grid((a.n_rows + 63u) / 64u, kGroupWaves, n_cus)), span_grid(group_grid(a.max_spans, kGroupWaves * 64, n_cus));
    if (a.cw == 1) hipLaunchKernelGGL(group_hash_kernel<1>, rows_grid, block, 0, stream, a);
    else hipLaunchKernelGGL(group_hash_kernel<2>, rows_grid, block, 0, stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(group_insert_kernel, span_grid, block, 0, stream, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(group_finish_kernel, span_grid, block, 0, stream, a);
    return hipGetLastError();
}

} // namespace needle
