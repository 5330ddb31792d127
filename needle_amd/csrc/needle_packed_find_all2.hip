// Instantiations of the packed-rows find-all kernel for UTF-16 rows; its shape and launcher (one persistent workgroup per CU, the
// shape from the transducer's LDS footprint as launch_find_all_lockstep chooses it).
#include "needle_packed_find_all.h"
#include "needle_launch.h"
namespace needle {
hipError_t launch_packed_find_all1(const PackedFindAllArgs &a, int chb, int grid, int waves, size_t lds, hipStream_t s);

bool packed_find_all_shape(uint32_t prog_lds_bytes, int char_width, int *waves, int *chb) {
    const size_t p = (prog_lds_bytes + 15u) & ~15u, cap = 160u * 1024u;
    static const int cand[7][2] = {{16, 128}, {16, 64}, {14, 64}, {12, 64}, {10, 64}, {8, 64}, {4, 64}};
    for (const auto &c : cand)
        if ((char_width == 2 || c[1] == 64) && p + (size_t)c[0] * 64 * c[1] <= cap) {
            *waves = c[0];
            *chb = c[1];
            return true;
        }
    return false;
}

hipError_t launch_packed_find_all(int char_width, const PackedFindAllArgs &a, int n_cus, hipStream_t stream) {
    if (a.f.s.n_rows == 0) return hipSuccess;
    int waves = 0, chb = 0;
    if (!a.f.s.hdr.ft_on || !packed_find_all_shape(a.f.s.hdr.lds_bytes, char_width, &waves, &chb)) return hipErrorInvalidValue;
    const uint64_t n_groups = (a.f.s.n_rows + 63) >> 6;
    uint64_t blocks = (n_groups + waves - 1) / waves;
    if (blocks > (uint64_t)n_cus) blocks = (uint64_t)n_cus;
    const size_t lds = ((a.f.s.hdr.lds_bytes + 15u) & ~15u) + (size_t)waves * 64 * chb;
    if (char_width == 1) return launch_packed_find_all1(a, chb, (int)blocks, waves, lds, stream);
    return launch_packed_find_all_w<2>(a, chb, (int)blocks, waves, lds, stream);
}
} // namespace needle
