// Instantiations of the packed-rows find-all kernel for UTF-16 rows; its shape and launcher (one persistent workgroup per CU, the
// shape from the transducer's LDS footprint: the lock-step kernels' one candidate list, needle_find_all_ls.hip).
#include "needle_packed_find_all.h"
#include "needle_launch.h"
namespace needle {
hipError_t launch_packed_find_all1(const PackedFindAllArgs &a, int chb, int grid, int waves, size_t lds, hipStream_t s);

// (8-bit rows: 64-byte windows per lane only, needle_packed_find_all.h)
bool packed_find_all_shape(uint32_t prog_lds_bytes, int char_width, int *waves, int *chb) {
    return find_all_lockstep_shape(prog_lds_bytes, char_width == 2, waves, chb);
}

hipError_t launch_packed_find_all(int char_width, const PackedFindAllArgs &a, int n_cus, hipStream_t stream) {
    if (a.f.s.n_rows == 0) return hipSuccess;
    int waves = 0, chb = 0, blocks = 0;
    size_t lds = 0;
    if (!a.f.s.hdr.ft_on || !packed_find_all_shape(a.f.s.hdr.lds_bytes, char_width, &waves, &chb)) return hipErrorInvalidValue;
    find_all_lockstep_grid(a.f.s.hdr.lds_bytes, a.f.s.n_rows, waves, chb, n_cus, &blocks, &lds);
    if (char_width == 1) return launch_packed_find_all1(a, chb, blocks, waves, lds, stream);
    return launch_packed_find_all_w<2>(a, chb, blocks, waves, lds, stream);
}
} // namespace needle
