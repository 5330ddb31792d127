// The per-lane find-all kernel of packed UTF-16 rows (needle_packed_find_all_lane.h), its shape and its launcher.
#include "needle_packed_find_all_lane.h"
#include "needle_launch.h"
namespace needle {
hipError_t launch_packed_find_all_lane1(const PackedFindAllArgs &a, int chb, int grid, int waves, size_t lds, hipStream_t s);

bool packed_find_all_lane_mode(uint32_t mode) { return mode == MODE_PACK || mode == MODE_TABLE8 || mode == MODE_TABLE16; }

bool packed_find_all_lane_shape(uint32_t prog_lds_bytes, int char_width, int *waves, int *chb) {
    (void)char_width; // (no candidate spills for either width)
    return find_all_lane_shape(prog_lds_bytes, waves, chb);
}

// One persistent workgroup per CU, as launch_packed_find_all.
hipError_t launch_packed_find_all_lane(int char_width, const PackedFindAllArgs &a, int n_cus, hipStream_t stream) {
    if (a.f.s.n_rows == 0) return hipSuccess;
    int waves = 0, chb = 0;
    if (!packed_find_all_lane_mode(a.f.s.hdr.mode) || !packed_find_all_lane_shape(a.f.s.hdr.lds_bytes, char_width, &waves, &chb)) return hipErrorInvalidValue;
    const uint64_t n_groups = (a.f.s.n_rows + 63) >> 6;
    uint64_t blocks = (n_groups + waves - 1) / waves;
    if (blocks > (uint64_t)n_cus) blocks = (uint64_t)n_cus;
    const size_t lds = ((a.f.s.hdr.lds_bytes + 15u) & ~15u) + (size_t)waves * 64 * chb;
    if (char_width == 1) return launch_packed_find_all_lane1(a, chb, (int)blocks, waves, lds, stream);
    return launch_packed_find_all_lane_m<2>(a, chb, (int)blocks, waves, lds, stream);
}
} // namespace needle
