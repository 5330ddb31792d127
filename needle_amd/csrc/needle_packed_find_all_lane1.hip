// The per-lane find-all kernel of packed 8-bit rows (needle_packed_find_all_lane.h), in a translation unit of its own: it compiles in
// parallel with the UTF-16 one.
#include "needle_packed_find_all_lane.h"
namespace needle {
hipError_t launch_packed_find_all_lane1(const PackedFindAllArgs &a, int chb, int grid, int waves, size_t lds, hipStream_t s) {
    return launch_packed_find_all_lane_m<1>(a, chb, grid, waves, lds, s);
}
} // namespace needle
