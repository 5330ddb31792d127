// Instantiations of the packed-rows find-all kernel for 8-bit rows (the reference's repeated Matcher.find(),
// DFAClassBuilder.java:616-659).
#include "needle_packed_find_all.h"
namespace needle {
hipError_t launch_packed_find_all1(const PackedFindAllArgs &a, int chb, int grid, int waves, size_t lds, hipStream_t s) {
    return launch_packed_find_all_w<1>(a, chb, grid, waves, lds, s);
}
} // namespace needle
