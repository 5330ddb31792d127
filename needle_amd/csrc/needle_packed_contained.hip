// Instantiations of the packed-rows scan kernel for containedIn() (DFAClassBuilder.createContainedInMethod :956-1025).
#include "needle_packed.h"
namespace needle {
hipError_t launch_packed_contained_in(const PackedArgs &a, int cw, PackedShape sh, hipStream_t s) {
    return cw == 1 ? launch_packed_m<OP_CONTAINED_IN, 1>(a, sh, s) : launch_packed_m<OP_CONTAINED_IN, 2>(a, sh, s);
}
} // namespace needle
