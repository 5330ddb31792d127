// Instantiations of the packed-rows scan kernel for find() on 8-bit rows (DFAClassBuilder.createFindMethodInternal :625-659,
// createIndexMethod :335-471, createIndexMethodReversed :529-586).
#include "needle_packed.h"
namespace needle {
hipError_t launch_packed_find1(const PackedArgs &a, PackedShape sh, hipStream_t s) { return launch_packed_m<OP_FIND, 1>(a, sh, s); }
} // namespace needle
