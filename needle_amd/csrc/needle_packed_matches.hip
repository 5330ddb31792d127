// Instantiations of the packed-rows scan kernel for matches() (DFAClassBuilder.createMatchesMethod :854-912).
#include "needle_packed.h"
namespace needle {
hipError_t launch_packed_matches(const PackedArgs &a, int cw, PackedShape sh, hipStream_t s) {
    return cw == 1 ? launch_packed_m<OP_MATCHES, 1>(a, sh, s) : launch_packed_m<OP_MATCHES, 2>(a, sh, s);
}
} // namespace needle
