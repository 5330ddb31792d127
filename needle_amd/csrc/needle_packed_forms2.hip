// Instantiations of the packed-rows scan kernel for find() with one dword / uint16 per row on UTF-16 rows
// (needle_find_packed{16,8}_packed_dev; start() / end(): DFAClassBuilder.java:625-667).
#include "needle_packed.h"
namespace needle {
hipError_t launch_packed_forms2(const PackedArgs &a, PackedShape sh, hipStream_t s) { return launch_packed_m<OP_FIND, 2, PK_FORMS>(a, sh, s); }
} // namespace needle
