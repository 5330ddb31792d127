// Instantiations of the packed-rows scan kernel for find() from per-row cursors on UTF-16 rows (needle_find_next_packed_dev;
// DFAClassBuilder.java:616-659); window sizes: needle_packed.h packed_cursor_narrow.
#include "needle_packed.h"
namespace needle {
hipError_t launch_packed_next2(const PackedArgs &a, PackedShape sh, hipStream_t s) { return launch_packed_m<OP_FIND, 2, PK_CURSOR>(a, sh, s); }
} // namespace needle
