// Instantiations of the pattern-set kernel of packed rows (needle_packed_set.h) for 8-bit rows.
#include "needle_packed_set.h"
namespace needle {
hipError_t launch_packed_set1(int op, const PackedSetArgs &a, PackedShape sh, hipStream_t s) { return launch_packed_set_cw<1>(op, a, sh, s); }
} // namespace needle
