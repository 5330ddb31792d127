// Instantiations of the pattern-set kernel of packed rows (needle_packed_set.h) for UTF-16 rows; its launcher (shape: the packed
// scan's, from the program's LDS footprint -- a wave's window is the tile of that shape).
#include "needle_packed_set.h"
#include "needle_launch.h"
namespace needle {
hipError_t launch_packed_set1(int op, const PackedSetArgs &a, PackedShape sh, hipStream_t s);

hipError_t launch_packed_set(int op, int char_width, const PackedSetArgs &a_in, int n_cus, hipStream_t stream) {
    if (a_in.p.s.n_rows == 0) return hipSuccess;
    if (op != OP_MATCHES && op != OP_CONTAINED_IN) return hipErrorInvalidValue;
    PackedSetArgs a = a_in;
    PackedShape sh;
    int in_f = 0;
    if (!shape_for_program(a.p.s.hdr, char_width, &sh.waves, &sh.chb, &in_f) || in_f) return hipErrorInvalidValue;
    a.p.s.tiles_in_f_rows = 0;
    const uint64_t n_groups = (a.p.s.n_rows + 63) >> 6;
    uint64_t blocks = (n_groups + sh.waves - 1) / sh.waves;
    if (blocks > (uint64_t)n_cus) blocks = (uint64_t)n_cus; // one persistent workgroup per CU
    sh.grid = (int)blocks;
    sh.lds = ((a.p.s.hdr.lds_bytes + 15u) & ~15u) + (size_t)sh.waves * 64 * sh.chb;
    return char_width == 1 ? launch_packed_set1(op, a, sh, stream) : launch_packed_set_cw<2>(op, a, sh, stream);
}
} // namespace needle
