// Instantiations of the packed-rows scan kernel for find() on UTF-16 rows; the launcher of the packed-rows scan (shape: the
// tiled scan's, from the automaton's LDS footprint -- a wave's window is the tile of that shape).
#include "needle_packed.h"
#include "needle_launch.h"
namespace needle {
hipError_t launch_packed_matches(const PackedArgs &a, int cw, PackedShape sh, hipStream_t s);
hipError_t launch_packed_contained_in(const PackedArgs &a, int cw, PackedShape sh, hipStream_t s);
hipError_t launch_packed_find1(const PackedArgs &a, PackedShape sh, hipStream_t s);
hipError_t launch_packed_next1(const PackedArgs &a, PackedShape sh, hipStream_t s);
hipError_t launch_packed_next2(const PackedArgs &a, PackedShape sh, hipStream_t s);
hipError_t launch_packed_forms1(const PackedArgs &a, PackedShape sh, hipStream_t s);
hipError_t launch_packed_forms2(const PackedArgs &a, PackedShape sh, hipStream_t s);

hipError_t launch_packed(int op, int char_width, const PackedArgs &a_in, int n_cus, hipStream_t stream) {
    if (a_in.s.n_rows == 0) return hipSuccess;
    PackedArgs a = a_in;
    PackedShape sh;
    int in_f = 0;
    if (!shape_for_program(a.s.hdr, char_width, &sh.waves, &sh.chb, &in_f)) return hipErrorInvalidValue;
    a.s.tiles_in_f_rows = (uint32_t)in_f;
    const bool cursors = op == OP_FIND && a.s.from != nullptr, forms = op == OP_FIND && a.s.packed != nullptr;
    if (cursors && packed_cursor_narrow(char_width, a.s.hdr.mode)) sh.chb = 64; // (needle_packed.h)
    const uint64_t n_groups = (a.s.n_rows + 63) >> 6;
    uint64_t blocks = (n_groups + sh.waves - 1) / sh.waves;
    if (blocks > (uint64_t)n_cus) blocks = (uint64_t)n_cus; // one persistent workgroup per CU
    sh.grid = (int)blocks;
    sh.lds = ((a.s.hdr.lds_bytes + 15u) & ~15u) + (size_t)(sh.waves - (in_f ? 4 : 0)) * 64 * sh.chb;
    switch (op) {
    case OP_MATCHES: return launch_packed_matches(a, char_width, sh, stream);
    case OP_CONTAINED_IN: return launch_packed_contained_in(a, char_width, sh, stream);
    default:
        if (cursors) return char_width == 1 ? launch_packed_next1(a, sh, stream) : launch_packed_next2(a, sh, stream);
        if (forms) return char_width == 1 ? launch_packed_forms1(a, sh, stream) : launch_packed_forms2(a, sh, stream);
        return char_width == 1 ? launch_packed_find1(a, sh, stream) : launch_packed_m<OP_FIND, 2>(a, sh, stream);
    }
}
} // namespace needle
