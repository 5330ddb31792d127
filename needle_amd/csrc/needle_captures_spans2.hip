// Instantiation of the capture kernel of span lists (needle_captures_spans.h) for UTF-16 rows; its launcher.  Shape: as many waves per
// workgroup (at most 16) as have room for their offsets and slot files behind the program; persistent workgroups, two per CU where two
// fit the LDS -- the loads are scattered 16-byte blocks, so it is waves in flight that hide their latency.
#include "needle_captures_spans.h"
#include "needle_launch.h"
namespace needle {
hipError_t launch_captures_spans1(const CapSpansArgs &a, int grid, int waves, size_t lds, hipStream_t s);

hipError_t launch_captures_spans(int char_width, const CapSpansArgs &a, int n_cus, hipStream_t stream) {
    if (a.n_rows == 0) return hipSuccess;
    const uint32_t prog = a.hdr.lds_bytes, per_wave = cap_wave_lds(a.hdr.n_slots);
    if ((prog & 15u) != 0u || prog + per_wave > kCapLdsBytes) return hipErrorInvalidValue;
    uint32_t waves = (kCapLdsBytes - prog) / per_wave;
    if (waves > (uint32_t)kWavesPerBlock) waves = (uint32_t)kWavesPerBlock;
    const size_t lds = (size_t)prog + (size_t)waves * per_wave;
    const uint64_t n_groups = (a.n_rows + 63u) >> 6;
    uint64_t blocks = (n_groups + waves - 1u) / waves;
    const uint64_t cap = (uint64_t)(n_cus > 0 ? n_cus : 1) * (lds * 2u <= kCapLdsBytes ? 2u : 1u);
    if (blocks > cap) blocks = cap;
    return char_width == 1 ? launch_captures_spans1(a, (int)blocks, (int)waves, lds, stream) : launch_captures_spans_cw<2>(a, (int)blocks, (int)waves, lds, stream);
}
} // namespace needle
