// Instantiations of the pattern-set kernel of span lists (needle_set_spans.h) for 8-bit rows.
#include "needle_set_spans.h"
namespace needle {
hipError_t launch_set_spans1(const SetSpansArgs &a, int grid, int waves, size_t lds, hipStream_t s) { return launch_set_spans_cw<1>(a, grid, waves, lds, s); }
} // namespace needle
