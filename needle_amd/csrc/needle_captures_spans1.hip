// Instantiation of the capture kernel of span lists (needle_captures_spans.h) for 8-bit rows.
#include "needle_captures_spans.h"
namespace needle {
hipError_t launch_captures_spans1(const CapSpansArgs &a, int grid, int waves, size_t lds, hipStream_t s) { return launch_captures_spans_cw<1>(a, grid, waves, lds, s); }
} // namespace needle
