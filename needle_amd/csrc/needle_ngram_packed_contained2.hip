// needle_ngram_packed_contained2.hip -- the packed-rows filter kernel (needle_ngram_packed.h): OP_CONTAINED_IN, char width 2.
#include "needle_ngram_packed.h"
namespace needle {
hipError_t launch_ngram_packed_contained2(const NgramArgs &A, int n_cus, size_t lds, hipStream_t s) { return launch_ngp_m<OP_CONTAINED_IN, 2>(A, n_cus, lds, s); }
} // namespace needle
