// needle_ngram_packed_find_all1.hip -- the packed-rows filter kernel (needle_ngram_packed.h): OP_NG_FIND_ALL, char width 1.
#include "needle_ngram_packed.h"
namespace needle {
hipError_t launch_ngram_packed_find_all1(const NgramArgs &A, int n_cus, size_t lds, hipStream_t s) { return launch_ngp_m<OP_NG_FIND_ALL, 1>(A, n_cus, lds, s); }
} // namespace needle
