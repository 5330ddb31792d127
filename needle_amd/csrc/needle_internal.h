// What the library's translation units share besides the launchers (needle_launch.h): the error channel, the scratch pool, and the
// few internals the host-buffer layer (needle_host.cpp) needs beyond the public _dev entries.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "../../include/needle_hip.h"

namespace needle {

// needle_api.cpp: the calling thread's needle_last_error()
int set_error(int code, const std::string &msg);
inline int hip_fail(hipError_t e, const char *what) { return set_error(NEEDLE_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

// needle_api.cpp: the library's own stream-ordered memory pool
hipError_t scratch_malloc(void **out, size_t bytes, hipStream_t stream);
hipError_t scratch_free(void *p, hipStream_t stream);
hipError_t scratch_trim(size_t keep_bytes);

// needle_compact.hip: needle_find_compact_dev with row_base added to the row numbers written, so that the records of a host batch's
// chunks run on
int find_compact(const needle_pattern *p, const needle_batch_view *v, uint64_t *d_bitmap, needle_match_rec *d_recs, uint64_t cap,
                 uint64_t *d_n_matched, uint64_t row_base, void *stream);
// needle_api.cpp: NEEDLE_FIND_ALL_ROUNDS=1 (the round-per-match find-all forced)
bool find_all_rounds_forced();
// needle_api.cpp: NEEDLE_ERR_UNSUPPORTED where the set has no plan for this op (OP_MATCHES | OP_CONTAINED_IN) and char width (1 | 2)
int set_plan_usable(const needle_pattern_set *s, int op, int char_width);
// needle_api.cpp: the set's members (1 .. 32)
uint32_t set_pattern_count(const needle_pattern_set *s);
// needle_api.cpp: what the Matcher mirror reads of the pattern where the generated loops are skipped
struct MatcherRoots {
    bool forwards_root_accepts, backwards_root_accepts;
    int32_t fixed_len;
};
MatcherRoots matcher_roots(const needle_pattern *p);
// needle_api.cpp: the checks of a packed view that hold for host and device memory alike
int check_packed(const needle_packed_view *v);

} // namespace needle

#define HIP_TRY(expr)                                             \
    do {                                                          \
        hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return needle::hip_fail(_e, #expr); \
    } while (0)
