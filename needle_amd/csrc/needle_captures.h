// needle_captures.h -- the capture program of a pattern: the group spans of a full match of a span, as a tagged DFA
// that a lane walks with one column lookup and one table lookup per char (needle_captures_spans.h).
//
// Contract (include/needle_hip.h, needle_captures_spans_packed_dev): for a text t that the pattern matches whole, group g >= 1 is what
// a backtracking matcher reports for a full match of t -- the first path in priority order (alternation left before right; `*`, `+`,
// `?`, {m,n} one more iteration before stopping), each group its last passage on that path, a group never passed (-1, -1).
//
// Construction (needle_captures.cpp):
//   1. needle_regex.cpp parses the regex a second time with the groups kept and emits a priority Thompson program (CapNfa).
//   2. Determinisation.  A state is the ORDERED tuple of live program positions (char-set or MATCH instructions), highest priority
//      first; the closure is a depth-first walk in priority order in which the first visit of an instruction wins.  The state's k-th
//      thread owns the slots k * 2G .. k * 2G + 2G - 1 (G groups; tag 2 (g - 1) is group g's start, 2 (g - 1) + 1 its end).  A
//      transition lists the new state's threads as (old thread, tags passed in the closure): the new thread's slots are the old
//      thread's, with the passed tags set to the position behind the char.  Old -> new thread indices are order-preserving, so the
//      parallel copy is sequenced here: threads that move up in descending order, threads that move down in ascending order, the sets
//      last.  A transition that moves no thread and passes no tag has op list 0.  There is no lookahead: a loop that may be a
//      group's last piece (`[^ ]*` in front of a literal) makes the thread behind the loop anew on every iteration and sets the
//      group's end tag each time, so such chars do run an op list (profiles/captures.md: 78 % of the chars of a request line).
//      A thread that stays where it is keeps its slots untouched, so every slot of a live thread was written by the initial op list or
//      by a transition: nothing is cleared between spans but what the initial op list writes.
//   3. Lowering to a plain LDS program per char width (CapProgram).
//
// Refused (needle_captures_info.reason), never answered wrongly: a loop whose body can match the empty string (Perl-style matchers
// apply an empty-iteration rule there that a priority automaton does not reproduce), patterns without regex text, more than 16
// groups, programs that do not fit the LDS.  The construction stops at its budget: a 3000-keyword dictionary is refused at its first
// state.
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace needle {

constexpr int kCapMaxGroups = 16;          // NEEDLE_CAPTURES_MAX_GROUPS
constexpr uint32_t kCapMaxSlots = 128;     // slots of a lane (threads x 2G): 512 bytes per lane, 32 KiB per wave
constexpr uint32_t kCapMaxCols = 255;      // columns (uint8 column maps)
constexpr uint32_t kCapMaxStates = 16384;
constexpr uint32_t kCapMaxOps = 32768;     // op words of all lists
constexpr uint32_t kCapLdsBytes = 160u * 1024u;
constexpr uint32_t kCapWaveOffsets = 2u * 65u * 8u; // a wave's 65 span offsets + 65 row offsets (needle_csr_rows.h)
constexpr uint32_t kCapMinWaves = 2;       // the program and this many waves' offsets and slot files must fit the LDS

enum CapReason : int { CAP_OK = 0, CAP_NULLABLE_LOOP = 1, CAP_NO_REGEX = 2, CAP_TOO_MANY_GROUPS = 3, CAP_TOO_BIG = 4 };

// The tagged DFA on the host, as needle_pattern_captures_tables exports it.  State 0 is the sink, state `start` the initial one.
//   next[state * n_cols + col], op_id[state * n_cols + col]: the transition and its op list (0: none)
//   op list k: the pairs ops[2 * i], ops[2 * i + 1] = (dst slot, src) for i in [op_off[k], op_off[k + 1]), run in order;
//              src >= 0: a slot; kCapSrcPos: the position behind the char just read; kCapSrcNone: -1
//   init_op:   the op list run before the first char (position 0)
//   fin[state]: the first thread standing on MATCH (its slots are the groups), or -1
constexpr int32_t kCapSrcPos = -1, kCapSrcNone = -2;
struct CapTables {
    int reason = CAP_NO_REGEX;
    std::string why;
    int n_groups = 0, n_states = 0, n_cols = 0, max_threads = 0, n_slots = 0, n_op_lists = 0, start = 1, init_op = 0;
    std::vector<uint8_t> class_map; // 65536: char -> column
    std::vector<int32_t> next, op_id, op_off, ops, fin;
};

// What the kernel reads of the blob (all offsets in bytes, 16-byte aligned).
struct CapHeader {
    uint32_t n_states, n_cols, n_groups, n_slots, start, init_op;
    uint32_t lds_bytes;  // the whole blob (a multiple of 16)
    uint32_t off_cmap;   // char width 1: uint8 column[256]; char width 2: uint8 page_of[256]
    uint32_t off_pages;  // char width 2: uint8 column[n_pages][256]
    uint32_t off_table;  // uint32 [n_states][n_cols]: next state | op list << 16
    uint32_t off_opidx;  // uint32 [n_op_lists]: first op word | count << 20
    uint32_t off_ops;    // uint32 []: dst slot | src << 16 (kCapDevPos: the position behind the char, kCapDevNone: -1)
    uint32_t off_fin;    // int32 [n_states]
};
constexpr uint32_t kCapDevPos = 0xFFFFu, kCapDevNone = 0xFFFEu;
struct CapProgram {
    bool ok = false;
    CapHeader hdr{};
    std::vector<uint8_t> blob;
};

struct CapSpansArgs {
    const uint8_t *rows;        // the view's data (device, 4-byte aligned)
    const uint64_t *offsets;    // n_rows + 1 row offsets, in code units
    uint64_t n_rows;
    const uint8_t *prog;
    CapHeader hdr;
    const uint64_t *span_off;   // n_rows + 1
    const int32_t *start, *end; // relative to the row, in code units
    int32_t *gstart, *gend;     // planes: [g * plane_stride + m], g = 0 .. n_groups
    uint64_t plane_stride;
};
constexpr uint32_t cap_wave_lds(uint32_t n_slots) { return kCapWaveOffsets + n_slots * 256u; }

// The tables of `regex` (reason != CAP_OK: refused, `why` says so).  A NEEDLE_* status: anything but NEEDLE_OK means the second parse
// itself failed (it cannot where compile_regex accepted the regex).
int build_captures(const std::u16string &regex, int flags, CapTables &out, std::string &err);
// The LDS program for rows of `char_width`; !ok: it does not fit (CAP_TOO_BIG for this char width).
CapProgram lower_captures(const CapTables &t, int char_width);

} // namespace needle
