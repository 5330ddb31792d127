// Regex -> reference-layout tables (the role DFACompiler.compileToBytes plays up to the point where it
// hands four DFAs to DFAClassBuilder: needle-compiler/.../DFACompiler.java:45-65).
#pragma once
#include <string>
#include <utility>
#include <vector>
#include "needle_lower.h"

namespace needle {

// Returns a NEEDLE_* status (include/needle_hip.h); on failure `err` holds the message.
int compile_regex(const std::u16string &regex, int flags, RefTables &out, std::string &err);

// The second parse, with capturing groups kept (needle_captures.h): the priority Thompson program of the regex.  compile_regex's own
// parse, its tables and their numbering do not pass through here.
//   CAP_CSET   one char of `ranges` (inclusive, sorted, disjoint), then pc + 1
//   CAP_SPLIT  x before y
//   CAP_JMP    x
//   CAP_SAVE   tag x (group g >= 1: start = 2 (g - 1), end = 2 (g - 1) + 1), then pc + 1
//   CAP_MATCH
enum CapOp : int { CAP_CSET, CAP_SPLIT, CAP_JMP, CAP_SAVE, CAP_MATCH };
struct CapInstr {
    int op = CAP_MATCH, x = -1, y = -1;
    std::vector<std::pair<int, int>> ranges;
};
struct CapNfa {
    int n_groups = 0;           // numbered by opening parenthesis; (?<name> counts, (?: does not
    bool nullable_loop = false; // some `*`, `+` or {m,n} with n > 1 has a body that can match the empty string: no program
    bool too_big = false;       // more than max_instrs instructions: no program
    std::vector<CapInstr> prog;
};
int build_captures_nfa(const std::u16string &regex, int flags, size_t max_instrs, CapNfa &out, std::string &err);

} // namespace needle
