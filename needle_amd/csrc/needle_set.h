// Pattern sets: up to 32 patterns matched in ONE pass over a batch (needle_pattern_set, include/needle_hip.h).  Host side: the product
// automata of the members' reference tables and their grouping into plain LDS table programs; the kernel is needle_packed_set.h.
//
// Both products run over a COMBINED class map: two chars are in one combined class when every member agrees on its own class and
// on `c > max_char` of the automaton in question (classes numbered compactly, re-indexed after each member), so that the members'
// max_char rules are part of the product and it needs no OVER column.
//
//   matches() product.  Component i is a state of member i's W_MATCHES automaton, or dead: it dies on a -1 entry or on a char
//   above that automaton's max_char (DFAClassBuilder.java:892-910; the check is unconditional there).  mask[state] = the components
//   in accepting states, read ONCE, at the row's end.  All components dead = the sink (table entry -1).
//
//   containedIn() product, accept-OR form.  Component i is a state of member i's W_CONTAINED_IN automaton.  One step of one
//   component: standing in an accepting state it first returns to state 0 (its bit is in the row's mask already); then a char above
//   max_char (where max_char < 0xFFFF) gives state 0; otherwise the table entry, -1 giving 0 (DFAClassBuilder.java:1004-1022: the
//   killing char is consumed, not retried).  The row's mask is mask[start] OR-ed with mask[state] after EVERY char.  "Which members
//   have matched so far" is NOT part of the state: that product grows as 2^k (5944 states for eight log patterns where this
//   one has 145).
//
// Groups.  A product must stay a plain LDS table program (lower_pattern_set) within the caller's table budget.  Groups are built
// greedily in pattern order: the next member joins while the product -- its breadth-first construction aborted as soon as it
// exceeds the budget -- still fits, else it starts a new group.  A group is a run of consecutive member indices; its mask bits are
// the members' indices in the set.
#pragma once
#include <stdint.h>
#include <vector>
#include "needle_lower.h"

namespace needle {

struct SetGroup {
    int first = 0, count = 0; // members first .. first + count - 1 (mask bits first .. first + count - 1)
    SetProduct prod;
    Program prog;             // lower_pattern_set(prod)
};
struct SetPlan {
    std::vector<SetGroup> groups;
};

// The product of members[first .. first + count) for op (OP_MATCHES | OP_CONTAINED_IN) on rows of char_width, lowered within
// `budget` bytes of LDS.  false: it does not fit.
bool build_set_group(const std::vector<RefTables> &members, int first, int count, int op, int char_width, size_t budget, SetGroup *out);
// The greedy grouping of all members.  false: member *bad_index does not fit as a plain table on its own.
bool build_set_plan(const std::vector<RefTables> &members, int op, int char_width, size_t budget, SetPlan *out, int *bad_index);

} // namespace needle
