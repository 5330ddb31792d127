// Product automata and grouping of pattern sets (needle_set.h).  Host code only.
#include "needle_set.h"
#include <string.h>
#include <unordered_map>
#include <string>
#include <utility>

namespace needle {

namespace {
// One member as the products step it: its automaton of the op, its class and "above max_char" per COMBINED class.
struct Member {
    const RefDfa *d;
    int stride;
    std::vector<uint8_t> cls;  // by combined class
    std::vector<uint8_t> over; // by combined class
};
} // namespace

bool build_set_group(const std::vector<RefTables> &members, int first, int count, int op, int char_width, size_t budget, SetGroup *out) {
    const Which which = op == OP_MATCHES ? W_MATCHES : W_CONTAINED_IN;
    const bool contained = op == OP_CONTAINED_IN;
    SetGroup g;
    g.first = first;
    g.count = count;
    SetProduct &sp = g.prod;

    // ---- the combined class map, refined member by member; keys re-indexed after each one (a product of keys overflows 64 bits at 8 members).
    // Only the chars a row of this width can hold are told apart: members that differ above 255 alone share their 8-bit columns and states.
    const int n_chars = char_width == 1 ? 256 : 65536;
    std::vector<uint16_t> cc(65536, 0);
    std::vector<int> rep(1, 0); // a char of every combined class
    for (int i = 0; i < count; ++i) {
        const RefTables &t = members[(size_t)first + i];
        const RefDfa &d = t.dfa[which];
        // (containedIn() tests max_char only where it is below 0xFFFF, matches() always: the same predicate on 16-bit chars)
        std::vector<uint16_t> ids(rep.size() << 9, 0xFFFFu); // by (combined class so far, member's class, above max_char)
        std::vector<int> nrep;
        for (int c = 0; c < n_chars; ++c) {
            const uint32_t key = (uint32_t)cc[c] << 9 | (uint32_t)t.class_map[c] << 1 | (c > d.max_char ? 1u : 0u);
            if (ids[key] == 0xFFFFu) {
                if (nrep.size() >= 254) return false; // (the column maps hold a column in a byte)
                ids[key] = (uint16_t)nrep.size();
                nrep.push_back(c);
            }
            cc[c] = ids[key];
        }
        rep.swap(nrep);
    }
    const int N = (int)rep.size();
    sp.n_classes = N;
    sp.class_map.resize(65536);
    for (int c = 0; c < 65536; ++c) sp.class_map[c] = (uint8_t)cc[c];
    const size_t front = pattern_set_front_bytes(sp, char_width); // (the classes are final: the column maps' size is, too)
    if (pattern_set_program_bytes(sp, front, 1, char_width) == 0) return false;

    std::vector<Member> ms((size_t)count);
    for (int i = 0; i < count; ++i) {
        const RefTables &t = members[(size_t)first + i];
        Member &m = ms[(size_t)i];
        m.d = &t.dfa[which];
        m.stride = t.stride;
        m.cls.resize(N);
        m.over.resize(N);
        for (int k = 0; k < N; ++k) {
            m.cls[k] = t.class_map[rep[k]];
            m.over[k] = rep[k] > m.d->max_char;
        }
    }

    // ---- breadth-first product; a state = the components' states as int16 (-1: dead)
    typedef std::vector<int16_t> Key;
    auto key_str = [](const Key &k) { return std::string((const char *)k.data(), k.size() * 2); };
    auto mask_of = [&](const Key &k) {
        uint32_t bits = 0;
        for (int i = 0; i < count; ++i)
            if (k[i] >= 0 && ms[(size_t)i].d->accepting[k[i]]) bits |= 1u << (first + i);
        return bits;
    };
    std::unordered_map<std::string, int32_t> ids;
    std::vector<Key> states;
    const Key start((size_t)count, 0);
    ids.emplace(key_str(start), 0);
    states.push_back(start);
    sp.start = 0;
    sp.mask.push_back(mask_of(start));
    Key nxt((size_t)count);
    for (size_t s = 0; s < states.size(); ++s) {
        if ((s & 31) == 0) { // (aborted as soon as the product exceeds the budget)
            const size_t need = pattern_set_program_bytes(sp, front, (int)states.size(), char_width);
            if (need == 0 || need > budget) return false;
        }
        sp.table.resize((s + 1) * N);
        const Key cur = states[s]; // (a copy: `states` grows below)
        for (int k = 0; k < N; ++k) {
            bool all_dead = true;
            for (int i = 0; i < count; ++i) {
                const Member &m = ms[(size_t)i];
                int32_t c = cur[i];
                if (contained) {
                    if (m.d->accepting[c]) c = 0;
                    if (m.over[k]) c = 0;
                    else {
                        c = m.d->table[(size_t)c * m.stride + m.cls[k]];
                        if (c < 0) c = 0;
                    }
                } else if (c >= 0) {
                    c = m.over[k] ? -1 : m.d->table[(size_t)c * m.stride + m.cls[k]];
                    if (c < 0) c = -1;
                }
                nxt[i] = (int16_t)c;
                all_dead = all_dead && c < 0;
            }
            int32_t tgt = -1;
            if (contained || !all_dead) {
                auto it = ids.find(key_str(nxt));
                if (it == ids.end()) {
                    it = ids.emplace(key_str(nxt), (int32_t)states.size()).first;
                    states.push_back(nxt);
                    sp.mask.push_back(mask_of(nxt));
                }
                tgt = it->second;
            }
            sp.table[s * N + k] = tgt;
        }
    }
    sp.n_states = (int)states.size();
    g.prog = lower_pattern_set(sp, char_width, budget);
    if (g.prog.blob.empty()) return false;
    *out = std::move(g);
    return true;
}

bool build_set_plan(const std::vector<RefTables> &members, int op, int char_width, size_t budget, SetPlan *out, int *bad_index) {
    SetPlan plan;
    const int n = (int)members.size();
    for (int first = 0; first < n;) {
        SetGroup best;
        if (!build_set_group(members, first, 1, op, char_width, budget, &best)) {
            *bad_index = first;
            return false;
        }
        int count = 1;
        while (first + count < n) {
            SetGroup g;
            if (!build_set_group(members, first, count + 1, op, char_width, budget, &g)) break;
            best = std::move(g);
            ++count;
        }
        plan.groups.push_back(std::move(best));
        first += count;
    }
    *out = std::move(plan);
    return true;
}

} // namespace needle
