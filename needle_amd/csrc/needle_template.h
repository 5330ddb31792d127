// needle_template.h -- a replacement template with group references ("$2-$1") parsed into its canonical form, by the rules of
// java.util.regex.Matcher.appendReplacement (needle_template_parse, include/needle_hip.h).  Host code without HIP, as
// needle_host_plan.h is: tests/c/template_check.cpp includes it into a stand-alone program.
//
//   \x        the code unit x taken literally (also \$ and \\); a \ as the last unit is an error
//   $d...     a reference: the first digit must name a group (d <= G), further digits are taken while the number stays <= G
//             ($12 with G = 3 is group 1 followed by the literal 2); $0 is the whole match
//   ${name}   refused with a message of its own: the groups-kept parse of the regex drops the names
//   $ at the end or in front of anything else: an error;  every other unit is literal
// The canonical form is L_0 g_1 L_1 ... g_K L_K: K references (0 <= K <= kTemplateParseMaxRefs) and K + 1 literals, any of them empty,
// concatenated and located by lit_offsets[K + 2] (lit_offsets[0] = 0), at most kTemplateParseMaxUnits code units in all.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>

namespace needle {

constexpr uint32_t kTemplateParseMaxRefs = 16;    // NEEDLE_TEMPLATE_MAX_REFS
constexpr uint32_t kTemplateParseMaxUnits = 4096; // NEEDLE_REPLACE_MAX_UNITS

struct TemplateForm {
    std::vector<int32_t> groups;       // K
    std::vector<uint32_t> lit_offsets; // K + 2
    std::vector<uint16_t> lits;        // lit_offsets[K + 1]
};

// false: *err names the position (a code unit index of the template) and the rule.
inline bool template_parse(const uint16_t *t, size_t n, uint32_t n_groups, TemplateForm *out, std::string *err) {
    auto bad = [&](size_t at, const char *rule) {
        *err = "replacement template, code unit " + std::to_string(at) + ": " + rule;
        return false;
    };
    out->groups.clear();
    out->lits.clear();
    out->lit_offsets.assign(1, 0u);
    for (size_t i = 0; i < n;) {
        const uint16_t c = t[i];
        if (c == '\\') {
            if (i + 1 >= n) return bad(i, "a \\ at the end escapes nothing");
            out->lits.push_back(t[i + 1]);
            i += 2;
        } else if (c == '$') {
            if (i + 1 >= n) return bad(i, "a $ at the end names no group (write \\$ for a dollar sign)");
            if (t[i + 1] == '{') return bad(i, "named references ${name} are not supported: the compiled pattern keeps group numbers only");
            if (t[i + 1] < '0' || t[i + 1] > '9') return bad(i, "a $ must be followed by a group number (write \\$ for a dollar sign)");
            uint32_t g = (uint32_t)(t[i + 1] - '0');
            if (g > n_groups) return bad(i, "the pattern has no group of this number");
            size_t j = i + 2;
            while (j < n && t[j] >= '0' && t[j] <= '9') { // further digits, while the number still names a group
                const uint64_t next = (uint64_t)g * 10u + (uint64_t)(t[j] - '0');
                if (next > (uint64_t)n_groups) break;
                g = (uint32_t)next;
                ++j;
            }
            if (out->groups.size() >= kTemplateParseMaxRefs) return bad(i, "more than NEEDLE_TEMPLATE_MAX_REFS group references");
            out->groups.push_back((int32_t)g);
            out->lit_offsets.push_back((uint32_t)out->lits.size());
            i = j;
        } else {
            out->lits.push_back(c);
            ++i;
        }
        if (out->lits.size() > kTemplateParseMaxUnits) return bad(i - 1, "more than NEEDLE_REPLACE_MAX_UNITS literal code units");
    }
    out->lit_offsets.push_back((uint32_t)out->lits.size());
    return true;
}

} // namespace needle
