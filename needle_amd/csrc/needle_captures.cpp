// The capture program on the host (needle_captures.h): determinisation of the priority Thompson program into a tagged DFA, and its
// lowering to a plain LDS program.
#include "needle_captures.h"

#include <algorithm>
#include <cstring>
#include <map>

#include "../../include/needle_hip.h"
#include "needle_regex.h"

namespace needle {
namespace {

struct TooBig {
    std::string why;
};

struct Thread {
    int pc, src;
    uint32_t tags;
};

class Determiniser {
  public:
    Determiniser(const CapNfa &nfa_, CapTables &out_) : nfa(nfa_), prog(nfa_.prog), t(out_), stamp(nfa_.prog.size(), 0) {}

    void run() {
        G2 = 2 * nfa.n_groups;
        classes();
        t.op_off.assign(1, 0); // op list 0: empty
        t.op_off.push_back(0);
        op_ids[std::vector<int32_t>()] = 0;
        add_row(); // state 0: the sink
        t.fin.push_back(-1);
        std::vector<Thread> init;
        ++cur;
        close(0, 0u, 0, init);
        for (size_t k = 0; k < init.size(); ++k) init[k].src = -1; // (no old thread: every slot is set, to 0 or to -1)
        t.start = state_of(init);
        t.init_op = op_list(init);
        for (size_t s = 1; s < states.size(); ++s) { // (states are appended while this runs)
            for (int c = 0; c < t.n_cols; ++c) {
                std::vector<Thread> nt;
                ++cur;
                const std::vector<int> st = states[s]; // (a copy: state_of may grow `states`)
                for (size_t k = 0; k < st.size(); ++k) {
                    const CapInstr &in = prog[(size_t)st[k]];
                    if (in.op == CAP_CSET && set_has[(size_t)set_of[(size_t)st[k]]][(size_t)c]) close(st[k] + 1, 0u, (int)k, nt);
                }
                if (nt.empty()) continue; // (the sink, op list 0)
                const int to = state_of(nt);
                const int op = op_list(nt);
                t.next[s * (size_t)t.n_cols + (size_t)c] = to;
                t.op_id[s * (size_t)t.n_cols + (size_t)c] = op;
            }
        }
        t.n_states = (int)states.size();
        t.n_slots = t.max_threads * G2;
        t.n_op_lists = (int)t.op_off.size() - 1;
    }

  private:
    const CapNfa &nfa;
    const std::vector<CapInstr> &prog;
    CapTables &t;
    int G2 = 0;
    std::vector<int> stamp;
    int cur = 0;
    std::vector<int> set_of;                 // instruction -> distinct char set
    std::vector<std::vector<char>> set_has;  // [set][column]
    std::vector<std::vector<int>> states = {std::vector<int>()};
    std::map<std::vector<int>, int> state_ids;
    std::map<std::vector<int32_t>, int> op_ids;

    // Columns: the chars that the same char sets hold share one (the chars of no set too: every state sends them to the sink).
    void classes() {
        std::map<std::vector<std::pair<int, int>>, int> ids;
        std::vector<const std::vector<std::pair<int, int>> *> sets;
        set_of.assign(prog.size(), -1);
        std::vector<int> cuts = {0, 65536};
        for (size_t i = 0; i < prog.size(); ++i) {
            if (prog[i].op != CAP_CSET) continue;
            auto it = ids.find(prog[i].ranges);
            if (it == ids.end()) {
                it = ids.emplace(prog[i].ranges, (int)sets.size()).first;
                sets.push_back(&prog[i].ranges);
                for (const auto &r : prog[i].ranges) { cuts.push_back(r.first); cuts.push_back(r.second + 1); }
            }
            set_of[i] = it->second;
        }
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        std::map<std::vector<char>, int> cols;
        t.class_map.assign(65536, 0);
        std::vector<std::vector<char>> sig_of_col;
        for (size_t i = 0; i + 1 < cuts.size(); ++i) {
            const int lo = cuts[i], hi = cuts[i + 1] - 1;
            std::vector<char> sig(sets.size(), 0);
            for (size_t s = 0; s < sets.size(); ++s)
                for (const auto &r : *sets[s])
                    if (r.first <= lo && hi <= r.second) { sig[s] = 1; break; }
            auto it = cols.find(sig);
            if (it == cols.end()) {
                if (cols.size() >= kCapMaxCols) throw TooBig{"more than 255 columns"};
                it = cols.emplace(sig, (int)cols.size()).first;
                sig_of_col.push_back(sig);
            }
            for (int c = lo; c <= hi; ++c) t.class_map[(size_t)c] = (uint8_t)it->second;
        }
        t.n_cols = (int)cols.size();
        set_has.assign(sets.size(), std::vector<char>((size_t)t.n_cols, 0));
        for (size_t c = 0; c < sig_of_col.size(); ++c)
            for (size_t s = 0; s < sets.size(); ++s) set_has[s][c] = sig_of_col[c][s];
    }

    // The closure of `pc`, depth first in priority order; the first visit of an instruction wins within one step (`cur`).
    void close(int pc, uint32_t tags, int src, std::vector<Thread> &out) {
        for (;;) {
            if (stamp[(size_t)pc] == cur) return;
            stamp[(size_t)pc] = cur;
            const CapInstr &in = prog[(size_t)pc];
            if (in.op == CAP_JMP) pc = in.x;
            else if (in.op == CAP_SAVE) { tags |= 1u << in.x; ++pc; }
            else if (in.op == CAP_SPLIT) { close(in.x, tags, src, out); pc = in.y; }
            else break;
        }
        out.push_back(Thread{pc, src, tags});
        if (out.size() * (size_t)G2 > kCapMaxSlots) throw TooBig{"a state needs more than " + std::to_string(kCapMaxSlots) + " slots"};
    }

    void add_row() {
        t.next.resize(t.next.size() + (size_t)t.n_cols, 0);
        t.op_id.resize(t.op_id.size() + (size_t)t.n_cols, 0);
        if (t.next.size() * 4u > kCapLdsBytes) throw TooBig{"the table does not fit the LDS"};
    }

    int state_of(const std::vector<Thread> &th) {
        std::vector<int> key(th.size());
        for (size_t k = 0; k < th.size(); ++k) key[k] = th[k].pc;
        auto it = state_ids.find(key);
        if (it != state_ids.end()) return it->second;
        if (states.size() >= kCapMaxStates) throw TooBig{"more than " + std::to_string(kCapMaxStates) + " states"};
        const int id = (int)states.size();
        state_ids.emplace(key, id);
        states.push_back(key);
        add_row();
        int f = -1;
        for (size_t k = 0; k < key.size() && f < 0; ++k)
            if (prog[(size_t)key[k]].op == CAP_MATCH) f = (int)k;
        t.fin.push_back(f);
        t.max_threads = std::max(t.max_threads, (int)key.size());
        return id;
    }

    // The op list of a transition into threads `th` (src < 0: the initial state, whose unset tags are cleared).  Sources do not
    // decrease with the thread index, so a thread that moves up never reads what a thread that moves down writes, nor the other way
    // round; within each kind the order below keeps a source from being overwritten before it is read.
    int op_list(const std::vector<Thread> &th) {
        std::vector<int32_t> ops;
        auto copy_thread = [&](int k) {
            for (int tag = 0; tag < G2; ++tag)
                if (!(th[(size_t)k].tags >> tag & 1u)) {
                    ops.push_back(k * G2 + tag);
                    ops.push_back(th[(size_t)k].src < 0 ? kCapSrcNone : th[(size_t)k].src * G2 + tag);
                }
        };
        for (int k = (int)th.size() - 1; k >= 0; --k)
            if (th[(size_t)k].src >= 0 && th[(size_t)k].src < k) copy_thread(k);
        for (int k = 0; k < (int)th.size(); ++k)
            if (th[(size_t)k].src < 0 || th[(size_t)k].src > k) copy_thread(k);
        for (int k = 0; k < (int)th.size(); ++k)
            for (int tag = 0; tag < G2; ++tag)
                if (th[(size_t)k].tags >> tag & 1u) {
                    ops.push_back(k * G2 + tag);
                    ops.push_back(kCapSrcPos);
                }
        auto it = op_ids.find(ops);
        if (it != op_ids.end()) return it->second;
        const int id = (int)t.op_off.size() - 1;
        if (id >= 65535) throw TooBig{"too many op lists"};
        t.ops.insert(t.ops.end(), ops.begin(), ops.end());
        if (t.ops.size() / 2 > kCapMaxOps) throw TooBig{"the op lists do not fit the LDS"};
        t.op_off.push_back((int32_t)(t.ops.size() / 2));
        op_ids.emplace(std::move(ops), id);
        return id;
    }
};

void put_u32(std::vector<uint8_t> &b, size_t at, uint32_t v) { memcpy(b.data() + at, &v, 4); }
size_t align16(size_t n) { return (n + 15u) & ~(size_t)15; }

} // namespace

int build_captures(const std::u16string &regex, int flags, CapTables &out, std::string &err) {
    out = CapTables();
    CapNfa nfa;
    const int rc = build_captures_nfa(regex, flags, (size_t)1 << 20, nfa, err);
    if (rc != NEEDLE_OK) return rc;
    out.n_groups = nfa.n_groups;
    auto refuse = [&](int reason, const std::string &why) {
        const int g = out.n_groups;
        out = CapTables();
        out.n_groups = g;
        out.reason = reason;
        out.why = why;
        return NEEDLE_OK;
    };
    if (nfa.n_groups > kCapMaxGroups) return refuse(CAP_TOO_MANY_GROUPS, "more than 16 capturing groups");
    if (nfa.nullable_loop) return refuse(CAP_NULLABLE_LOOP, "a loop's body can match the empty string");
    if (nfa.too_big) return refuse(CAP_TOO_BIG, "the capture program has too many instructions");
    try {
        Determiniser(nfa, out).run();
    } catch (const TooBig &e) {
        return refuse(CAP_TOO_BIG, e.why);
    }
    out.reason = CAP_OK;
    return NEEDLE_OK;
}

CapProgram lower_captures(const CapTables &t, int char_width) {
    CapProgram p;
    if (t.reason != CAP_OK || (char_width != 1 && char_width != 2)) return p;
    CapHeader &h = p.hdr;
    h.n_states = (uint32_t)t.n_states;
    h.n_cols = (uint32_t)t.n_cols;
    h.n_groups = (uint32_t)t.n_groups;
    h.n_slots = (uint32_t)t.n_slots;
    h.start = (uint32_t)t.start;
    h.init_op = (uint32_t)t.init_op;
    // column maps: 8-bit rows one map of 256; UTF-16 rows a page per distinct run of 256 chars behind a map of the high byte
    std::vector<uint8_t> maps;
    if (char_width == 1) {
        maps.assign(t.class_map.begin(), t.class_map.begin() + 256);
        h.off_cmap = 0;
        h.off_pages = 0;
    } else {
        std::map<std::vector<uint8_t>, int> pages;
        std::vector<uint8_t> ptab(256), body;
        for (int hi = 0; hi < 256; ++hi) {
            std::vector<uint8_t> pg(t.class_map.begin() + hi * 256, t.class_map.begin() + hi * 256 + 256);
            auto it = pages.find(pg);
            if (it == pages.end()) {
                it = pages.emplace(pg, (int)pages.size()).first;
                body.insert(body.end(), pg.begin(), pg.end());
            }
            ptab[(size_t)hi] = (uint8_t)it->second; // (at most 256 pages)
        }
        maps = ptab;
        maps.insert(maps.end(), body.begin(), body.end());
        h.off_cmap = 0;
        h.off_pages = 256;
    }
    const size_t n_cells = (size_t)t.n_states * (size_t)t.n_cols, n_lists = (size_t)t.n_op_lists, n_ops = t.ops.size() / 2;
    h.off_table = (uint32_t)align16(maps.size());
    h.off_opidx = (uint32_t)align16(h.off_table + n_cells * 4);
    h.off_ops = (uint32_t)align16(h.off_opidx + n_lists * 4);
    h.off_fin = (uint32_t)align16(h.off_ops + n_ops * 4);
    h.lds_bytes = (uint32_t)align16(h.off_fin + (size_t)t.n_states * 4);
    if ((size_t)h.lds_bytes + (size_t)kCapMinWaves * cap_wave_lds(h.n_slots) > kCapLdsBytes) return p;
    p.blob.assign(h.lds_bytes, 0);
    memcpy(p.blob.data(), maps.data(), maps.size());
    for (size_t i = 0; i < n_cells; ++i) put_u32(p.blob, h.off_table + i * 4, (uint32_t)t.next[i] | (uint32_t)t.op_id[i] << 16);
    for (size_t k = 0; k < n_lists; ++k) {
        const uint32_t first = (uint32_t)t.op_off[k], cnt = (uint32_t)(t.op_off[k + 1] - t.op_off[k]);
        if (cnt > 4095u || first >= (1u << 20)) return p;
        put_u32(p.blob, h.off_opidx + k * 4, first | cnt << 20);
    }
    for (size_t i = 0; i < n_ops; ++i) {
        const int32_t src = t.ops[2 * i + 1];
        const uint32_t s = src == kCapSrcPos ? kCapDevPos : src == kCapSrcNone ? kCapDevNone : (uint32_t)src;
        put_u32(p.blob, h.off_ops + i * 4, (uint32_t)t.ops[2 * i] | s << 16);
    }
    for (size_t s = 0; s < (size_t)t.n_states; ++s) put_u32(p.blob, h.off_fin + s * 4, (uint32_t)t.fin[s]);
    p.ok = true;
    return p;
}

} // namespace needle
