// xworld_amd/csrc/xwb_language.h -- the teacher's sentences of XWorld2D, host side (the C ABI's copy of xworld_amd/language.py's rule texts).
//
// In the reference every task owns a context-free grammar (python/context_free_grammar.py; games/xworld3d/tasks/
// XWorld3DNav*.py and games/xworld/tasks/XWorldNav*.py: `_define_grammar`); its idle stage binds the start symbol and the
// goal names and calls CFG.generate(), a left-most expansion that draws random.choice for every non-terminal.  Here the
// sentence of an env is a pure function of the batch state (task, bound goal names, direction word, stage, event,
// episode) and of xwb-rng-v1 stream 3 ("language": key = (seed, global env id), counter = (block, episode, 3, 0); one
// below(n) per expanded non-terminal, also when it is bound), so nothing is stored per env and the device never sees
// strings.  This file holds the rule texts, their compiler into xwb_sentence_ids.h's flat tables and the host's draw; the
// walk itself is xwb_sentence_ids.h's, for strings as for word ids: a string is the id sequence of an interning vocabulary
// looked up in its word list.  The rule texts, the stream and the order of the draws are those of language.py;
// tests/test_language.py and tests/test_sentence_ids_host.py compare the two sentence for sentence, and language.py is pinned
// to the reference's CFG by tests/golden/sentences.json.
#pragma once
#include "xwb_sentence_ids.h"

#include <cstdint>
#include <functional>
#include <map>
#include <sstream>
#include <string>
#include <vector>

namespace xwb {
namespace lang {

// Philox4x32-10 (Salmon et al. 2011), host copy of xwb_common.h's
inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// xwb-rng-v1 stream: words of successive blocks; below(n) = (u32 * n) >> 32 and always consumes one word
struct Stream {
    uint32_t k0, k1, episode, sid, blk = 0;
    uint32_t buf[4];
    int left = 0;
    Stream(uint32_t seed, uint32_t gid, uint32_t ep, uint32_t stream_id) : k0(seed), k1(gid), episode(ep), sid(stream_id) {}
    uint32_t below(uint32_t n) {
        if (left == 0) {
            buf[0] = blk; buf[1] = episode; buf[2] = sid; buf[3] = 0;
            philox4x32_10(buf, k0, k1);
            blk++;
            left = 4;
        }
        const uint32_t v = buf[4 - left];
        left--;
        return n > 1 ? (uint32_t)(((uint64_t)v * n) >> 32) : 0u;
    }
};

inline std::vector<std::string> split_ws(const std::string &s) {
    std::vector<std::string> out;
    std::istringstream is(s);
    std::string w;
    while (is >> w) out.push_back(w);
    return out;
}

// Rules `X -> a b | 'c' d` (terminals in single quotes), parsed for compile_sentence_tables
struct Grammar {
    std::map<std::string, std::vector<std::vector<std::string>>> rules;
    explicit Grammar(const std::string &text) {
        std::istringstream is(text);
        std::string line;
        while (std::getline(is, line)) {
            const size_t arrow = line.find("->");
            if (arrow == std::string::npos) continue;
            const std::vector<std::string> lhs = split_ws(line.substr(0, arrow));
            if (lhs.empty()) continue;
            std::vector<std::vector<std::string>> alts;
            std::string rhs = line.substr(arrow + 2);
            size_t pos = 0;
            while (true) {
                const size_t bar = rhs.find('|', pos);
                alts.push_back(split_ws(rhs.substr(pos, bar == std::string::npos ? std::string::npos : bar - pos)));
                if (bar == std::string::npos) break;
                pos = bar + 1;
            }
            rules[lhs[0]] = alts;
        }
    }
};

// task id (include/xwb.h XWB_TASK_*) -> grammar; nullptr: the task never speaks
inline const Grammar *grammar_of(int task) {
    static const std::string common =
        "S -> start | timeup | correct | wrong\n"
        "correct -> 'Well' 'done' '!'\n"
        "wrong -> 'Wrong' '!'\n"
        "timeup -> 'Time' 'up' '.'\n"
        "Y -> 'Could' 'you' 'please' | 'Can' 'you' | 'Will' 'you'\n"
        "D -> 'destination' | 'target' | 'goal' | 'end'\n";
    static const std::string go5 = "A -> 'go' 'to' | 'navigate' 'to' | 'reach' | 'move' 'to' | 'collect'\n";
    static const std::string go4 = "A -> 'go' 'to' | 'navigate' 'to' | 'reach' | 'move' 'to'\n";
    static const std::string common2d =
        "S -> start | finish | timeup\n"
        "finish -> 'Well' 'done' '!'\n"
        "timeup -> 'Time' 'up' '.'\n"
        "A -> 'go' 'to' | 'navigate' 'to' | 'reach' | 'move' 'to'\n"
        "Y -> 'Could' 'you' 'please' | 'Can' 'you' | 'Will' 'you'\n"
        "D -> 'destination' | 'target' | 'goal'\n";
    static const Grammar g0(common + go5 +
        "start -> I0 | I1 | I2 | I3 | I4 | I5 | I6\n"
        "I0 -> G\n"
        "I1 -> A G 'please' '.'\n"
        "I2 -> 'Please' A G '.'\n"
        "I3 -> A G '.'\n"
        "I4 -> G 'is' 'your' D '.'\n"
        "I5 -> G 'is' 'the' D '.'\n"
        "I6 -> Y A G '?'\n");
    static const Grammar g1(common + go5 +
        "start -> I0 | I1 | I2 | I3 | I4\n"
        "I0 -> A NP G\n"
        "I1 -> A NP G 'please' '.'\n"
        "I2 -> 'Please' A NP G '.'\n"
        "I3 -> NP G 'is' 'your' D '.'\n"
        "I4 -> Y A NP G '?'\n"
        "NP -> 'the' 'object' N\n"
        "N -> 'near' | 'by' | 'besides'\n");
    static const Grammar g2(common + go4 +
        "start -> I0 | I1 | I2 | I3 | I4\n"
        "I0 -> A L B '.'\n"
        "I1 -> A L B 'please' '.'\n"
        "I2 -> 'Please' A L B '.'\n"
        "I3 -> L B 'is' 'your' D '.'\n"
        "I4 -> Y A L B '?'\n"
        "B -> 'between' G1 'and' G2\n"
        "L -> 'the' 'location' | 'the' 'grid' | 'the' 'place'\n");
    static const Grammar g3(common + go5 +
        "start -> I0 | I1 | I2 | I3 | I4\n"
        "I0 -> A NP G '.'\n"
        "I1 -> A NP G 'please' '.'\n"
        "I2 -> 'Please' A NP G '.'\n"
        "I3 -> NP G 'is' 'your' D '.'\n"
        "I4 -> Y A NP G '?'\n"
        "NP -> 'the' 'object' P | 'the' 'object' 'that' 'is' P\n"
        "P -> LEFT | RIGHT | BEHIND | FRONT\n"
        "LEFT -> 'left' 'of' | 'to' 'the' 'left' 'of'\n"
        "RIGHT -> 'right' 'of' | 'to' 'the' 'right' 'of'\n"
        "BEHIND -> 'behind'\n"
        "FRONT -> 'in' 'the' 'front' 'of' | 'front' 'of'\n");
    static const Grammar g4(common + go5 +
        "start -> I0 | I1 | I2 | I4 | I5 | I6\n"
        "I0 -> V G '.'\n"
        "I1 -> V G 'please' '.'\n"
        "I2 -> 'Please' V G '.'\n"
        "I4 -> E G 'is' 'your' D '.'\n"
        "I5 -> E G 'is' 'the' D '.'\n"
        "I6 -> Y VV G '?'\n"
        "V -> 'do' 'not' A | 'avoid'\n"
        "VV -> 'not' A | 'avoid'\n"
        "E -> 'anything' 'except' | 'anything' 'but'\n");
    static const Grammar g5(common2d +
        "start -> I1 | I2 | I3 | I4 | I5 | I6\n"
        "I1 -> A G 'please' '.'\n"
        "I2 -> 'Please' A G '.'\n"
        "I3 -> A G '.'\n"
        "I4 -> G 'is' 'your' D '.'\n"
        "I5 -> G 'is' 'the' D '.'\n"
        "I6 -> Y A G '?'\n");
    static const Grammar g7(common2d +
        "start -> I1 | I2 | I3 | I4 | I5 | I6 | I7\n"
        "I1 -> A G 'please' '.'\n"
        "I2 -> 'Please' A G '.'\n"
        "I3 -> A G '.'\n"
        "I4 -> G 'is' 'your' D '.'\n"
        "I5 -> G 'is' 'the' D '.'\n"
        "I6 -> Y A G '?'\n"
        "I7 -> G '.'\n"
        "G -> C O\n");
    switch (task) {
        case 0: return &g0;
        case 1: return &g1;
        case 2: return &g2;
        case 3: return &g3;
        case 4: return &g4;
        case 5: return &g5;
        case 7: return &g7;
        default: return nullptr;
    }
}

// ---- the rule texts above compiled into xwb_sentence_ids.h's flat tables, under a vocabulary ----

inline std::string fold_ascii(std::string w) {
    for (char &ch : w) if (ch >= 'A' && ch <= 'Z') ch = (char)(ch - 'A' + 'a');
    return w;
}

// words[i] -> i.  Empty entries (blank lines of a dict file) keep their ids and never match a word.  intern: the vocabulary
// behind the strings instead -- an unknown word is appended as it stands (no folding, no unk) and words[id] gives it back.
struct Vocab {
    std::map<std::string, int32_t> ids;
    std::vector<std::string> words;             // intern only
    int32_t unk = 0;
    bool fold = false, intern = false;
    explicit Vocab(bool interning = false) : intern(interning) {}
    int32_t id(const std::string &w) {
        if (intern) {
            const auto r = ids.emplace(w, (int32_t)words.size());
            if (r.second) words.push_back(w);
            return r.first->second;
        }
        const std::map<std::string, int32_t>::const_iterator it = ids.find(fold ? fold_ascii(w) : w);
        return it == ids.end() ? unk : it->second;
    }
};

// "" on success, else what is wrong
inline std::string make_vocab(const char *const *words, int32_t n_words, int32_t unk, int32_t fold, Vocab &v) {
    if (!words) return "words is NULL";
    if (n_words <= 0 || n_words > sent::MAX_WORD_ID) return "n_words out of range";
    if (unk < 0 || unk >= n_words) return "unk_id is not an id of the vocabulary";
    v.ids.clear();
    v.unk = unk;
    v.fold = fold != 0;
    for (int32_t i = 0; i < n_words; ++i) {
        if (!words[i]) return "NULL word in the vocabulary";
        if (!words[i][0]) continue;
        const std::string w = v.fold ? fold_ascii(words[i]) : std::string(words[i]);
        if (!v.ids.emplace(w, i).second) return "duplicate word in the vocabulary: '" + w + "'";
    }
    return "";
}

inline bool has_space(const std::string &s) {
    for (char ch : s) if (ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r' || ch == '\v' || ch == '\f') return true;
    return false;
}
// the word id of a bound name / colour: the whole string is one word
inline bool one_word(const std::string &s) { return !s.empty() && !has_space(s); }
inline std::string not_one_word(const std::string &s) {
    return "a name or colour is not one word: '" + s + "' (a bound name is one vocabulary entry)";
}

struct SentLayout {
    std::vector<int32_t> tab;
    sent::SentTab lay{};
    int32_t max_words[sent::N_TASKS] = {};      // longest sentence per task (a bound name or colour is one word); 0: silent task
};

// the rules a task binds (language.py instruction_bindings / sentence_2d): those are slots, the others non-terminals
inline int slot_of(int task, const std::string &sym) {
    if (sym == "S") return sent::SL_S;
    if (sym == "P" && task == 3) return sent::SL_P;
    if (sym == "G" && task != 2 && task != 7) return sent::SL_G;
    if (task == 2 && sym == "G1") return sent::SL_G1;
    if (task == 2 && sym == "G2") return sent::SL_G2;
    if (task == 7 && sym == "O") return sent::SL_O;
    if (task == 7 && sym == "C") return sent::SL_C;
    return -1;
}

// Builds the tables of every task with a grammar.  "" on success, else what is wrong.  (An interning vocabulary takes the
// names as they stand: sentence_text refuses the one a sentence binds.)
inline std::string compile_sentence_tables(Vocab &v, const std::vector<std::string> &goal_names, const std::vector<std::string> &icon_names,
                                           const std::vector<std::string> &icon_colors, SentLayout &out) {
    using namespace sent;
    for (const std::vector<std::string> *names : {&goal_names, &icon_names, &icon_colors})
        for (const std::string &s : *names)
            if (!v.intern && !one_word(s)) return not_one_word(s);
    std::vector<int32_t> special(N_TASKS * N_SPECIAL, -1), nts, alts, syms;   // nts / alts: pairs (first, count)
    std::vector<int32_t> nt_task;                                             // owning task of each non-terminal
    static const char *const SPECIAL_NAMES[N_SPECIAL] = {"start", "correct", "wrong", "timeup", "finish", "FRONT", "BEHIND", "LEFT", "RIGHT"};
    for (int task = 0; task < N_TASKS; ++task) {
        const Grammar *g = grammar_of(task);
        if (!g) continue;
        std::map<std::string, int32_t> nt_id;
        for (const auto &r : g->rules)
            if (slot_of(task, r.first) < 0) { nt_id[r.first] = (int32_t)nt_task.size(); nt_task.push_back(task); }
        nts.resize(2 * nt_task.size());
        for (const auto &r : g->rules) {
            const std::map<std::string, int32_t>::const_iterator self = nt_id.find(r.first);
            if (self == nt_id.end()) continue;
            nts[2 * self->second] = (int32_t)(alts.size() / 2);
            nts[2 * self->second + 1] = (int32_t)r.second.size();
            for (const std::vector<std::string> &alt : r.second) {
                alts.push_back((int32_t)syms.size());
                alts.push_back((int32_t)alt.size());
                for (const std::string &s : alt) {
                    if (s.size() >= 2 && s[0] == '\'') { syms.push_back(v.id(s.substr(1, s.size() - 2))); continue; }
                    const int sl = slot_of(task, s);
                    if (sl >= 0) { syms.push_back(SYM_SLOT | sl); continue; }
                    const std::map<std::string, int32_t>::const_iterator it = nt_id.find(s);
                    if (it == nt_id.end()) return "grammar of task " + std::to_string(task) + ": no rule for " + s;
                    syms.push_back(SYM_NT | it->second);
                }
            }
        }
        for (int k = 0; k < N_SPECIAL; ++k) {
            const std::map<std::string, int32_t>::const_iterator it = nt_id.find(SPECIAL_NAMES[k]);
            if (it != nt_id.end()) special[task * N_SPECIAL + k] = it->second;
        }
    }
    // longest sentence and deepest stack per symbol (the grammars are acyclic: a cycle is an error)
    const int n_nt = (int)nt_task.size();
    std::vector<int> words(n_nt, -1), depth(n_nt, -1), state(n_nt, 0);
    std::string err;
    std::function<void(int)> visit;
    // words / stack entries a symbol of `task` expands to, at most; S and P: the largest rule they can be bound to (+1: the
    // bound rule itself sits on the stack first)
    std::function<void(int, int32_t, int &, int &)> cost = [&](int task, int32_t s, int &w, int &d) {
        w = 1; d = 1;
        if (s & SYM_NT) { visit(s & SYM_VALUE); w = words[s & SYM_VALUE]; d = depth[s & SYM_VALUE]; return; }
        const int sl = s & SYM_VALUE;
        if (!(s & SYM_SLOT) || (sl != SL_S && sl != SL_P)) return;
        w = 0;
        const int k0 = sl == SL_S ? SP_START : SP_FRONT, k1 = sl == SL_S ? SP_FINISH : SP_RIGHT;
        for (int k = k0; k <= k1; ++k) {
            const int32_t nt = special[task * N_SPECIAL + k];
            if (nt < 0) continue;
            visit(nt);
            if (words[nt] > w) w = words[nt];
            if (depth[nt] > d) d = depth[nt];
        }
    };
    visit = [&](int nt) {
        if (state[nt] == 2 || !err.empty()) return;
        if (state[nt] == 1) { err = "cyclic grammar"; return; }
        state[nt] = 1;
        int wmax = 0, dmax = 1;
        for (int32_t a = nts[2 * nt]; a < nts[2 * nt] + nts[2 * nt + 1]; ++a) {
            const int32_t s0 = alts[2 * a], len = alts[2 * a + 1];
            int wsum = 0;
            for (int32_t i = 0; i < len; ++i) {
                int w = 0, d = 1;
                cost(nt_task[nt], syms[s0 + i], w, d);
                wsum += w;
                if ((len - 1 - i) + d > dmax) dmax = (len - 1 - i) + d;
            }
            if (wsum > wmax) wmax = wsum;
        }
        words[nt] = wmax; depth[nt] = dmax; state[nt] = 2;
    };
    for (int task = 0; task < N_TASKS; ++task) {
        if (special[task * N_SPECIAL + SP_START] < 0) continue;
        int w = 0, d = 1;
        cost(task, SYM_SLOT | SL_S, w, d);              // the sentence starts from S (bound)
        if (!err.empty()) return err;
        if (d + 1 > STACK_MAX) return "grammar of task " + std::to_string(task) + " needs a deeper stack than STACK_MAX";
        out.max_words[task] = w;
    }
    SentTab &L = out.lay;
    L.n_nt = n_nt; L.n_alt = (int32_t)(alts.size() / 2); L.n_sym = (int32_t)syms.size();
    L.n_goal = (int32_t)goal_names.size(); L.n_icon = (int32_t)icon_names.size();
    L.off_nt = N_TASKS * N_SPECIAL;
    L.off_alt = L.off_nt + (int32_t)nts.size();
    L.off_sym = L.off_alt + (int32_t)alts.size();
    L.off_goal = L.off_sym + L.n_sym;
    L.off_iname = L.off_goal + L.n_goal;
    L.off_icolor = L.off_iname + L.n_icon;
    L.total = L.off_icolor + L.n_icon;
    std::vector<int32_t> &t = out.tab;
    t.assign(special.begin(), special.end());
    t.insert(t.end(), nts.begin(), nts.end());
    t.insert(t.end(), alts.begin(), alts.end());
    t.insert(t.end(), syms.begin(), syms.end());
    for (const std::string &s : goal_names) t.push_back(v.id(s));
    for (const std::string &s : icon_names) t.push_back(v.id(s));
    for (int i = 0; i < L.n_icon; ++i) t.push_back(v.id(i < (int)icon_colors.size() ? icon_colors[i] : std::string("na")));
    L.t = nullptr;
    return "";
}

// the longest sentence a task can produce (bound names one word each): the tables' structure does not depend on the words
inline int32_t max_sentence_words(int task) {
    static const SentLayout layout = [] {
        SentLayout l;
        Vocab v;
        (void)compile_sentence_tables(v, {}, {}, {}, l);
        return l;
    }();
    return task >= 0 && task < sent::N_TASKS ? layout.max_words[task] : 0;
}

// ---- one sentence on the host: the slots sent::pick_* selected, walked through the tables ----

// The ids of the sentence; blk0: the first block of stream 3 it draws from (a 2-D-native task: 4 * num_steps).  false: the
// tables or the stack are out of range.
inline bool host_walk(const sent::SentTab &T, const sent::Slots &b, bool first, uint32_t seed, uint32_t gid, uint32_t episode,
                      uint32_t blk0, std::vector<int32_t> &ids) {
    Stream st(seed, gid, episode, 3);
    st.blk = blk0;
    auto draw = [&](uint32_t n) { return first ? 0u : st.below(n); };
    auto emit = [&](int32_t, int32_t w) { ids.push_back(w); };
    int32_t stack[sent::STACK_MAX];
    return sent::expand(T, b, draw, stack, 1, emit) >= 0;
}

// ids of an interning vocabulary -> "w0 w1 ...".  "" on success.  No word of the rule texts holds white space, so one that
// does is a bound name that is not one word.
inline std::string join_words(const std::vector<std::string> &words, const std::vector<int32_t> &ids, std::string &out) {
    out.clear();
    for (size_t i = 0; i < ids.size(); ++i) {
        const std::string &w = words[ids[i]];
        if (has_space(w)) return not_one_word(w);
        if (i) out += ' ';
        out += w;
    }
    return "";
}

// One sentence without a batch (the xwb_language_* hooks): the tables of these names under v, the slots, the walk.  two_d: a
// 2-D-native task's arguments -- the target's icon is (goal_names[name_a], color), event 3 selects its time-up message, which
// binds no name.  "" on success, else what is wrong; ids stays empty when the teacher is silent.
inline std::string hook_sentence(Vocab &v, bool two_d, int task, int stage, int event, const char *const *goal_names, int32_t n_goals,
                                 uint32_t name_a, uint32_t name_b, int direction, const char *color, uint32_t seed, uint32_t gid,
                                 uint32_t episode, uint32_t num_steps, std::vector<int32_t> &ids) {
    if (n_goals < 0 || (n_goals > 0 && !goal_names)) return "NULL argument";
    std::vector<std::string> goals, inames, icolors;
    for (int32_t i = 0; i < n_goals; ++i) {
        if (!goal_names[i]) return "NULL name";
        goals.push_back(goal_names[i]);
    }
    if (two_d && event != 3) {
        if (name_a >= goals.size()) return "name_a out of range";
        if (task == 7 && !color) return "NULL colour";
        inames.push_back(goals[name_a]);
        icolors.push_back(color ? color : "na");
    }
    SentLayout L;
    const std::string err = compile_sentence_tables(v, goals, inames, icolors, L);
    if (!err.empty()) return err;
    L.lay.t = L.tab.data();
    sent::Slots b;
    bool first = false;
    const bool speaks = two_d ? sent::pick_2d(L.lay, task, event == 3, 0, b, first)
                              : sent::pick_3d(L.lay, task, stage, event, name_a, name_b, direction, b, first);
    if (speaks && !host_walk(L.lay, b, first, seed, gid, episode, two_d ? 4 * num_steps : 0, ids)) return "sentence expansion out of range";
    return "";
}

}  // namespace lang
}  // namespace xwb
