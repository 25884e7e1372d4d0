// xwb_sentence_ids.h -- the teacher's sentence as word ids: the flat grammar tables, the rule for which task group spoke, the
// slots it binds and the expansion that walks the tables.  The one path to a sentence, on the device (xwb_sentence_ids.hip: one
// lane per env) and on the host (xwb_language.h host_walk: xwb_sentence, the state packets, the xwb_language_* hooks; a string
// is the id sequence looked up in a word list).
//
// xwb_language.h's rule texts are compiled (compile_sentence_tables there) into one int32 table per batch:
//   [task * N_SPECIAL + k]         per task 0..8: the non-terminal of start, correct, wrong, timeup, finish, FRONT, BEHIND, LEFT,
//                                  RIGHT (-1: none; a task without a grammar has no start)
//   [off_nt  + 2 * nt]             first alternative, number of alternatives
//   [off_alt + 2 * alt]            first symbol, number of symbols
//   [off_sym + i]                  a symbol: a word id (terminal), SYM_NT | non-terminal, SYM_SLOT | slot (a bound rule)
//   [off_goal + name id]           word id of each goal name (xwb_set_names' goal_names)
//   [off_iname / off_icolor + icon] word id of each icon's name / colour (the 2-D-native tasks bind those)
// A bound rule (S, P, G, G1, G2, O, C) has one alternative and still consumes one below(n) draw, as in language.py's
// Grammar.expand.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define XWB_SENT_HD __host__ __device__ __forceinline__
#else
#define XWB_SENT_HD inline
#endif

namespace xwb {
namespace sent {

constexpr int32_t SYM_NT = 0x40000000, SYM_SLOT = 0x20000000, SYM_VALUE = 0x0fffffff;
constexpr int32_t MAX_WORD_ID = SYM_VALUE;           // vocabularies hold fewer words than this
enum : int { SL_S = 0, SL_P, SL_G, SL_G1, SL_G2, SL_O, SL_C, N_SLOTS };
enum : int { SP_START = 0, SP_CORRECT, SP_WRONG, SP_TIMEUP, SP_FINISH, SP_FRONT, SP_BEHIND, SP_LEFT, SP_RIGHT, N_SPECIAL };
constexpr int N_TASKS = 9;
constexpr int STACK_MAX = 16;                         // the compiler rejects grammars that need a deeper stack
constexpr int MAX_EXPANSIONS = 256;                   // symbols popped per sentence, at most

struct SentTab {
    const int32_t *t;
    int32_t n_nt, n_alt, n_sym, n_goal, n_icon;
    int32_t off_nt, off_alt, off_sym, off_goal, off_iname, off_icolor, total;
};

// what the bound rules of one sentence hold: S -> start_nt, P -> p_nt, G / G1 / G2 / O / C -> one word id each
struct Slots {
    int32_t start_nt = -1, p_nt = -1, g = 0, g1 = 0, g2 = 0, o = 0, c = 0;
};

// language.py's Grammar.expand as a loop: the stack holds the symbols still to expand, the left-most on top, so the draws come in the recursion's
// order.  emit(k, word) receives word k of the sentence.  Returns the word count, -1 when the tables or the stack are out of range.
// stk: STACK_MAX entries, `stride` apart.
template <typename Draw, typename Emit>
XWB_SENT_HD int32_t expand(const SentTab &T, const Slots &b, Draw &draw, int32_t *stk, int stride, Emit &emit) {
    int sp = 0;
    int32_t n = 0;
    stk[0] = SYM_SLOT | SL_S;
    sp = 1;
    for (int guard = 0; sp > 0; ++guard) {
        if (guard >= MAX_EXPANSIONS) return -1;
        const int32_t sym = stk[(--sp) * stride];
        if (!(sym & (SYM_NT | SYM_SLOT))) { emit(n, sym); ++n; continue; }
        int32_t nt;
        if (sym & SYM_SLOT) {
            const int32_t sl = sym & SYM_VALUE;
            (void)draw(1u);                                   // a bound rule: one alternative, one draw
            if (sl == SL_S || sl == SL_P) {
                nt = sl == SL_S ? b.start_nt : b.p_nt;
                if (nt < 0 || nt >= T.n_nt || sp >= STACK_MAX) return -1;
                stk[(sp++) * stride] = SYM_NT | nt;
                continue;
            }
            const int32_t w = sl == SL_G ? b.g : sl == SL_G1 ? b.g1 : sl == SL_G2 ? b.g2 : sl == SL_O ? b.o : sl == SL_C ? b.c : -1;
            if (w < 0) return -1;
            emit(n, w);
            ++n;
            continue;
        }
        nt = sym & SYM_VALUE;
        if (nt >= T.n_nt) return -1;
        const int32_t a0 = T.t[T.off_nt + 2 * nt], na = T.t[T.off_nt + 2 * nt + 1];
        const int32_t a = a0 + (int32_t)draw((uint32_t)na);
        if (na < 1 || a < 0 || a >= T.n_alt) return -1;
        const int32_t s0 = T.t[T.off_alt + 2 * a], len = T.t[T.off_alt + 2 * a + 1];
        if (len < 0 || s0 < 0 || s0 + len > T.n_sym || sp + len > STACK_MAX) return -1;
        for (int32_t k = len - 1; k >= 0; --k) stk[(sp++) * stride] = T.t[T.off_sym + s0 + k];
    }
    return n;
}

// language.sentence(): which rule S is bound to, and the names.  *first: the event messages take the
// first alternative everywhere and draw nothing.  Returns false when the teacher is silent.
XWB_SENT_HD bool pick_3d(const SentTab &T, int task, int stage, int event, uint32_t name_a, uint32_t name_b, int direction, Slots &b,
                         bool &first) {
    if (task < 0 || task >= N_TASKS) return false;
    const int32_t *sp = T.t + task * N_SPECIAL;
    if (sp[SP_START] < 0) return false;
    if (event >= 1 && event <= 3) {
        first = true;
        b.start_nt = sp[event == 1 ? SP_CORRECT : event == 2 ? SP_WRONG : SP_TIMEUP];
        return b.start_nt >= 0;
    }
    if (stage != 1 || name_a == 0xFFFFu || name_a >= (uint32_t)T.n_goal) return false;
    first = false;
    if (task == 2) {
        if (name_b >= (uint32_t)T.n_goal) return false;
        b.g1 = T.t[T.off_goal + name_a];
        b.g2 = T.t[T.off_goal + name_b];
    } else {
        b.g = T.t[T.off_goal + name_a];
    }
    if (task == 3) {
        if (direction < 1 || direction > 4) return false;
        b.p_nt = sp[SP_FRONT + direction - 1];        // xw_device.h DIR_*: 1 front, 2 behind, 3 left, 4 right
        if (b.p_nt < 0) return false;
    }
    b.start_nt = sp[SP_START];
    return true;
}

// language.sentence_2d / sentence_2d_timeup: a 2-D-native task's instruction (the target's icon bound) or its time-up message
XWB_SENT_HD bool pick_2d(const SentTab &T, int task, bool timeup, int icon, Slots &b, bool &first) {
    if (task != 5 && task != 7) return false;
    const int32_t *sp = T.t + task * N_SPECIAL;
    if (timeup) {
        first = true;
        b.start_nt = sp[SP_TIMEUP];
        return b.start_nt >= 0;
    }
    if (icon < 0 || icon >= T.n_icon) return false;
    first = false;
    if (task == 7) {
        b.o = T.t[T.off_iname + icon];
        b.c = T.t[T.off_icolor + icon];
    } else {
        b.g = T.t[T.off_iname + icon];
    }
    b.start_nt = sp[SP_START];
    return b.start_nt >= 0;
}

// One env's packed state, as the step kernels leave it: task_state = target (int16) | stage << 16 | event << 20 | task << 24
// (xwb_get_env_state unpacks the same bits), sent_names = name id a | b << 16
struct EnvWords {
    int32_t task_state, task_steps;
    bool two;                                 // a second task group: its two words
    int32_t task_state2, task_steps2;
    int32_t num_steps;
    uint32_t sent_names;
    int grp_order;                            // exclusive scheduling of two groups: the grp_order byte (bit 1: the group that ran), else -1
    bool one_channel;
    int cells;
};

// What one task group says, from its packed task state (batched.py: BatchedSimulator's rule for one group).  cell_at(cell): the grid code there, read only for the
// 2-D-native tasks' instruction.
template <typename CellAt>
XWB_SENT_HD bool pick_group(const SentTab &T, const EnvWords &w, int32_t ts, int32_t tsteps, CellAt &cell_at, Slots &b, bool &first,
                            bool &is2d) {
    const int task = (ts >> 24) & 0xf, stage = (ts >> 16) & 0xf, event = (ts >> 20) & 0xf;
    const int target = (int16_t)(ts & 0xffff);
    if (task == 5 || task == 7) {
        // 2-D-native Target / ColorTarget: they speak on the teach() call that picked the target, and "Time up ." on the
        // one_channel step that ran out of time (xworld_task.py:205-211): back to idle with the target still recorded
        is2d = true;
        if (stage == 0 && event == 0 && target >= 0 && w.num_steps > 0 && w.one_channel) return pick_2d(T, task, true, -1, b, first);
        if (stage != 1 || tsteps != 0 || target < 0 || target >= w.cells) return false;
        // (bit 15 marks target goals; two groups: the 3-D stage may have moved the goal away since, then no icon is there)
        return pick_2d(T, task, false, (int)(cell_at(target) & 0x7fffu) - 1, b, first);
    }
    is2d = false;
    const int direction = task == 3 && target >= 0 ? (target >> 8) & 7 : 0;
    return pick_3d(T, task, stage, event, w.sent_names & 0xffffu, w.sent_names >> 16, direction, b, first);
}

// BatchedSimulator.sentence: does the teacher speak, and what -- the group the last teach() ran (exclusive scheduling), else
// the first group in conf order that speaks: Task::teacher_speak only records into an empty buffer (teaching_task.cpp:118-127).
// is2d: a 2-D-native task spoke, its draws start at block 4 * num_steps.
template <typename CellAt>
XWB_SENT_HD bool pick_env(const SentTab &T, const EnvWords &w, CellAt &cell_at, Slots &b, bool &first, bool &is2d) {
    const int ran = w.grp_order < 0 ? -1 : (w.grp_order >> 1) & 1;
    if (ran == 1) return w.two && pick_group(T, w, w.task_state2, w.task_steps2, cell_at, b, first, is2d);
    if (pick_group(T, w, w.task_state, w.task_steps, cell_at, b, first, is2d)) return true;
    if (ran == 0 || !w.two) return false;
    b = Slots();
    return pick_group(T, w, w.task_state2, w.task_steps2, cell_at, b, first, is2d);
}

}  // namespace sent
}  // namespace xwb
