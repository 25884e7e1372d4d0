// xwb_sentence_ids.hip -- the teacher's sentence of every env as word ids, in one launch (include/xwb.h xwb_set_vocabulary,
// xwb_sentence_max_words, xwb_sentence_ids) and its host twin (xwb_language_sentence_ids).
//
// The sentence of an env is a pure function of its live state and of xwb-rng-v1 stream 3 (xwb_language.h), so the device expands
// it itself: one lane per env reads what xwb_get_env_state / env_sentence read (task FSMs, episode, step count, bound name ids,
// the exclusive group order; for the 2-D-native tasks the one grid cell at the target), picks the group that spoke by
// env_sentence's rules and walks the grammar tables (xwb_sentence_ids.h) with an explicit stack in LDS.  The launch is ordered
// on the caller's stream only: it reads nothing the regeneration pass on the internal queue writes (that pass fills the
// shadow arrays), exactly like the copies of xwb_get_env_state.
#include "xwb_sim.h"
#include "xwb_language.h"

#include <algorithm>

using namespace xwb;
using namespace xwb::host;

namespace {

constexpr int SENT_BLOCK = 64;              // one wavefront per workgroup (256 measured the same: the lanes' serial expansion is the cost)
constexpr size_t SENT_TAB_LDS_MAX = 32768;     // tables up to this size are staged in LDS (+ 4 KiB of stacks)

struct SentIdsParams {
    int n, cells, max_len, one_channel;
    int32_t pad_id, silent_id;
    uint32_t seed, gid0;
    const int32_t *task_state, *task_steps, *task_state2, *task_steps2, *num_steps;
    const uint32_t *episode, *sent_names;
    const uint8_t *grp_order;                 // exclusive scheduling of two groups, else NULL
    const uint16_t *grid;
    sent::SentTab tab;
    int tab_lds;                              // the tables fit the launch's dynamic LDS: every block stages them there
    int32_t *ids, *len;
};

// BatchedSimulator._group_sentence / group_sentence (xwb_getters.hip) for one group's packed task state
__device__ __forceinline__ bool group_pick(const SentIdsParams &p, const sent::SentTab &T, int e, int32_t ts, int32_t tsteps, int32_t nsteps,
                                           sent::Slots &b, bool &first, bool &is2d) {
    const int task = (ts >> 24) & 0xf, stage = (ts >> 16) & 0xf, event = (ts >> 20) & 0xf;
    const int target = (int16_t)(ts & 0xffff);
    if (task == 5 || task == 7) {
        is2d = true;
        // the one_channel step that ran out of time: back to idle with the target still recorded
        if (stage == 0 && event == 0 && target >= 0 && nsteps > 0 && p.one_channel) return sent::pick_2d(T, task, true, -1, b, first);
        if (stage != 1 || tsteps != 0 || target < 0 || target >= p.cells) return false;
        const int icon = (int)(p.grid[(size_t)e * (size_t)p.cells + (size_t)target] & 0x7fffu) - 1;   // (bit 15: target goal)
        return sent::pick_2d(T, task, false, icon, b, first);
    }
    is2d = false;
    const uint32_t sn = p.sent_names[e];
    const int direction = task == 3 && target >= 0 ? (target >> 8) & 7 : 0;
    return sent::pick_3d(T, task, stage, event, sn & 0xffffu, sn >> 16, direction, b, first);
}

struct DevDraw {
    Stream st;
    bool first;
    __device__ __forceinline__ uint32_t operator()(uint32_t n) { return first ? 0u : st.below(n); }
};

struct DevEmit {
    int32_t *row;
    int32_t max_len;
    __device__ __forceinline__ void operator()(int32_t k, int32_t w) { if (k < max_len) row[k] = w; }
};

__global__ __launch_bounds__(SENT_BLOCK) void xw_sentence_ids_kernel(SentIdsParams p) {
    __shared__ int32_t stack[sent::STACK_MAX * SENT_BLOCK];
    extern __shared__ int32_t tab_lds[];
    // every symbol popped reads the tables: staged in LDS they are a short wait instead of a dependent L2 round trip per pop
    // (32768 envs: 24 us against 27 us reading them from global memory)
    sent::SentTab T = p.tab;
    if (p.tab_lds) {
        for (int i = threadIdx.x; i < T.total; i += SENT_BLOCK) tab_lds[i] = T.t[i];
        __syncthreads();
        T.t = tab_lds;
    }
    const int e = blockIdx.x * SENT_BLOCK + threadIdx.x;
    if (e >= p.n) return;
    const int32_t nsteps = p.num_steps[e];
    const int ran = p.grp_order ? (p.grp_order[e] >> 1) & 1 : -1;
    sent::Slots b;
    bool first = false, is2d = false, speaks;
    // env_sentence: the group the last teach() ran (exclusive scheduling), else the first group (conf order) that speaks --
    // Task::teacher_speak only records into an empty buffer
    if (ran == 1) speaks = p.task_state2 && group_pick(p, T, e, p.task_state2[e], p.task_steps2[e], nsteps, b, first, is2d);
    else {
        speaks = group_pick(p, T, e, p.task_state[e], p.task_steps[e], nsteps, b, first, is2d);
        if (!speaks && ran < 0 && p.task_state2) {
            b = sent::Slots();
            speaks = group_pick(p, T, e, p.task_state2[e], p.task_steps2[e], nsteps, b, first, is2d);
        }
    }
    int32_t *row = p.ids + (size_t)e * (size_t)p.max_len;
    int32_t n = -1;
    if (speaks) {
        DevDraw d;
        d.first = first;
        d.st.init(p.seed, p.gid0 + (uint32_t)e, p.episode[e], 3u);
        if (is2d) d.st.blk = 4u * (uint32_t)nsteps;          // language.sentence_2d: blocks 4 * num_steps onwards
        DevEmit out{row, p.max_len};
        n = sent::expand(T, b, d, stack + threadIdx.x, SENT_BLOCK, out);
    }
    if (n < 0) {                                               // silent (or a table / stack out of range)
        n = p.silent_id >= 0 ? 1 : 0;
        if (n) row[0] = p.silent_id;
    }
    for (int32_t k = n; k < p.max_len; ++k) row[k] = p.pad_id;
    p.len[e] = n;
}

struct HostEmit {
    std::vector<int32_t> *out;
    void operator()(int32_t, int32_t w) { out->push_back(w); }
};

struct HostDraw {
    lang::Stream *st;
    uint32_t operator()(uint32_t n) { return st ? st->below(n) : 0u; }
};

std::string sent_names_check(const char *const *names, int32_t n, std::vector<std::string> &out) {
    if (n < 0 || (n > 0 && !names)) return "NULL argument";
    for (int32_t i = 0; i < n; ++i) {
        if (!names[i]) return "NULL name";
        out.push_back(names[i]);
    }
    return "";
}

}  // namespace

namespace xwb {
namespace host {

int sentence_tables_rebuild(xwb_sim *s) {
    s->sent_tab_ok = false;
    std::vector<const char *> w;
    for (const std::string &x : s->vocab_words) w.push_back(x.c_str());
    lang::Vocab v;
    std::string err = lang::make_vocab(w.data(), (int32_t)w.size(), s->vocab_unk, s->vocab_fold, v);
    if (!err.empty()) return fail(XWB_ERR_ARG, err);
    lang::SentLayout L;
    err = lang::compile_sentence_tables(v, s->goal_names, s->icon_names, s->icon_colors, L);
    if (!err.empty()) return fail(XWB_ERR_ARG, err);
    XWB_ON_DEVICE(s);
    HIP_TRY(hipDeviceSynchronize());                           // a launch still reading the old tables
    const size_t bytes = L.tab.size() * sizeof(int32_t);
    if (bytes > s->sent_tab_cap) {
        if (s->d_sent_tab) HIP_TRY(hipFree(s->d_sent_tab));
        s->d_sent_tab = nullptr;
        s->sent_tab_cap = 0;
        HIP_TRY(hipMalloc(&s->d_sent_tab, bytes));
        s->sent_tab_cap = bytes;
    }
    HIP_TRY(hipMemcpy(s->d_sent_tab, L.tab.data(), bytes, hipMemcpyHostToDevice));
    s->sent_lay = L.lay;
    s->sent_lay.t = s->d_sent_tab;
    s->sent_tab_ok = true;
    return XWB_OK;
}

}  // namespace host
}  // namespace xwb

extern "C" {

int xwb_set_vocabulary(xwb_sim *s, const char *const *words, int32_t n_words, int32_t unk_id, int32_t fold_case) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_STATE, "not an xworld batch");
    lang::Vocab v;
    const std::string err = lang::make_vocab(words, n_words, unk_id, fold_case, v);
    if (!err.empty()) return fail(XWB_ERR_ARG, err);
    if (s->have_names) {                                       // the names must be single words of this vocabulary's lookup
        lang::SentLayout L;
        const std::string e2 = lang::compile_sentence_tables(v, s->goal_names, s->icon_names, s->icon_colors, L);
        if (!e2.empty()) return fail(XWB_ERR_ARG, e2);
    }
    s->vocab_words.assign(words, words + n_words);
    s->vocab_unk = unk_id;
    s->vocab_fold = fold_case != 0;
    s->have_vocab = true;
    s->sent_tab_ok = false;
    return s->have_names ? sentence_tables_rebuild(s) : XWB_OK;
}

int xwb_sentence_max_words(xwb_sim *s, int32_t *n) {
    if (!s || !n) return fail(XWB_ERR_ARG, "NULL argument");
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_STATE, "not an xworld batch");
    int32_t m = 1;                                             // the silent sentence ("-")
    auto add = [&](const int32_t *tasks, int32_t k) {
        for (int32_t i = 0; i < k; ++i) m = std::max(m, lang::max_sentence_words(tasks[i]));
    };
    static const int32_t only_target[1] = {XWB_TASK_TARGET};
    if (s->cfg.n_tasks > 0) add(s->cfg.tasks, s->cfg.n_tasks); else add(only_target, 1);
    add(s->cfg.tasks2, s->cfg.n_tasks2);
    *n = m;
    return XWB_OK;
}

int xwb_sentence_ids(xwb_sim *s, int32_t *ids_dev, int32_t *len_dev, int32_t max_len, int32_t pad_id, int32_t silent_id, void *stream) {
    if (!s || !ids_dev || !len_dev) return fail(XWB_ERR_ARG, "NULL argument");
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_STATE, "not an xworld batch");
    if (max_len < 1) return fail(XWB_ERR_ARG, "max_len < 1");
    if (!s->have_names || !s->have_vocab) return fail(XWB_ERR_STATE, "xwb_sentence_ids needs xwb_set_names and xwb_set_vocabulary");
    if (!s->sent_tab_ok) return fail(XWB_ERR_STATE, "the sentence tables failed to build (see the error of xwb_set_names / xwb_set_vocabulary)");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    SentIdsParams p{};
    p.n = s->n;
    p.cells = s->cfg.max_dim * s->cfg.max_dim;
    p.max_len = max_len;
    p.one_channel = s->cfg.task_mode == XWB_TASKMODE_ONE_CHANNEL;
    p.pad_id = pad_id;
    p.silent_id = silent_id;
    p.seed = s->cfg.seed;
    p.gid0 = s->cfg.env_gid0;
    p.task_state = s->d_task_state; p.task_steps = s->d_task_steps;
    p.task_state2 = s->d_task_state2; p.task_steps2 = s->d_task_steps2;
    p.num_steps = s->d_num_steps; p.episode = s->d_episode; p.sent_names = s->d_sent_names;
    p.grp_order = s->d_grp_order;
    p.grid = s->d_grid;
    p.tab = s->sent_lay;
    p.ids = ids_dev; p.len = len_dev;
    const size_t tab_bytes = (size_t)p.tab.total * sizeof(int32_t);
    p.tab_lds = tab_bytes <= SENT_TAB_LDS_MAX;
    const unsigned blocks = (unsigned)((s->n + SENT_BLOCK - 1) / SENT_BLOCK);
    hipLaunchKernelGGL(xw_sentence_ids_kernel, dim3(blocks), dim3(SENT_BLOCK), p.tab_lds ? tab_bytes : 0, as_stream(stream), p);
    HIP_TRY(hipGetLastError());
    return XWB_OK;
}

int xwb_language_sentence_ids(int32_t task, int32_t stage, int32_t event, const char *const *goal_names, int32_t n_goal_names,
                              uint32_t name_a, uint32_t name_b, int32_t direction, const char *color, uint32_t seed, uint32_t gid,
                              uint32_t episode, uint32_t num_steps, const char *const *words, int32_t n_words, int32_t unk_id,
                              int32_t fold_case, int32_t *ids, int32_t cap, int32_t *need) {
    if (!need || cap < 0 || (cap > 0 && !ids)) return fail(XWB_ERR_ARG, "NULL argument");
    std::vector<std::string> goals, inames, icolors;
    std::string err = sent_names_check(goal_names, n_goal_names, goals);
    if (!err.empty()) return fail(XWB_ERR_ARG, err);
    lang::Vocab v;
    err = lang::make_vocab(words, n_words, unk_id, fold_case, v);
    if (!err.empty()) return fail(XWB_ERR_ARG, err);
    const bool is2d = task == 5 || task == 7;
    if (is2d && event != 3) {                                  // one icon: the target's name and colour
        if (name_a >= (uint32_t)n_goal_names) return fail(XWB_ERR_ARG, "name_a out of range");
        if (task == 7 && !color) return fail(XWB_ERR_ARG, "NULL colour");
        inames.push_back(goals[name_a]);
        icolors.push_back(color ? color : "na");
    }
    lang::SentLayout L;
    err = lang::compile_sentence_tables(v, goals, inames, icolors, L);
    if (!err.empty()) return fail(XWB_ERR_ARG, err);
    L.lay.t = L.tab.data();
    sent::Slots b;
    bool first = false;
    const bool speaks = is2d ? sent::pick_2d(L.lay, task, event == 3, 0, b, first)
                             : sent::pick_3d(L.lay, task, stage, event, name_a, name_b, direction, b, first);
    std::vector<int32_t> out;
    if (speaks) {
        lang::Stream st(seed, gid, episode, 3);
        if (is2d) st.blk = 4 * num_steps;
        HostDraw d{first ? nullptr : &st};
        HostEmit e{&out};
        int32_t stack[sent::STACK_MAX];
        if (sent::expand(L.lay, b, d, stack, 1, e) < 0) return fail(XWB_ERR_ARG, "sentence expansion out of range");
    }
    *need = (int32_t)out.size();
    for (int32_t k = 0; k < *need && k < cap; ++k) ids[k] = out[k];
    return XWB_OK;
}

}  // extern "C"
