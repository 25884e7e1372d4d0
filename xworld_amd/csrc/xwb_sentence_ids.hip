// xwb_sentence_ids.hip -- the teacher's sentence of every env as word ids, in one launch (include/xwb.h xwb_set_vocabulary,
// xwb_sentence_max_words, xwb_sentence_ids), and the same walk for one sentence on the host (xwb_language_sentence_ids).
//
// The sentence of an env is a pure function of its live state and of xwb-rng-v1 stream 3 (xwb_language.h), so the device expands
// it itself: one lane per env reads the packed words xwb_get_env_state unpacks (task FSMs, episode, step count, bound name ids,
// the exclusive group order; for the 2-D-native tasks the one grid cell at the target), picks the group that spoke
// (xwb_sentence_ids.h pick_env, as xwb_sentence does) and walks the grammar tables with an explicit stack in LDS.  The launch is ordered
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

struct DevCell {                             // the grid code under a cell of env e
    const uint16_t *grid;
    __device__ __forceinline__ uint16_t operator()(int cell) const { return grid[cell]; }
};

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
    sent::EnvWords w;
    w.task_state = p.task_state[e]; w.task_steps = p.task_steps[e];
    w.two = p.task_state2 != nullptr;
    w.task_state2 = w.two ? p.task_state2[e] : 0; w.task_steps2 = w.two ? p.task_steps2[e] : 0;
    w.num_steps = p.num_steps[e];
    w.sent_names = p.sent_names[e];
    w.grp_order = p.grp_order ? (int)p.grp_order[e] : -1;
    w.one_channel = p.one_channel != 0;
    w.cells = p.cells;
    DevCell cell{p.grid + (size_t)e * (size_t)p.cells};
    sent::Slots b;
    bool first = false, is2d = false;
    const bool speaks = sent::pick_env(T, w, cell, b, first, is2d);
    int32_t *row = p.ids + (size_t)e * (size_t)p.max_len;
    int32_t n = -1;
    if (speaks) {
        DevDraw d;
        d.first = first;
        d.st.init(p.seed, p.gid0 + (uint32_t)e, p.episode[e], 3u);
        if (is2d) d.st.blk = 4u * (uint32_t)w.num_steps;     // language.sentence_2d: blocks 4 * num_steps onwards
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
    const XwParams &x = s->xw;
    p.task_state = x.task_state; p.task_steps = x.task_steps;
    p.task_state2 = x.task_state2; p.task_steps2 = x.task_steps2;
    p.num_steps = s->d_num_steps; p.episode = s->d_episode; p.sent_names = x.sent_names;
    p.grp_order = x.grp_order;
    p.grid = x.grid;
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
    lang::Vocab v;
    std::string err = lang::make_vocab(words, n_words, unk_id, fold_case, v);
    std::vector<int32_t> out;
    if (err.empty())
        err = lang::hook_sentence(v, task == 5 || task == 7, task, stage, event, goal_names, n_goal_names, name_a, name_b, direction, color,
                                  seed, gid, episode, num_steps, out);
    if (!err.empty()) return fail(XWB_ERR_ARG, err);
    *need = (int32_t)out.size();
    for (int32_t k = 0; k < *need && k < cap; ++k) ids[k] = out[k];
    return XWB_OK;
}

}  // extern "C"
