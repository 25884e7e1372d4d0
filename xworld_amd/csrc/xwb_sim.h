// xwb_sim.h -- internal to libxwb.so: the batch object behind the opaque xwb_sim of include/xwb.h, and what the host-side
// translation units share (xwb_create.hip: configuration, set-up, create / destroy; xwb_verbs.hip: reset / step and the queue
// hand-off; xwb_getters.hip: getters, per-env host access, packets, sentences; xwb_checkpoint.hip: save / load / copy envs).
//
// Who owns a device buffer: the d_* members hold what all three games share, the simple games' own state and the few XWorld2D
// buffers XwParams has no field for; every other XWorld2D buffer has ONE name, its field of xwb_sim::xw.
//
// A xwb_sim is the batched counterpart of simulator::SimulatorInterface (simulator_interface.h:40-89): it owns the SoA state
// of num_envs environments in HBM and sequences the kernels in the reference's call order (simulator_interface.cpp:95-143).
// No CPU fallback exists: without a usable gfx950 device xwb_create fails.
#pragma once
#include "../../include/xwb.h"
#include "../../include/xwb_testing.h"
#include "xwb_common.h"
#include "xwb_sentence_ids.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace xwb {
namespace host {

// sets xwb_last_error of the calling thread, returns `code` (xwb_create.hip)
int fail(int code, const std::string &msg);

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess)                                                                 \
            return ::xwb::host::fail(XWB_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

struct EventPair { hipEvent_t a, b; };

// Every entry point that touches the device runs with the batch's device current and restores the caller's
// device on return: two batches on different GPUs of one process, or a caller whose current device is not the
// batch's, launch on the right device.
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
        if (prev != dev) changed = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (changed && prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define XWB_ON_DEVICE(s) DeviceGuard _device_guard((s)->device)

struct KernelTimer {
    std::vector<EventPair> pool;
    size_t used = 0;
};

}  // namespace host
}  // namespace xwb

struct xwb_sim {
    xwb_config cfg;
    int device = 0;
    int n = 0;
    size_t obs_bytes_per_env = 0;
    int out_h = 0, out_w = 0, out_c = 0;
    int num_actions = 0;
    uint32_t policy_step = 0;
    bool list_valid = false;
    // what the last step call leaves for the verbs after it (xwb_verbs.hip): set by every xworld step call, cleared by
    // step_record_invalidate when the state it describes is replaced
    struct StepRecord {
        int path = XWB_PATH_NONE;          // the kernel sequence it ran; XWB_PATH_NONE: nothing of it is pending any more
        bool epochs = false;               // its hand-overs are epochs: a later verb's waiters wait for what its kernels publish
                                           // (kept by step_record_invalidate: xwb_step_path reports it)
        bool step_pub_queued = false;      // a kernel that publishes its epoch to sync[SYNC_STEP] is in the caller's queue (after a
                                           // fused launch that is xwb_reset_done's list render: until then, waiters use events)
    } rec;
    // xwb_xw_pack_grids: what the last frame-drawing verb read (xw_pack_grids_kernel's src) and how many such verbs ran since
    // the last pack (a context ring can only be replayed elsewhere one draw at a time)
    int frame_src = 0, draws_since_pack = 0;
    bool draw_off = false;                 // xwb_xw_set_draw(sim, 0): frames are not drawn (their consumer draws them from xwb_xw_pack_grids)
    bool autoreset_done = false;           // the last step call already reset the envs whose codes are still set
    bool step_open = false;                // a plain step call's finished envs still await their reset: xwb_copy_envs is refused
    // the done list lives in two buffers and its counter in three (xw.done_list, xw.done_ep, xw.done_count and xw.idle_count hold
    // the bases, xw_params picks the current ones), rotated by every xworld step call (list_sel, count_sel): step k
    // appends to list k & 1 / counter k % 3 and zeroes counter (k + 1) % 3, so the regeneration pass of step k - 1, which reads that
    // step's list and counter on the internal queue, is never in the way -- only the one of step k - 2 has to be through
    int count_sel = 0, list_sel = 0;
    uint64_t step_seq = 0;                 // xworld step calls so far
    bool profiling = false;
    xwb::host::KernelTimer t_render, t_step, t_reset, t_list;   // t_list: the list render (first frames of the envs a reset started)
    int last_path = XWB_PATH_NONE;         // xwb_step_path: which kernel sequence the last step call ran
    hipStream_t side = nullptr;            // reset of finished envs runs here, beside render_all
    uint32_t *d_minstd = nullptr;          // XWB_RNG_MINSTD: one engine state per env
    uint32_t epoch_step = 0, epoch_reset = 0;
    // queue hand-off mode (include/xwb.h xwb_queue_sync_mode): decided per caller stream by a one-time probe
    struct StreamProbe { hipStream_t st; bool ok; int reason; };
    std::vector<StreamProbe> probes;
    int sync_reason = XWB_SYNC_REASON_NOT_USED;
    uint32_t probe_token = 0;
    uint32_t *h_poison = nullptr;          // pinned host word: a watchdog expired (XwParams::poison_host points at it)
    bool poisoned = false;
    hipEvent_t ev_step = nullptr, ev_reset = nullptr, ev_term = nullptr, ev_cells = nullptr;
    hipEvent_t ev_view = nullptr;          // egocentric xwb_xw_render_view / xwb_xw_symbolic: the internal queue's later work follows their kernel
    hipEvent_t ev_results = nullptr;       // xwb_gather_results_beside's hand-over when the last step did not run on epochs (made on first use)
    // common device buffers
    int32_t *d_actions_in = nullptr;       // staging for xwb_step_host
    uint8_t *d_mask = nullptr;             // staging for xwb_reset_env
    int32_t *d_actions = nullptr, *d_num_steps = nullptr, *d_err = nullptr, *d_reset_partial = nullptr;   // (SgParams::reset_partial)
    uint32_t *d_episode = nullptr;
    float *d_reward = nullptr;
    uint8_t *d_done = nullptr, *d_success = nullptr;
    void *d_obs = nullptr, *d_obs_owned = nullptr;
    float2 *d_packed = nullptr;            // caller-owned (xwb_bind_results): slot 0 of the ring
    int64_t packed_slots = 1, packed_pos = 0;   // xwb_bind_results_ring: step call k writes slot k % slots
    // simple_game
    int32_t *d_pos = nullptr;
    uint8_t *d_flags = nullptr;
    // simple_race
    float *d_x = nullptr, *d_y = nullptr, *d_angle = nullptr;
    xwb::RaceParams race{};
    // pre-generated next episodes (XwParams::shadow / swap_shadow): xwb_step_autoreset's fast path
    bool pregen = false, shadow_ok = false, regen_pending = false, regen_by_epoch = false;
    bool regen_deferred = false;           // xwb_reset_done after a fused step: the pass is queued by the next verb (in the step's mode)
    int shadow_breaks = 0;                 // times another verb made the shadows stale (the lazy default path gives up after a few)
    uint32_t epoch_regen = 0, epoch_regen_prev = 0;   // epochs of the last two regeneration passes handed over by epoch ...
    uint64_t regen_seq = 0, regen_seq_prev = 0;       // ... and the step calls (step_seq) whose lists they read
    // look-ahead snapshots (XwParams::snap_grid_*): while snap_ok, set snap_sel holds the grids as the built-in policy's step
    // number snap_step with act_rep = snap_act_rep WILL leave them; every verb that writes the live state without patching the
    // snapshot clears snap_ok, and the next xwb_step then runs step -> render as two launches again
    uint16_t *d_snap_grid[2] = {nullptr, nullptr};
    int snap_sel = 0, snap_act_rep = 1;
    bool snap_ok = false;
    uint32_t snap_step = 0;
    int ego_cell_edge = 1;
    uint8_t *d_view_atlas = nullptr;       // full observation, xwb_xw_render_view: [n_icons + 1][64][64][3] B,G,R (entry 0: a white cell)
    std::vector<uint8_t> tile_table;   // host copy, n_icons x c x 12 x 12
    std::vector<int32_t> icon_type_h, icon_name_h, icon_colored_h;
    // xwb_set_names: the strings behind the name ids (the teacher's sentences are built from them)
    std::vector<std::string> goal_names, icon_names, icon_colors;
    bool have_names = false;
    // ... and the grammar tables compiled with them under an interning vocabulary, host only (xwb_language.h): xwb_sentence and
    // the state packets walk sent_host_lay and look the ids up in sent_words
    std::vector<int32_t> sent_host_tab;
    std::vector<std::string> sent_words;
    xwb::sent::SentTab sent_host_lay{};
    // xwb_set_vocabulary / xwb_sentence_ids (xwb_sentence_ids.hip): the caller's words, and the grammar tables compiled with them
    // and with the names above, uploaded to d_sent_tab (rebuilt when either changes)
    std::vector<std::string> vocab_words;
    int32_t vocab_unk = 0, vocab_fold = 0;
    bool have_vocab = false, sent_tab_ok = false;
    int32_t *d_sent_tab = nullptr;
    size_t sent_tab_cap = 0;
    xwb::sent::SentTab sent_lay{};
    xwb::XwParams xw{};                // XWorld2D: scalars and buffers; verbs launch with xw_params(s), a copy with the per-call fields filled in
    std::vector<void *> allocs;
};

namespace xwb {
namespace host {

template <typename T>                      // (T may be const: the tables of XwParams the kernels only read)
inline int dev_alloc(xwb_sim *s, T **p, size_t count, int fill = 0) {
    void *q = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    HIP_TRY(hipMalloc(&q, bytes));
    HIP_TRY(hipMemset(q, fill, bytes));
    s->allocs.push_back(q);
    *p = static_cast<T *>(q);
    return XWB_OK;
}

// a table made on the host: allocates it (dev_alloc's rules; room for `room` elements where the device reads past the table's
// end), uploads host[0 .. count) and assigns -- P is T, or const T for the read-only tables of XwParams, or the type the
// kernels read the same bytes as
template <typename P, typename T>
inline int dev_upload(xwb_sim *s, P **p, const T *host, size_t count, size_t room = 0) {
    T *q = nullptr;
    if (const int rc = dev_alloc(s, &q, count > room ? count : room)) return rc;
    if (count) HIP_TRY(hipMemcpy(q, host, count * sizeof(T), hipMemcpyHostToDevice));
    *p = reinterpret_cast<P *>(q);
    return XWB_OK;
}
template <typename P, typename T>
inline int dev_upload(xwb_sim *s, P **p, const std::vector<T> &host, size_t room = 0) { return dev_upload(s, p, host.data(), host.size(), room); }

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

extern const char *const POISON_MSG;
inline bool is_poisoned(xwb_sim *s) {
    if (!s->poisoned && s->h_poison && *(volatile uint32_t *)s->h_poison) s->poisoned = true;
    return s->poisoned;
}
#define XWB_TRY(expr) do { const int _rc = (expr); if (_rc) return _rc; } while (0)   // (a host helper's XWB_* code)
#define XWB_LIVE(s) do { if (::xwb::host::is_poisoned(s)) return ::xwb::host::fail(XWB_ERR_STATE, ::xwb::host::POISON_MSG); } while (0)

// ---- xwb_verbs.hip ----
// may calls on stream `st` hand over through epochs?  may_probe: only xwb_create and xwb_queue_sync_mode run the probe
bool use_epochs(xwb_sim *s, hipStream_t st, bool may_probe);
// the concurrency probe itself: do kernels of `st` and of the batch's internal queue run side by side?  (synchronises both)
bool epoch_probe(xwb_sim *s, hipStream_t st, int *reason);
// the probe, re-selecting the internal stream when it shares `st`'s hardware queue
bool side_beside(xwb_sim *s, hipStream_t st, int *reason);
// -1: the environment / a tool does not override the hand-over mode, 0: events, 1: epochs
int queue_sync_env(int *reason);
// the host wrote live state with the device idle (xwb_xw_load_map_task): the pre-generated episodes and the look-ahead
// snapshot no longer follow from it, and no regeneration pass is in flight.  The step record stays: the queues still hold what
// it says (xwb_gather_results_beside after a map replay waits for the same epoch as before it).
void pregen_invalidate(xwb_sim *s);
// ... and what a step call leaves behind is void as well (the whole live state was replaced): nothing of it is pending any more
void step_record_invalidate(xwb_sim *s);
void timer_begin(xwb_sim *s, KernelTimer &t, hipStream_t st);
void timer_end(xwb_sim *s, KernelTimer &t, hipStream_t st);
SgParams sg_params(xwb_sim *s);
RaceParams race_params(xwb_sim *s);
XwParams xw_params(xwb_sim *s);
int join_regen(xwb_sim *s, hipStream_t st);
int launch_regen(xwb_sim *s, bool by_epoch);
int flush_regen(xwb_sim *s);

// ---- xwb_sentence_ids.hip ----
// compiles the word-id tables from the vocabulary and the names and uploads them (synchronises the device); both must be set
int sentence_tables_rebuild(xwb_sim *s);

}  // namespace host
}  // namespace xwb
