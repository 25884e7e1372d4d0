// xwb_verbs.hip -- host side of libxwb.so, part 2: the verbs (reset / step / their variants) and the hand-off between the
// batch's two queues.  Kernel sequences follow the reference's call order (simulator_interface.cpp:95-143).
#include "xwb_sim.h"

using namespace xwb;
using namespace xwb::host;

namespace xwb {
namespace host {

// The step loop's two queues hand over through epochs in device memory (XwParams::sync) instead of event / barrier packets
// (3-6 us of idle GPU each).  A waiter polls until a kernel of the other queue has run.  Three things keep that safe
// (include/xwb.h, xwb_queue_sync_mode): publishers are enqueued before their waiters everywhere below; epochs are only used on
// a caller stream that passed a concurrency probe against s->side (epoch_probe); a watchdog poisons the batch.
// Overrides of the AUTO mode: XWB_QUEUE_SYNC=events|epochs, and tools that serialise kernel execution (rocprofv3's counter
// collection: ROCPROF_COUNTER_COLLECTION / ROCPROF_COUNTERS; AMD_SERIALIZE_KERNEL; HIP_LAUNCH_BLOCKING) -> events.
// returns -1: no override, 0: events, 1: epochs; *reason = XWB_SYNC_REASON_ENV | _TOOL
int queue_sync_env(int *reason) {
    static int mode = -2, why = 0;
    if (mode == -2) {
        auto on = [](const char *name) { const char *v = getenv(name); return v && *v && strcmp(v, "0") != 0; };
        mode = -1;
        if (on("ROCPROF_COUNTER_COLLECTION") || getenv("ROCPROF_COUNTERS") || on("AMD_SERIALIZE_KERNEL") || on("HIP_LAUNCH_BLOCKING") ||
            on("CUDA_LAUNCH_BLOCKING")) { mode = 0; why = XWB_SYNC_REASON_TOOL; }
        if (const char *v = getenv("XWB_QUEUE_SYNC")) {
            if (strcmp(v, "events") == 0) { mode = 0; why = XWB_SYNC_REASON_ENV; }
            else if (strcmp(v, "epochs") == 0) { mode = 1; why = XWB_SYNC_REASON_ENV; }
        }
    }
    *reason = why;
    return mode;
}

// the next epoch of a counter (0 means "nothing to wait for")
uint32_t next_epoch(uint32_t &e) {
    if (++e == 0) e = 1;
    return e;
}

// One-time probe of (caller stream, s->side): do kernels of the two really run concurrently?  A waiter with a 2 ms watchdog
// is enqueued FIRST on one stream, its publisher on the other, in both directions; on streams that share a hardware queue
// (or under a tool that serialises kernels) the waiter runs alone, expires and raises the probe's own flag
// (sync[SYNC_PROBE_EXPIRED], not the batch's poison word).  Both streams are drained before and after, so work of the caller that is still queued cannot
// make the probe fail (or be delayed by it) -- the cost is one synchronisation the first time a stream is seen.
bool epoch_probe(xwb_sim *s, hipStream_t st, int *reason) {
    auto bad = [&](int why) { (void)hipGetLastError(); *reason = why; return false; };
    if (hipStreamSynchronize(st) != hipSuccess || hipStreamSynchronize(s->side) != hipSuccess) return bad(XWB_SYNC_REASON_PROBE_ERROR);
    if (hipMemsetAsync(s->xw.sync + SYNC_PROBE_EXPIRED, 0, sizeof(uint32_t), s->side) != hipSuccess || hipStreamSynchronize(s->side) != hipSuccess)
        return bad(XWB_SYNC_REASON_PROBE_ERROR);
    for (int dir = 0; dir < 2; ++dir) {
        hipStream_t waiter = dir ? st : s->side, publisher = dir ? s->side : st;
        next_epoch(s->probe_token);
        if (launch_xw_wait(s->xw.sync + SYNC_PROBE, s->probe_token, s->xw.sync + SYNC_PROBE_EXPIRED, nullptr, waiter, 200000ull) != hipSuccess)   // 2 ms
            return bad(XWB_SYNC_REASON_PROBE_ERROR);
        if (launch_xw_signal(s->xw.sync + SYNC_PROBE, s->probe_token, publisher) != hipSuccess) return bad(XWB_SYNC_REASON_PROBE_ERROR);
        if (hipStreamSynchronize(waiter) != hipSuccess || hipStreamSynchronize(publisher) != hipSuccess) return bad(XWB_SYNC_REASON_PROBE_ERROR);
    }
    uint32_t expired = 1;
    if (hipMemcpy(&expired, s->xw.sync + SYNC_PROBE_EXPIRED, sizeof expired, hipMemcpyDeviceToHost) != hipSuccess) return bad(XWB_SYNC_REASON_PROBE_ERROR);
    if (expired) {
        (void)hipMemset(s->xw.sync + SYNC_PROBE_EXPIRED, 0, sizeof(uint32_t));
        *reason = XWB_SYNC_REASON_PROBE_FAILED;
        return false;
    }
    *reason = XWB_SYNC_REASON_PROBE_OK;
    return true;
}

// Make s->side a stream whose kernels run beside those of `st`.  HIP maps streams onto a few hardware queues
// (GPU_MAX_HW_QUEUES, 4) in creation order; an internal queue that shares the CALLER's hardware queue runs nothing beside the
// caller's kernels: the map generator then follows the render it was meant to hide behind (C4: 0.190 instead of 0.113 ms per
// step -- seen with the first batch created after an RCCL communicator, and with pool streams of the caller).  If the probe
// of (st, side) finds no concurrency, up to seven further streams are tried; a candidate must also still run beside every
// stream that passed its probe earlier.  The old stream is idle when it is replaced (the probe drains it).  Returns the
// verdict for `st`; nothing changes when no candidate passes.
bool side_beside(xwb_sim *s, hipStream_t st, int *reason) {
    if (epoch_probe(s, st, reason) || *reason != XWB_SYNC_REASON_PROBE_FAILED) return *reason == XWB_SYNC_REASON_PROBE_OK;
    // the streams that passed earlier are probed again against each candidate -- but only those that are still alive: a caller
    // may have destroyed one without xwb_queue_sync_forget.  hipStreamQuery validates the handle (hipSuccess / hipErrorNotReady
    // for a live stream); anything else means "forget this stream", not "candidate rejected".
    std::vector<hipStream_t> keep;
    for (size_t i = 0; i < s->probes.size();) {
        const hipStream_t q = s->probes[i].st;
        if (q != st && q != nullptr) {
            const hipError_t live = hipStreamQuery(q);
            if (live != hipSuccess && live != hipErrorNotReady) { (void)hipGetLastError(); s->probes.erase(s->probes.begin() + (long)i); continue; }
        }
        if (s->probes[i].ok && q != st) keep.push_back(q);
        ++i;
    }
    hipStream_t original = s->side;
    std::vector<hipStream_t> rejected;                              // kept alive until the choice is made: the next one maps elsewhere
    bool found = false;
    for (int attempt = 0; attempt < 7 && !found; ++attempt) {
        hipStream_t alt = nullptr;
        if (hipStreamCreateWithFlags(&alt, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
        s->side = alt;
        int r = 0;
        found = epoch_probe(s, st, &r);
        for (size_t k = 0; found && k < keep.size(); ++k) found = epoch_probe(s, keep[k], &r);
        if (!found) rejected.push_back(alt);
    }
    for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
    if (!found) { s->side = original; *reason = XWB_SYNC_REASON_PROBE_FAILED; return false; }
    (void)hipStreamDestroy(original);
    for (size_t i = 0; i < s->probes.size();)                       // verdicts of "no concurrency" were about the old stream
        if (!s->probes[i].ok) s->probes.erase(s->probes.begin() + (long)i); else ++i;
    *reason = XWB_SYNC_REASON_PROBE_OK;
    return true;
}

// may calls on stream `st` hand over through epochs?  (xworld batches only: the other games have no internal stream)
// may_probe: only xwb_create (the default stream) and xwb_queue_sync_mode (any stream, an explicit call) run the probe -- it
// synchronises both streams and the host; the step verbs never do: a stream nobody probed hands over through events.
bool use_epochs(xwb_sim *s, hipStream_t st, bool may_probe) {
    if (!s->xw.sync || !s->side) { s->sync_reason = XWB_SYNC_REASON_NOT_USED; return false; }
    if (s->cfg.queue_sync == XWB_QUEUE_SYNC_EVENTS) { s->sync_reason = XWB_SYNC_REASON_CONFIG; return false; }
    if (s->cfg.queue_sync == XWB_QUEUE_SYNC_EPOCHS) { s->sync_reason = XWB_SYNC_REASON_CONFIG; return true; }
    int why = 0;
    const int env = queue_sync_env(&why);
    if (env >= 0) { s->sync_reason = why; return env == 1; }
    for (auto &pr : s->probes) if (pr.st == st) { s->sync_reason = pr.reason; return pr.ok; }
    if (!may_probe) { s->sync_reason = XWB_SYNC_REASON_NOT_PROBED; return false; }
    {   // a stream under graph capture cannot be synchronised (the probe would invalidate the capture): events, nothing cached
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
        if (cap != hipStreamCaptureStatusNone) { s->sync_reason = XWB_SYNC_REASON_NOT_PROBED; return false; }
    }
    int reason = 0;
    const bool ok = side_beside(s, st, &reason);
    if (s->probes.size() >= 16) s->probes.erase(s->probes.begin());
    s->probes.push_back(xwb_sim::StreamProbe{st, ok, reason});
    s->sync_reason = reason;
    return ok;
}


void timer_begin(xwb_sim *s, KernelTimer &t, hipStream_t st) {
    if (!s->profiling) return;
    if (t.used == t.pool.size()) {
        EventPair ep;
        if (hipEventCreate(&ep.a) != hipSuccess || hipEventCreate(&ep.b) != hipSuccess) return;
        t.pool.push_back(ep);
    }
    (void)hipEventRecord(t.pool[t.used].a, st);
}

void timer_end(xwb_sim *s, KernelTimer &t, hipStream_t st) {
    if (!s->profiling || t.used >= t.pool.size()) return;
    (void)hipEventRecord(t.pool[t.used].b, st);
    t.used++;
}

// the results slot of the step call being queued (xwb_bind_results_ring)
float2 *packed_slot(xwb_sim *s) {
    return s->d_packed ? s->d_packed + (size_t)(s->packed_pos % s->packed_slots) * (size_t)s->n : nullptr;
}

SgParams sg_params(xwb_sim *s) {
    SgParams p{};
    const xwb_config &c = s->cfg;
    p.n = s->n; p.array_size = c.array_size; p.context = c.context; p.max_steps = c.max_steps;
    p.act_rep = 1; p.mode = MODE_STEP; p.auto_reset = 0;
    p.policy_seed = c.policy_seed; p.env_gid0 = c.env_gid0; p.policy_step = s->policy_step;
    p.actions = nullptr; p.mask = nullptr; p.actions_out = s->d_actions;
    p.pos = s->d_pos; p.flags = s->d_flags; p.num_steps = s->d_num_steps; p.episode = s->d_episode;
    p.reward = s->d_reward; p.done = s->d_done; p.obs = static_cast<uint8_t *>(s->d_obs);
    p.packed = packed_slot(s);
    p.n_steps = 1;
    p.err_count = s->d_err; p.reset_partial = nullptr;
    return p;
}

RaceParams race_params(xwb_sim *s) {
    RaceParams p = s->race;
    const xwb_config &c = s->cfg;
    p.n = s->n; p.context = c.context; p.max_steps = c.max_steps; p.act_rep = 1; p.mode = MODE_STEP;
    p.auto_reset = 0;
    p.policy_seed = c.policy_seed; p.env_gid0 = c.env_gid0; p.policy_step = s->policy_step; p.seed = c.seed;
    p.actions = nullptr; p.mask = nullptr; p.actions_out = s->d_actions;
    p.x = s->d_x; p.y = s->d_y; p.angle = s->d_angle; p.num_steps = s->d_num_steps; p.episode = s->d_episode;
    p.reward = s->d_reward; p.done = s->d_done; p.obs = static_cast<float *>(s->d_obs);
    p.packed = packed_slot(s);
    p.n_steps = 1;
    p.err_count = s->d_err; p.reset_partial = nullptr;
    p.minstd = s->d_minstd;
    return p;
}

// The simple games' one kernel: `n_steps` steps (MODE_STEP; `autoreset`: finished envs start their next episode inside it) or a
// reset of the envs `mode` selects.  A launch that may reset envs writes its per-workgroup counts (xwb_done_count reports the
// last such launch).
int simple_launch(xwb_sim *s, int mode, const uint8_t *mask, const int32_t *actions, int32_t act_rep, bool autoreset, int32_t n_steps,
                  hipStream_t st) {
    KernelTimer &t = mode == MODE_STEP ? s->t_step : s->t_reset;
    auto fill = [&](auto &p) {
        p.mode = mode; p.mask = mask; p.actions = actions; p.act_rep = act_rep; p.auto_reset = autoreset ? 1 : 0; p.n_steps = n_steps;
        if (mode != MODE_STEP || autoreset) p.reset_partial = s->d_reset_partial;
    };
    timer_begin(s, t, st);
    if (s->cfg.game == XWB_SIMPLE_GAME) {
        SgParams p = sg_params(s);
        fill(p);
        HIP_TRY(launch_simple_game(p, st));
    } else {
        RaceParams p = race_params(s);
        fill(p);
        HIP_TRY(launch_simple_race(p, st));
    }
    timer_end(s, t, st);
    return XWB_OK;
}

// The parameters of a launch: s->xw with the fields that change from call to call -- the caller's frames and results slot, the
// policy's step number, and the current buffers of the rotations, whose bases s->xw holds (xwb_sim.h count_sel, list_sel)
XwParams xw_params(xwb_sim *s) {
    XwParams p = s->xw;
    p.obs = static_cast<uint8_t *>(s->d_obs);
    p.packed = packed_slot(s);
    p.policy_step = s->policy_step;
    p.no_draw = s->draw_off ? 1 : 0;
    p.list_flag = 2;
    p.done_list += (size_t)s->list_sel * (size_t)s->n;
    p.done_ep += (size_t)s->list_sel * (size_t)s->n;
    p.done_count_next = p.done_count + (s->count_sel + 1) % 3;
    p.done_count += s->count_sel;
    if (p.idle_count) { p.idle_count_next = p.idle_count + (s->count_sel + 1) % 3; p.idle_count += s->count_sel; }
    return p;
}

// the reset kernel's parameters for a pre-generation pass: episode[e] + 1 of the listed envs into the shadow arrays
XwParams shadow_params(xwb_sim *s) {
    XwParams q = xw_params(s);
    q.shadow = 1; q.auto_reset = AUTO_RESET_KEEP; q.sig_epoch = 0; q.wait_epoch = 0; q.packed = nullptr;
    q.grid = q.sh_grid; q.agent_xy = q.sh_agent_xy; q.task_state = q.sh_task_state; q.task_state2 = q.sh_task_state2;
    q.sent_names = q.sh_sent_names; q.cand2d = q.sh_cand2d; q.goal_cells = q.sh_goal_cells;
    return q;
}

// ---- hand-overs between the caller's queue and the internal one ----
// A hand-over is a sync word (epochs) and the event that stands in for it when the call hands over through events.
struct HandOver { SyncSlot slot; hipEvent_t xwb_sim::*ev; };
const HandOver STEP_DONE{SYNC_STEP, &xwb_sim::ev_step};
const HandOver RESET_DONE{SYNC_RESET, &xwb_sim::ev_reset};
const HandOver REGEN_DONE{SYNC_REGEN, &xwb_sim::ev_reset};
const HandOver SPAN_CELLS_DONE{SYNC_SPAN_CELLS, &xwb_sim::ev_cells};
const HandOver TERM_DONE{SYNC_SPAN_TERM, &xwb_sim::ev_term};

// publish `h` on queue `q`: behind the work queued there so far (a one-thread signal kernel, or an event record)
int publish(xwb_sim *s, const HandOver &h, bool by_epoch, uint32_t epoch, hipStream_t q) {
    if (by_epoch) HIP_TRY(launch_xw_signal(s->xw.sync + h.slot, epoch, q));
    else HIP_TRY(hipEventRecord(s->*h.ev, q));
    return XWB_OK;
}

// order the work queued on `q` from here on after `h` (a one-wavefront waiter under the batch's watchdog, or an event wait)
int order_after(xwb_sim *s, const HandOver &h, bool by_epoch, uint32_t epoch, hipStream_t q) {
    if (by_epoch) HIP_TRY(launch_xw_wait(s->xw.sync + h.slot, epoch, s->xw.sync + SYNC_POISON, s->xw.poison_host, q));
    else HIP_TRY(hipStreamWaitEvent(q, s->*h.ev, 0));
    return XWB_OK;
}

void pregen_invalidate(xwb_sim *s) {
    s->shadow_ok = false; s->regen_pending = false; s->regen_deferred = false; s->snap_ok = false;
}

void step_record_invalidate(xwb_sim *s) {
    s->rec.path = XWB_PATH_NONE;
    s->rec.step_pub_queued = false;
    pregen_invalidate(s);
}

// A regeneration pass of xwb_step_autoreset may still be reading the done list and the episode counters on the side queue:
// every other verb that touches them orders `st` behind it first (the next xwb_step_autoreset waits inside its step kernel).
int join_regen(xwb_sim *s, hipStream_t st) {
    XWB_TRY(flush_regen(s));
    if (!s->regen_pending) return XWB_OK;
    XWB_TRY(order_after(s, REGEN_DONE, s->regen_by_epoch, s->epoch_regen, st));
    s->regen_pending = false;
    return XWB_OK;
}

// The regeneration pass of the lazy loop: the episodes after the ones the last step's finished envs are about to start (or have
// just started), into the free shadow slots, on the internal queue behind that step's kernel.
int launch_regen(xwb_sim *s, bool by_epoch) {
    XwParams q = shadow_params(s);
    XWB_TRY(order_after(s, STEP_DONE, by_epoch, s->epoch_step, s->side));
    timer_begin(s, s->t_reset, s->side);
    HIP_TRY(launch_xw_reset(q, MODE_RESET_DONE, s->side));
    timer_end(s, s->t_reset, s->side);
    if (by_epoch) {
        s->epoch_regen_prev = s->epoch_regen; s->regen_seq_prev = s->regen_seq; s->regen_seq = s->step_seq;
        next_epoch(s->epoch_regen);
    }
    XWB_TRY(publish(s, REGEN_DONE, by_epoch, s->epoch_regen, s->side));
    s->regen_pending = true; s->regen_by_epoch = by_epoch;
    return XWB_OK;
}

// ... which xwb_reset_done leaves to the next verb after a fused step (see there): every verb that steps, or that touches what
// the pass reads or writes (join_regen), queues it first -- with the list and counter of the step it belongs to still current
// (and its hand-over mode: only a step call changes s->rec.epochs, after this)
int flush_regen(xwb_sim *s) {
    if (!s->regen_deferred) return XWB_OK;
    s->regen_deferred = false;
    return launch_regen(s, s->rec.epochs);
}

// ---- pieces the reset routines and xwb_step_autoreset share ----
// the map generator for the envs `mode` selects and, under egocentric observation off the span path, their goal images; timed
int launch_reset(xwb_sim *s, const XwParams &p, int mode, bool warp, hipStream_t q) {
    timer_begin(s, s->t_reset, q);
    HIP_TRY(launch_xw_reset(p, mode, q));
    if (warp) HIP_TRY(launch_xw_warp_goals(p, mode != MODE_RESET_ALL, q));
    timer_end(s, s->t_reset, q);
    return XWB_OK;
}

// a render under timer `t` (t_render: every env / the alive ones; t_list: the first frames of the listed envs)
int launch_render(xwb_sim *s, KernelTimer &t, const XwParams &p, RenderMode how, hipStream_t q) {
    timer_begin(s, t, q);
    HIP_TRY(launch_xw_render(p, how, q));
    timer_end(s, t, q);
    return XWB_OK;
}

// What a step call runs, decided once at its top.
struct StepPlan {
    int path;          // XWB_PATH_*: the kernel sequence
    bool epochs;       // the hand-overs are epochs: what xwb_create / xwb_queue_sync_mode found out about `st`; events for a
                       // stream nobody probed (no verb synchronises the host by itself)
    bool snaps;        // the step also writes the look-ahead snapshot for the next one (XwParams::snap_grid_out)
};

StepPlan choose_path(xwb_sim *s, const int32_t *actions_dev, int32_t act_rep, bool autoreset, hipStream_t st) {
    StepPlan k{XWB_PATH_CLASSIC, use_epochs(s, st, false), false};
    if (s->cfg.visible_radius) {
        k.path = xw_ego_span(s->xw) ? XWB_PATH_EGO_SPAN : XWB_PATH_EGO_PER_ENV;
    } else if (autoreset) {
        // xwb_step_autoreset with pre-generated episodes (XwParams::swap_shadow): the step kernel starts the next episode of
        // the envs it finishes, ONE render draws every env, the side queue regenerates the consumed shadows beside it
        if (s->pregen) k.path = XWB_PATH_PREGEN;
    } else if (s->pregen && s->shadow_breaks < 3 && !(s->cfg.debug_flags & XWB_DEBUG_NO_LAZY)) {
        // ... and a plain step whose xwb_reset_done installs them (XwParams::list_swap): no terminal snapshot, the render reads
        // the live grid.  Only while the caller's verbs leave the shadows alone (a loop of masked / single resets would pay a
        // whole-batch regeneration per call: after a few such breaks the batch stays on the classic path).
        // Under the built-in policy it also writes the grids as the NEXT step will leave them (XwParams::snap_grid_out); when the
        // previous verbs kept such a snapshot current for exactly this step, this call is ONE launch: render blocks that draw from
        // it, step blocks beside them.
        k.snaps = s->d_snap_grid[0] != nullptr && actions_dev == nullptr;
        const bool fused = k.snaps && s->snap_ok && s->snap_step == s->policy_step && s->snap_act_rep == act_rep && !s->draw_off;
        k.path = fused ? XWB_PATH_LAZY_FUSED : XWB_PATH_LAZY;
    }
    return k;
}

bool is_lazy(int path) { return path == XWB_PATH_LAZY || path == XWB_PATH_LAZY_FUSED; }

// XWB_PATH_PREGEN: every env from its live grid; the render publishes the step epoch, the regeneration pass follows it
int step_pregen(xwb_sim *s, XwParams &p, bool epochs, hipStream_t st) {
    if (!epochs) { p.sig_epoch = 0; XWB_TRY(publish(s, STEP_DONE, false, 0, st)); }
    XWB_TRY(launch_render(s, s->t_render, p, RENDER_ALL, st));
    return launch_regen(s, epochs);
}

// xwb_step_autoreset without pre-generated episodes: reset + first frame of the new episode of the finished envs on the side
// stream, beside the render of everyone else; their terminal frames are not materialised.
// Epochs (full observation, and the egocentric span path, whose cells kernel publishes the step epoch): the side queue's first
// kernel waits for "step kernel complete", which the FIRST kernel of the render publishes; a one-wavefront kernel at the end of
// this call waits for the side queue's.  The render is enqueued BEFORE the side queue's waiter (publisher first: xw_device.h),
// and the side queue's signal before the final waiter.
int step_autoreset_classic(xwb_sim *s, XwParams &p, bool epochs, bool span, hipStream_t st) {
    const bool ep = epochs && (!p.visible_radius || span);
    if (!ep) { p.sig_epoch = 0; XWB_TRY(publish(s, STEP_DONE, false, 0, st)); }
    XWB_TRY(launch_render(s, s->t_render, p, RENDER_ALIVE, st));
    XWB_TRY(order_after(s, STEP_DONE, ep, s->epoch_step, s->side));
    if (ep) next_epoch(s->epoch_reset);
    XwParams pr = xw_params(s);
    pr.sig_epoch = 0; pr.auto_reset = AUTO_RESET_KEEP;
    // (span path: the goal images of the reset envs are redrawn in the list render's first launch, beside their cell tables;
    // nothing else reads them -- the big render's kernels skip the finished envs)
    XWB_TRY(launch_reset(s, pr, MODE_RESET_DONE, pr.visible_radius && !span, s->side));
    XWB_TRY(launch_render(s, s->t_list, pr, span ? RENDER_LIST_WARP : RENDER_LIST, s->side));
    XWB_TRY(publish(s, RESET_DONE, ep, s->epoch_reset, s->side));      // queued behind the list render
    return order_after(s, RESET_DONE, ep, s->epoch_reset, st);
}

// XWB_PATH_LAZY_FUSED: the step is complete when this kernel is: nothing publishes its epoch here -- xwb_reset_done's list
// render does
int step_fused(xwb_sim *s, XwParams &p, bool epochs, hipStream_t st) {
    p.sig_epoch = 0;
    timer_begin(s, s->t_render, st);
    HIP_TRY(launch_xw_step_render(p, st));
    timer_end(s, s->t_render, st);
    if (!epochs) XWB_TRY(publish(s, STEP_DONE, false, 0, st));
    return XWB_OK;
}

// xwb_step's render on the classic, lazy and egocentric paths.  Classic: finished envs keep a terminal snapshot of their grid
// (step kernel) from which the big render draws their last frame, so a following xwb_reset_done can regenerate the live state
// beside that render right away (lazy: nothing rewrites the live grid beside it).  The egocentric render reads more than the grid
// (heading, goal images): there the terminal frames are rendered from the (short) list on the side stream, beside the big render,
// which skips those envs; a following xwb_reset_done queues behind that list render.  On the span path (kernels_xworld_ego_span.hip)
// only the front kernels read the env state: its hand-overs are published behind them, the terminal frames leave through a short
// list gather and the big gather skips them.
int step_plain(xwb_sim *s, XwParams &p, bool epochs, int path, hipStream_t st) {
    const bool per_env = path == XWB_PATH_EGO_PER_ENV;
    if (per_env || (!p.visible_radius && !epochs)) XWB_TRY(publish(s, STEP_DONE, false, 0, st));
    if (per_env) {
        XwParams pr = xw_params(s);
        pr.sig_epoch = 0; pr.list_flag = 1; pr.ego_list_beside = 1;
        XWB_TRY(order_after(s, STEP_DONE, false, 0, s->side));
        HIP_TRY(launch_xw_render(pr, RENDER_LIST, s->side));
        XWB_TRY(publish(s, TERM_DONE, false, 0, s->side));
    }
    timer_begin(s, s->t_render, st);
    if (path == XWB_PATH_EGO_SPAN) {
        p.list_flag = 1;
        if (epochs) HIP_TRY(launch_xw_render(p, RENDER_SPAN_STEP, st));          // (p.sig_epoch: sync[SYNC_SPAN_*])
        else HIP_TRY(launch_xw_render(p, RENDER_SPAN_STEP, st, s->ev_step, s->ev_term, s->ev_cells));
    } else {
        HIP_TRY(launch_xw_render(p, p.visible_radius ? RENDER_ALIVE : (is_lazy(path) ? RENDER_ALL : RENDER_ALL_TERM), st));
    }
    timer_end(s, s->t_render, st);
    if (per_env) XWB_TRY(order_after(s, TERM_DONE, false, 0, st));
    return XWB_OK;
}

int do_step(xwb_sim *s, const int32_t *actions_dev, int32_t act_rep, bool autoreset, hipStream_t st) {
    if (act_rep < 1) return fail(XWB_ERR_ARG, "act_rep must be >= 1");
    if (s->cfg.game != XWB_XWORLD2D) {
        XWB_TRY(simple_launch(s, MODE_STEP, nullptr, actions_dev, act_rep, autoreset, 1, st));
    } else {
        XWB_TRY(flush_regen(s));
        const StepPlan k = choose_path(s, actions_dev, act_rep, autoreset, st);
        const bool lazy = is_lazy(k.path), pregen = k.path == XWB_PATH_PREGEN;
        if (pregen || lazy) {
            if (!s->shadow_ok) {               // first use, or another verb reset envs since: make every env's next episode
                XWB_TRY(join_regen(s, st));
                HIP_TRY(launch_xw_reset(shadow_params(s), MODE_RESET_ALL, st));
                s->shadow_ok = true;
            } else if (s->regen_pending && !s->regen_by_epoch) {
                XWB_TRY(join_regen(s, st));    // (events: the step kernel cannot wait for itself)
            }
        } else {
            XWB_TRY(join_regen(s, st));
        }
        s->count_sel = (s->count_sel + 1) % 3; // this step appends to the counter the previous one zeroed ...
        s->list_sel ^= 1;                      // ... and to the list the one before it filled
        s->step_seq += 1;
        XwParams p = xw_params(s);
        p.actions = actions_dev; p.act_rep = act_rep;
        if (pregen) { p.swap_shadow = 1; p.regen_wait = s->regen_pending ? s->epoch_regen : 0; }   // (it rewrites shadows: the newest pass)
        if (lazy) {
            // the buffers this step writes were last read by the regeneration pass of the step call two back (xwb_sim.h count_sel)
            p.swap_shadow = 2;
            p.regen_wait = !s->regen_pending || !s->regen_by_epoch ? 0u : (s->regen_seq + 2 <= s->step_seq ? s->epoch_regen : s->epoch_regen_prev);
        }
        const bool fused = k.path == XWB_PATH_LAZY_FUSED;
        if (k.snaps) {
            p.snap_grid_out = s->d_snap_grid[s->snap_sel ^ 1];
            if (fused) p.snap_grid_in = s->d_snap_grid[s->snap_sel];
        }
        const uint32_t epoch = next_epoch(s->epoch_step);
        p.sig_epoch = k.epochs ? epoch : 0;    // published by the kernel behind the step kernel
        if (!fused) {
            timer_begin(s, s->t_step, st);
            HIP_TRY(launch_xw_step(p, st));
            // exclusive scheduling of two groups: idle XWorld3DNav* groups the step picked run their idle stage now
            if (p.idle_list) HIP_TRY(launch_xw_idle3d(p, st));
            timer_end(s, s->t_step, st);
        }
        if (k.snaps) s->snap_sel ^= 1;
        s->snap_ok = k.snaps;
        s->snap_step = s->policy_step + 1u;
        s->snap_act_rep = act_rep;
        if (pregen) XWB_TRY(step_pregen(s, p, k.epochs, st));
        else if (autoreset) XWB_TRY(step_autoreset_classic(s, p, k.epochs, k.path == XWB_PATH_EGO_SPAN, st));
        else if (fused) XWB_TRY(step_fused(s, p, k.epochs, st));
        else XWB_TRY(step_plain(s, p, k.epochs, k.path, st));
        s->list_valid = !autoreset;
        s->rec.path = k.path;
        s->rec.epochs = k.epochs;
        s->rec.step_pub_queued = !fused;
        // (a plain step on the classic path drew the finished envs from their terminal snapshots)
        s->frame_src = k.path == XWB_PATH_CLASSIC && !autoreset ? PACK_SRC_TERM : PACK_SRC_LIVE;
        s->draws_since_pack += 1;
    }
    s->last_path = s->rec.path;
    s->policy_step += 1;
    s->packed_pos += 1;
    s->autoreset_done = autoreset;
    s->step_open = !autoreset;
    return XWB_OK;
}

// ---- the reset side ----
// Which queue timeline a reset verb runs, decided once (run_reset).
enum ResetPath {
    RESET_ON_CALLER,         // everything on the caller's stream: the whole batch, a mask, a rebuilt list, or the done list of a lazy
                             // step whose shadows another verb made stale
    RESET_BESIDE_FULL,       // the done list of the step just queued: map generator on the internal queue beside render_all
    RESET_BESIDE_SPAN,       // ... beside the egocentric span render, with its three hand-overs
    RESET_BESIDE_PER_ENV,    // ... beside the per-env egocentric render
    RESET_INSTALL,           // after a lazy / fused step: the list render installs the pre-generated episodes
};
struct ResetPlan {
    ResetPath path;
    bool epochs;             // the routine's hand-overs are epochs
};

ResetPlan choose_reset(xwb_sim *s, int mode) {
    ResetPlan k{RESET_ON_CALLER, false};
    // only the list the last step call left, untouched since, can be reset beside (or installed behind) that call's render
    if (mode != MODE_RESET_DONE || !s->list_valid) return k;
    if (is_lazy(s->rec.path)) {
        // (a lazy step's render reads the live grid: the classic reset may not rewrite it beside that render)
        if (!s->shadow_ok) return k;
        k.path = RESET_INSTALL;
    } else if (!s->cfg.visible_radius) k.path = RESET_BESIDE_FULL;
    else k.path = s->rec.path == XWB_PATH_EGO_SPAN ? RESET_BESIDE_SPAN : RESET_BESIDE_PER_ENV;
    // Epochs need a publisher that is already in the caller's queue.  The installing list render is its own (it publishes the
    // fused step's epoch itself); the span render's front kernels publish sync[SYNC_SPAN_*] in every step call on epochs; under
    // full observation it is the kernel behind the step kernel, which a fused launch does not have.  The per-env egocentric
    // render hands over through events.
    k.epochs = s->rec.epochs && (k.path == RESET_INSTALL || k.path == RESET_BESIDE_SPAN || (!s->cfg.visible_radius && s->rec.step_pub_queued));
    return k;
}

// What every reset that regenerates live envs does first.
int reset_preamble(xwb_sim *s, int frame_src, hipStream_t st) {
    XWB_TRY(join_regen(s, st));
    s->frame_src = frame_src;
    s->draws_since_pack += 1;
    if (s->shadow_ok) s->shadow_breaks += 1;
    s->shadow_ok = false;                  // the episodes these envs start now are the ones their shadows held
    s->snap_ok = false;                    // ... and the live grids are rewritten without the snapshot
    return XWB_OK;
}

// the done list again from done[] (MODE_RESET_DONE) or from `mask` (MODE_RESET_MASK), into the current list and counter
int rebuild_done_list(xwb_sim *s, int mode, const uint8_t *mask, hipStream_t st) {
    XWB_TRY(join_regen(s, st));
    XwParams p = xw_params(s);
    p.mask = mask;
    HIP_TRY(hipMemsetAsync(p.done_count, 0, sizeof(int32_t), st));
    HIP_TRY(launch_xw_compact(p, mode, st));
    return XWB_OK;
}

// RESET_ON_CALLER: map generator, goal images, frames, one after the other on `st`; the reset kernel clears the codes
int reset_on_caller(xwb_sim *s, int mode, hipStream_t st) {
    XWB_TRY(reset_preamble(s, mode == MODE_RESET_ALL ? PACK_SRC_LIVE : PACK_SRC_LIST, st));
    XwParams p = xw_params(s);
    p.auto_reset = AUTO_RESET_CLEAR;
    XWB_TRY(launch_reset(s, p, mode, p.visible_radius != 0, st));
    if (mode == MODE_RESET_ALL) return launch_render(s, s->t_render, p, RENDER_ALL, st);
    return launch_render(s, s->t_list, p, RENDER_LIST, st);
}

// RESET_BESIDE_FULL, RESET_BESIDE_PER_ENV: the list comes from the step kernel that was just launched on `st` followed by the
// big render; the (latency-bound, two-wavefront) reset kernel runs on the internal queue as soon as the step kernel is done, i.e.
// *beside* that render.  Under full observation render_all may read grid rows of finished envs while they are being
// regenerated; those envs' frames are rewritten in full by the list render below, which waits for both.  The per-env
// egocentric render skips the finished envs (their terminal frames were drawn behind the step kernel: step_plain); there the
// goal images follow the map generator, and the hand-overs are events (choose_reset).
int reset_beside_render(xwb_sim *s, bool epochs, hipStream_t st) {
    XWB_TRY(reset_preamble(s, PACK_SRC_LIST, st));
    XwParams p = xw_params(s);
    // work already queued on `st` may still read this step's codes: the list render, ordered on `st` after that work, clears them
    p.auto_reset = AUTO_RESET_BY_LIST;
    // (epochs: the publisher is the step call's kernel behind the step kernel, already enqueued)
    XWB_TRY(order_after(s, STEP_DONE, epochs, s->epoch_step, s->side));
    XWB_TRY(launch_reset(s, p, MODE_RESET_DONE, p.visible_radius != 0, s->side));
    if (epochs) next_epoch(s->epoch_reset);
    XWB_TRY(publish(s, RESET_DONE, epochs, s->epoch_reset, s->side));
    if (epochs) p.wait_epoch = s->epoch_reset;                       // (the list render waits for it itself)
    else XWB_TRY(order_after(s, RESET_DONE, false, 0, st));
    return launch_render(s, s->t_list, p, RENDER_LIST, st);
}

// RESET_BESIDE_SPAN: the map generator only has to wait for the kernel that reads the grids; the goal images are redrawn by the
// list render's first launch, beside the cell tables, once the step's term gather is through (it shares their buffers).
int reset_beside_span(xwb_sim *s, bool epochs, hipStream_t st) {
    XWB_TRY(reset_preamble(s, PACK_SRC_LIST, st));
    XwParams p = xw_params(s);
    p.auto_reset = AUTO_RESET_BY_LIST;                               // (as reset_beside_render: the gather on `st` clears the codes)
    XWB_TRY(order_after(s, SPAN_CELLS_DONE, epochs, s->epoch_step, s->side));
    XWB_TRY(launch_reset(s, p, MODE_RESET_DONE, false, s->side));
    // the map generator and the front kernels of the new episodes' first frames run on the side queue, beside the big
    // gather (they write nothing the caller reads).  Only the short gather that stores those frames runs on the CALLER's
    // stream: it overwrites the terminal frames, which work queued there before this call may still read (xwb.h xwb_reset_done).
    XWB_TRY(order_after(s, TERM_DONE, epochs, s->epoch_step, s->side));
    HIP_TRY(launch_xw_render(p, RENDER_LIST_FRONT_WARP, s->side));
    if (epochs) next_epoch(s->epoch_reset);
    XWB_TRY(publish(s, RESET_DONE, epochs, s->epoch_reset, s->side));
    XWB_TRY(order_after(s, RESET_DONE, epochs, s->epoch_reset, st));
    return launch_render(s, s->t_list, p, RENDER_LIST_GATHER, st);
}

// RESET_INSTALL: the step kept no terminal snapshot and every env's next episode is pre-generated: the list render installs the
// shadows of the finished envs and draws their first frames (st); the side queue regenerates what was consumed, for nobody in
// particular -- the next holder of the done list waits for it device-side.  The shadows stay valid: no reset_preamble.
int reset_install(xwb_sim *s, bool epochs, hipStream_t st) {
    const bool fused = s->rec.path == XWB_PATH_LAZY_FUSED;
    s->frame_src = PACK_SRC_LIST; s->draws_since_pack += 1;
    XwParams p = xw_params(s);
    p.auto_reset = AUTO_RESET_BY_LIST; p.list_swap = 1;
    // the installs go to the live state AND to the snapshot of it that the next fused step draws from
    if (s->snap_ok) { p.snap_grid_out = s->d_snap_grid[s->snap_sel]; p.snap_act_rep = s->snap_act_rep; }
    // after a fused step this render is the first kernel behind the step in the caller's queue: it publishes that step's epoch
    p.sig_epoch = fused && epochs ? s->epoch_step : 0;
    if (p.sig_epoch) s->rec.step_pub_queued = true;
    // the shadows it installs are the last regeneration pass's: the render waits for its epoch itself, an event is joined here
    if (s->regen_pending && !s->regen_by_epoch) XWB_TRY(join_regen(s, st));
    p.wait_slot = SYNC_REGEN;
    p.wait_epoch = s->regen_pending ? s->epoch_regen : 0;
    XWB_TRY(launch_render(s, s->t_list, p, RENDER_LIST, st));
    // Behind a fused step + render launch the regeneration cannot start before this list render does (it publishes the step's
    // epoch), and nothing needs it before the next step call: it is queued at the top of that call (flush_regen), where it
    // runs beside the render exactly as it would from here -- but a caller that synchronises the device after this verb
    // does not wait 70 us for pre-generated episodes nobody has asked for yet.
    if (fused) { s->regen_deferred = true; return XWB_OK; }
    return launch_regen(s, epochs);
}

// the xworld half of xwb_reset / xwb_reset_done / xwb_reset_masked (and through it xwb_reset_env), the list in place
int run_reset(xwb_sim *s, int mode, hipStream_t st) {
    const ResetPlan k = choose_reset(s, mode);
    s->list_valid = false;
    if (k.path == RESET_ON_CALLER) return reset_on_caller(s, mode, st);
    if (k.path == RESET_BESIDE_SPAN) return reset_beside_span(s, k.epochs, st);
    if (k.path == RESET_INSTALL) return reset_install(s, k.epochs, st);
    return reset_beside_render(s, k.epochs, st);                     // (full observation, or the per-env egocentric render)
}

}  // namespace host
}  // namespace xwb

extern "C" {

int xwb_reset(xwb_sim *s, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    hipStream_t st = as_stream(stream);
    s->autoreset_done = false;
    s->step_open = false;
    if (s->cfg.game != XWB_XWORLD2D) return simple_launch(s, MODE_RESET_ALL, nullptr, nullptr, 1, false, 1, st);
    return run_reset(s, MODE_RESET_ALL, st);
}

int xwb_reset_done(xwb_sim *s, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    hipStream_t st = as_stream(stream);
    s->step_open = false;
    if (s->autoreset_done) {
        // xwb_step_autoreset / xwb_step_n already reset every env whose code is set (the codes are kept for the caller
        // to read): clearing them is all that is left -- resetting those envs again would skip an episode
        s->autoreset_done = false;
        HIP_TRY(hipMemsetAsync(s->d_done, 0, (size_t)s->n, st));
        return XWB_OK;
    }
    if (s->cfg.game != XWB_XWORLD2D) return simple_launch(s, MODE_RESET_DONE, nullptr, nullptr, 1, false, 1, st);
    // no step since the last reset: the list is rebuilt from done[]
    if (!s->list_valid) XWB_TRY(rebuild_done_list(s, MODE_RESET_DONE, nullptr, st));
    return run_reset(s, MODE_RESET_DONE, st);
}

int xwb_reset_masked(xwb_sim *s, const uint8_t *mask_dev, void *stream) {
    if (!s || !mask_dev) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    hipStream_t st = as_stream(stream);
    s->step_open = false;                  // (which envs a mask restarts is the caller's business)
    if (s->cfg.game != XWB_XWORLD2D) return simple_launch(s, MODE_RESET_MASK, mask_dev, nullptr, 1, false, 1, st);
    XWB_TRY(rebuild_done_list(s, MODE_RESET_MASK, mask_dev, st));
    return run_reset(s, MODE_RESET_MASK, st);
}

int xwb_reset_env(xwb_sim *s, int32_t env, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    if (env < 0 || env >= s->n) return fail(XWB_ERR_ARG, "env out of range");
    hipStream_t st = as_stream(stream);
    HIP_TRY(hipMemsetAsync(s->d_mask, 0, (size_t)s->n, st));
    HIP_TRY(hipMemsetAsync(s->d_mask + env, 1, 1, st));
    return xwb_reset_masked(s, s->d_mask, stream);
}

int xwb_step(xwb_sim *s, const int32_t *actions_dev, int32_t act_rep, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    return do_step(s, actions_dev, act_rep, false, as_stream(stream));
}

int xwb_step_host(xwb_sim *s, const int32_t *actions_host, int32_t act_rep, void *stream) {
    if (!s || !actions_host) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    hipStream_t st = as_stream(stream);
    // Pinned (page-locked, device-mapped) host memory: the step kernel reads the ids where they are -- 4 bytes per env over PCIe
    // inside the kernel's first round trip -- instead of behind a copy operation of its own (C4, 131 KB: the copy is ~20 us of
    // a 112 us step, the in-kernel read ~2).  The caller keeps the buffer unchanged until `stream` has passed the call, as for
    // any asynchronous copy from pinned memory.  Pageable memory: staged through the batch's device buffer as before.
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, actions_host) == hipSuccess && attr.type == hipMemoryTypeHost && attr.devicePointer)
        return do_step(s, static_cast<const int32_t *>(attr.devicePointer), act_rep, false, st);
    (void)hipGetLastError();
    HIP_TRY(hipMemcpyAsync(s->d_actions_in, actions_host, sizeof(int32_t) * (size_t)s->n, hipMemcpyHostToDevice, st));
    return do_step(s, s->d_actions_in, act_rep, false, st);
}

int xwb_step_n(xwb_sim *s, int32_t n_steps, int32_t act_rep, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    if (n_steps < 1 || act_rep < 1) return fail(XWB_ERR_ARG, "n_steps and act_rep must be >= 1");
    hipStream_t st = as_stream(stream);
    if (s->cfg.game == XWB_XWORLD2D) {                      // one render per step is the work: nothing to fuse
        // one call = one slot of a results ring, as for the simple games: every step writes it, the last one stays
        const int64_t slot = s->packed_pos;
        for (int i = 0; i < n_steps; ++i) {
            s->packed_pos = slot;
            int rc = do_step(s, nullptr, act_rep, true, st);
            if (rc) return rc;
        }
        return XWB_OK;
    }
    XWB_TRY(simple_launch(s, MODE_STEP, nullptr, nullptr, act_rep, true, n_steps, st));
    s->policy_step += (uint32_t)n_steps;
    s->packed_pos += 1;
    s->autoreset_done = true;
    s->step_open = false;
    return XWB_OK;
}

int xwb_run(xwb_sim *s, int32_t iterations, int32_t act_rep, int32_t flags, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    if (iterations < 1 || act_rep < 1) return fail(XWB_ERR_ARG, "iterations and act_rep must be >= 1");
    if (flags & ~XWB_RUN_AUTORESET) return fail(XWB_ERR_ARG, "unknown flag");
    for (int32_t i = 0; i < iterations; ++i) {
        int rc = (flags & XWB_RUN_AUTORESET) ? xwb_step_autoreset(s, nullptr, act_rep, stream) : xwb_step(s, nullptr, act_rep, stream);
        if (rc == XWB_OK && !(flags & XWB_RUN_AUTORESET)) rc = xwb_reset_done(s, stream);
        if (rc) return rc;
    }
    return XWB_OK;
}

int xwb_step_autoreset(xwb_sim *s, const int32_t *actions_dev, int32_t act_rep, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    return do_step(s, actions_dev, act_rep, true, as_stream(stream));
}

int xwb_check_errors(xwb_sim *s, void *stream, int32_t *n_bad) {
    if (!s || !n_bad) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    hipStream_t st = as_stream(stream);
    HIP_TRY(hipMemcpyAsync(n_bad, s->d_err, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemsetAsync(s->d_err, 0, sizeof(int32_t), st));
    uint32_t timed_out = 0;
    if (s->xw.sync) HIP_TRY(hipMemcpyAsync(&timed_out, s->xw.sync + SYNC_POISON, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (timed_out) s->poisoned = true;                 // sticky: the device word is never cleared
    XWB_LIVE(s);
    return XWB_OK;
}

int xwb_queue_sync_mode(xwb_sim *s, void *stream, int32_t *mode, int32_t *reason) {
    if (!s || !mode) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    const bool e = use_epochs(s, as_stream(stream), true);
    *mode = e ? XWB_QUEUE_SYNC_EPOCHS : XWB_QUEUE_SYNC_EVENTS;
    if (reason) *reason = s->sync_reason;
    return XWB_OK;
}

int xwb_step_path(xwb_sim *s, int32_t *path, int32_t *sync_mode, int32_t *shadow_breaks) {
    if (!s || !path) return fail(XWB_ERR_ARG, "NULL argument");
    *path = s->last_path;
    if (sync_mode) *sync_mode = s->cfg.game == XWB_XWORLD2D ? (s->rec.epochs ? XWB_QUEUE_SYNC_EPOCHS : XWB_QUEUE_SYNC_EVENTS) : XWB_QUEUE_SYNC_AUTO;
    if (shadow_breaks) *shadow_breaks = s->shadow_breaks;
    return XWB_OK;
}

int xwb_queue_sync_forget(xwb_sim *s, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    hipStream_t st = as_stream(stream);
    for (size_t i = 0; i < s->probes.size();)
        if (s->probes[i].st == st) s->probes.erase(s->probes.begin() + (long)i); else ++i;
    return XWB_OK;
}

int xwb_debug_stall_handoff(xwb_sim *s, void *stream, int64_t budget_us) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    if (!s->xw.sync) return fail(XWB_ERR_STATE, "this game has no queue hand-off");
    if (budget_us < 1 || budget_us > 10000000) return fail(XWB_ERR_ARG, "budget_us must be in 1..10 000 000");
    XWB_ON_DEVICE(s);
    // (the probe's slot: its tokens count up from 1, so this value is never reached)
    HIP_TRY(launch_xw_wait(s->xw.sync + SYNC_PROBE, 0x7fffffffu, s->xw.sync + SYNC_POISON, s->xw.poison_host, as_stream(stream), (unsigned long long)budget_us * 100ull));
    return XWB_OK;
}

int xwb_bind_results(xwb_sim *s, float *packed_dev) { return xwb_bind_results_ring(s, packed_dev, 1); }

int xwb_bind_results_ring(xwb_sim *s, float *packed_dev, int64_t slots) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    if (packed_dev && (reinterpret_cast<uintptr_t>(packed_dev) & 7u)) return fail(XWB_ERR_ARG, "results buffer must be 8-byte aligned");
    if (slots < 1) return fail(XWB_ERR_ARG, "slots must be >= 1");
    s->d_packed = reinterpret_cast<float2 *>(packed_dev);
    s->packed_slots = slots;
    s->packed_pos = 0;
    return XWB_OK;
}

// xwb_comm.hip's way in (it only uses the public ABI otherwise): the rows the LAST step call wrote into the results ring, and
// `beside` (the communicator's stream) ordered behind that call's step kernel -- through the step's epoch when it published one
// (nothing is enqueued on the caller's stream then), else through one event recorded on `step_stream`.
extern "C" __attribute__((visibility("hidden"))) int xwb_internal_last_results(xwb_sim *s, void *beside, void *step_stream, const float **rows, int32_t *n) {
    if (!s || !rows || !n) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    if (!s->d_packed) return fail(XWB_ERR_STATE, "no results ring is bound (xwb_bind_results / xwb_bind_results_ring)");
    if (s->packed_pos < 1) return fail(XWB_ERR_STATE, "no step has written the results ring yet");
    *rows = reinterpret_cast<const float *>(s->d_packed + (size_t)((s->packed_pos - 1) % s->packed_slots) * (size_t)s->n);
    *n = s->n;
    // (the egocentric paths publish other slots, or record events; publisher first, waiter second: xw_device.h)
    const bool by_epoch = s->rec.epochs && s->rec.step_pub_queued && !s->cfg.visible_radius;
    const HandOver results{SYNC_STEP, &xwb_sim::ev_results};
    if (!by_epoch) {
        if (!s->ev_results) HIP_TRY(hipEventCreateWithFlags(&s->ev_results, hipEventDisableTiming));
        XWB_TRY(publish(s, results, false, 0, as_stream(step_stream)));
    }
    XWB_TRY(order_after(s, results, by_epoch, s->epoch_step, reinterpret_cast<hipStream_t>(beside)));
    return by_epoch ? 1 : 0;                                    // (>= 0: fine; 1 = nothing was enqueued on the caller's stream)
}

int xwb_bind_obs(xwb_sim *s, void *obs_dev) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    if (obs_dev && (reinterpret_cast<uintptr_t>(obs_dev) & 15u)) return fail(XWB_ERR_ARG, "obs buffer must be 16-byte aligned");
    s->d_obs = obs_dev ? obs_dev : s->d_obs_owned;
    return XWB_OK;
}

int xwb_xw_set_draw(xwb_sim *s, int32_t on) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_STATE, "not an xworld batch (the other games write their observation inside the step kernel)");
    if (s->cfg.visible_radius && !on) return fail(XWB_ERR_STATE, "egocentric frames cannot be drawn elsewhere from the cell codes: they stay on");
    s->draw_off = !on;
    return XWB_OK;
}

int xwb_xw_pack_grids(xwb_sim *s, uint16_t *grids_dev, uint8_t *flags_dev, void *stream) {
    if (!s || !grids_dev) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_STATE, "not an xworld batch");
    if (s->cfg.visible_radius) return fail(XWB_ERR_STATE, "egocentric frames are not a function of the cell codes alone (heading, goal poses, shadows): gather the screens");
    if (s->cfg.context > 1) {
        if (!flags_dev) return fail(XWB_ERR_ARG, "context > 1 needs the ring flags");
        if (s->draws_since_pack != 1)
            return fail(XWB_ERR_STATE, "context > 1: the draw state must be packed after EVERY verb that draws frames (a context ring is "
                                       "replayed one draw at a time); re-synchronise with the screens themselves");
    }
    // (everything a verb leaves behind on the side queue writes the pre-generated episodes, never the live state read here)
    HIP_TRY(launch_xw_pack_grids(xw_params(s), s->frame_src, grids_dev, flags_dev, as_stream(stream)));
    s->draws_since_pack = 0;
    return XWB_OK;
}

int xwb_xw_render_grids(xwb_sim *s, const uint16_t *grids_dev, const uint8_t *flags_dev, int32_t n_envs, void *obs_dev, void *stream) {
    if (!s || !grids_dev || !obs_dev) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_STATE, "not an xworld batch");
    if (s->cfg.visible_radius) return fail(XWB_ERR_STATE, "egocentric batches cannot render from cell codes alone");
    if (n_envs < 1) return fail(XWB_ERR_ARG, "n_envs must be >= 1");
    if (s->cfg.context > 1 && !flags_dev) return fail(XWB_ERR_ARG, "context > 1 needs the ring flags");
    if (reinterpret_cast<uintptr_t>(obs_dev) & 15u) return fail(XWB_ERR_ARG, "obs buffer must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(grids_dev) & 1u) return fail(XWB_ERR_ARG, "grids must be 2-byte aligned");
    XwParams q = xw_params(s);
    q.n = n_envs;
    q.grid = const_cast<uint16_t *>(grids_dev);
    q.fresh = const_cast<uint8_t *>(flags_dev);
    q.obs = static_cast<uint8_t *>(obs_dev);
    q.sig_epoch = 0; q.wait_epoch = 0; q.packed = nullptr; q.no_draw = 0;
    HIP_TRY(launch_xw_render(q, RENDER_ALL, as_stream(stream)));
    return XWB_OK;
}

int xwb_xw_view_dims(const xwb_sim *s, size_t *h, size_t *w, size_t *c) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_ARG, "not an xworld batch");
    const size_t edge = 64u * (size_t)(s->cfg.visible_radius ? s->cfg.visible_radius : s->cfg.max_dim);
    if (h) *h = edge;
    if (w) *w = edge;
    if (c) *c = 3;
    return XWB_OK;
}

int xwb_xw_render_view(xwb_sim *s, const int32_t *envs_dev, int32_t n, void *out_dev, size_t out_bytes, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_ARG, "not an xworld batch");
    if (n < 0) return fail(XWB_ERR_ARG, "n must be >= 0");
    if (!envs_dev && n > s->n) return fail(XWB_ERR_ARG, "n exceeds num_envs (without an index list the views are those of envs 0 .. n - 1)");
    if (n == 0) return XWB_OK;
    size_t edge = 0;
    XWB_TRY(xwb_xw_view_dims(s, &edge, nullptr, nullptr));
    if (!out_dev || out_bytes / (edge * edge * 3) < (size_t)n) return fail(XWB_ERR_ARG, "the output buffer is smaller than n views");
    if (reinterpret_cast<uintptr_t>(out_dev) & 15u) return fail(XWB_ERR_ARG, "the output buffer must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(envs_dev) & 3u) return fail(XWB_ERR_ARG, "the index list must be 4-byte aligned");
    hipStream_t st = as_stream(stream);
    // Ordered on `st` like xwb_xw_pack_grids, and reading what it reads: the live state (or xwb_step's terminal snapshots), never
    // the look-ahead snapshots or the pre-generated episodes, which are all the internal queue writes on the full-observation paths.
    HIP_TRY(launch_xw_view(xw_params(s), s->frame_src, envs_dev, n, s->d_view_atlas, out_dev, st));
    if (s->cfg.visible_radius) {
        // a finished egocentric env awaiting its reset is drawn from the live state (heading, goal images): an xwb_reset_done
        // queued after this call regenerates it on the internal queue, beside whatever still runs on `st` -- not beside this kernel
        HIP_TRY(hipEventRecord(s->ev_view, st));
        HIP_TRY(hipStreamWaitEvent(s->side, s->ev_view, 0));
    }
    return XWB_OK;
}

int xwb_xw_expert_field_dims(const xwb_sim *s, size_t *headings, size_t *cells) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_ARG, "not an xworld batch");
    if (headings) *headings = s->cfg.visible_radius ? 4 : 1;
    if (cells) *cells = (size_t)s->cfg.max_dim * (size_t)s->cfg.max_dim;
    return XWB_OK;
}

int xwb_xw_expert(xwb_sim *s, int32_t *actions_dev, int32_t *dist_dev, uint16_t *field_dev, int32_t no_path_action, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_ARG, "not an xworld batch");
    if (!actions_dev && !dist_dev) return fail(XWB_ERR_ARG, "actions_dev and dist_dev are both NULL");
    const XwParams &xw = s->xw;
    if (xw.group2d && !(xw.n_tasks2 > 0 && !xw.group2d_2))
        return fail(XWB_ERR_ARG, "the batch has no XWorld3DNav* task group: a 2-D-native task succeeds when the agent's cell equals its "
                                 "target, which is a goal's own cell and never entered (XMap::move_item), so it has no winning path");
    if (xw.group2d)
        return fail(XWB_ERR_ARG, "the XWorld3DNav* task group is the batch's SECOND group: the expert follows it in first position only "
                                 "(list it first in the conf / tasks; run second and non-exclusively it never sees a collision)");
    if ((reinterpret_cast<uintptr_t>(actions_dev) | reinterpret_cast<uintptr_t>(dist_dev)) & 3u)
        return fail(XWB_ERR_ARG, "actions_dev and dist_dev must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(field_dev) & 15u) return fail(XWB_ERR_ARG, "field_dev must be 16-byte aligned");
    if (xw.max_dim > XW_MAX_DIM) return fail(XWB_ERR_ARG, "max_dim exceeds the expert's boards");
    // Reads the live state, which only kernels on `stream` write between verbs (the internal queue writes pre-generated episodes
    // and snapshots; where it regenerates envs -- xwb_reset_done, xwb_step_autoreset -- the verb orders `stream` behind it).  An env
    // the last xwb_step finished is answered from its game-over code alone, so a later xwb_reset_done's map generator may run
    // beside this kernel: no event.  That holds because such a reset runs with AUTO_RESET_BY_LIST -- the codes are cleared by the
    // list render on `stream`, behind this kernel, not by the reset kernel on the internal queue; a reset that cleared done[]
    // itself beside the caller's queue would need the event xwb_xw_render_view records.  After xwb_step_autoreset the codes are
    // kept for the caller although the envs have started their next episodes: they are not looked at.
    HIP_TRY(launch_xw_expert(xw_params(s), actions_dev, dist_dev, field_dev, no_path_action, s->autoreset_done, as_stream(stream)));
    return XWB_OK;
}

int xwb_xw_evaluate_plans(xwb_sim *s, const int32_t *envs_dev, int32_t n, const int8_t *plans_dev, int32_t n_plans, int32_t horizon,
                          int32_t act_rep, float gamma, float *return_dev, int32_t *steps_dev, uint8_t *code_dev, int32_t *last_dev,
                          void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_ARG, "not an xworld batch");
    const XwParams &xw = s->xw;
    if (xw.n_tasks2 > 0)
        return fail(XWB_ERR_ARG, "the batch has two task groups: plans are evaluated for ONE XWorld3DNav* group (a second group's stage "
                                 "runs in every step and may draw)");
    if (xw.group2d)
        return fail(XWB_ERR_ARG, "the batch's group holds the 2-D-native tasks: their idle stage draws a task and a target at step "
                                 "time, so a plan's outcome is not a function of its action ids alone");
    if (!plans_dev) return fail(XWB_ERR_ARG, "plans_dev is NULL");
    if (n_plans < 1 || horizon < 1 || act_rep < 1) return fail(XWB_ERR_ARG, "n_plans, horizon and act_rep must be >= 1");
    if (envs_dev && n < 0) return fail(XWB_ERR_ARG, "n must be >= 0");
    if (!return_dev && !steps_dev && !code_dev && !last_dev) return fail(XWB_ERR_ARG, "all four outputs are NULL");
    if (!std::isfinite(gamma)) return fail(XWB_ERR_ARG, "gamma must be finite");
    if ((reinterpret_cast<uintptr_t>(envs_dev) | reinterpret_cast<uintptr_t>(return_dev) | reinterpret_cast<uintptr_t>(steps_dev) |
         reinterpret_cast<uintptr_t>(last_dev)) & 3u)
        return fail(XWB_ERR_ARG, "envs_dev, return_dev, steps_dev and last_dev must be 4-byte aligned");
    if (xw.max_dim > XW_MAX_DIM) return fail(XWB_ERR_ARG, "max_dim exceeds the kernel's grid staging");
    if (!envs_dev) n = s->n;
    if (n == 0) return XWB_OK;
    hipStream_t st = as_stream(stream);
    // Reads the live state the next xwb_step reads, as xwb_xw_expert does (see there: only kernels on `stream` write it between
    // verbs).  One difference: an env the last xwb_step finished reports its node (`last`), i.e. its agent cell and heading are
    // read, and on the classic path a later xwb_reset_done regenerates those on the internal queue.  While such envs exist
    // (step_open) one event orders that queue's LATER work behind this kernel, as xwb_xw_render_view does for egocentric batches.
    HIP_TRY(launch_xw_plans(xw_params(s), envs_dev, n, plans_dev, n_plans, horizon, act_rep, gamma, return_dev, steps_dev, code_dev,
                            last_dev, s->autoreset_done, st));
    if (s->step_open) {
        if (!s->ev_view) HIP_TRY(hipEventCreateWithFlags(&s->ev_view, hipEventDisableTiming | hipEventDisableSystemFence));   // (made on first use)
        HIP_TRY(hipEventRecord(s->ev_view, st));
        HIP_TRY(hipStreamWaitEvent(s->side, s->ev_view, 0));
    }
    return XWB_OK;
}

int xwb_xw_symbolic_dims(const xwb_sim *s, size_t *planes, size_t *rows, size_t *cols) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_ARG, "not an xworld batch");
    const size_t edge = (size_t)(s->cfg.visible_radius ? s->cfg.visible_radius : s->cfg.max_dim);
    if (planes) *planes = XWB_SYM_PLANES;
    if (rows) *rows = edge;
    if (cols) *cols = edge;
    return XWB_OK;
}

int xwb_xw_symbolic(xwb_sim *s, int16_t *out_dev, size_t out_bytes, void *stream) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    if (s->cfg.game != XWB_XWORLD2D) return fail(XWB_ERR_ARG, "not an xworld batch");
    size_t edge = 0;
    XWB_TRY(xwb_xw_symbolic_dims(s, nullptr, &edge, nullptr));
    if (edge > (size_t)XW_MAX_DIM) return fail(XWB_ERR_ARG, "the frame has more squares than the kernel's tables");
    if (!out_dev || out_bytes / (XWB_SYM_PLANES * edge * edge * sizeof(int16_t)) < (size_t)s->n)
        return fail(XWB_ERR_ARG, "the output buffer is smaller than num_envs observations");
    if (reinterpret_cast<uintptr_t>(out_dev) & 1u) return fail(XWB_ERR_ARG, "the output buffer must be 2-byte aligned");
    hipStream_t st = as_stream(stream);
    // The frame xwb_xw_render_view describes, by its rules: ordered on `st`, the selection of xwb_xw_pack_grids under full
    // observation (s->frame_src), the live state in egocentric mode.
    HIP_TRY(launch_xw_symbolic(xw_params(s), s->frame_src, out_dev, st));
    if (s->cfg.visible_radius) {
        // as xwb_xw_render_view: a later xwb_reset_done regenerates finished envs on the internal queue -- not beside this kernel
        HIP_TRY(hipEventRecord(s->ev_view, st));
        HIP_TRY(hipStreamWaitEvent(s->side, s->ev_view, 0));
    }
    return XWB_OK;
}

int xwb_profile_begin(xwb_sim *s) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    s->profiling = true;
    s->t_render.used = s->t_step.used = s->t_reset.used = s->t_list.used = 0;
    return XWB_OK;
}

int xwb_profile_end(xwb_sim *s, void *stream, const char *kernel, double *avg_us, int64_t *launches) {
    if (!s || !kernel || !avg_us || !launches) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    KernelTimer *t = nullptr;
    if (!strcmp(kernel, "render")) t = &s->t_render;
    else if (!strcmp(kernel, "step")) t = &s->t_step;
    else if (!strcmp(kernel, "reset")) t = &s->t_reset;
    else if (!strcmp(kernel, "list")) t = &s->t_list;
    else return fail(XWB_ERR_ARG, "kernel must be render | step | reset | list");
    HIP_TRY(hipStreamSynchronize(as_stream(stream)));
    double total_ms = 0;
    for (size_t i = 0; i < t->used; ++i) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, t->pool[i].a, t->pool[i].b));
        total_ms += ms;
    }
    *launches = (int64_t)t->used;
    *avg_us = t->used ? total_ms * 1000.0 / (double)t->used : 0.0;
    return XWB_OK;
}

int xwb_profile_stop(xwb_sim *s) {
    if (!s) return fail(XWB_ERR_ARG, "sim is NULL");
    s->profiling = false;
    return XWB_OK;
}

}  // extern "C"
