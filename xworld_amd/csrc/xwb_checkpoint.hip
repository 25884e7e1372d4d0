// xwb_checkpoint.hip -- host side of libxwb.so, part 4: what a batch's state is, and the verbs that move it -- xwb_state_bytes /
// xwb_save_state / xwb_load_state through the host, xwb_copy_envs env by env on the device.
#include "xwb_sim.h"

using namespace xwb;
using namespace xwb::host;

extern "C" {

// ---- checkpoint ----
extern "C++" {
namespace {
struct StateArray { void *ptr; size_t bytes; size_t per_env; };   // per_env: bytes of one env; 0: not an array of per-env state

// What a batch's dynamic state is: xwb_save_state writes these arrays, xwb_copy_envs copies the per-env ones env by env.
// list_sel / count_sel: which buffers of the done list's and its counter's rotation are the state's
std::vector<StateArray> state_arrays(xwb_sim *s, bool include_obs, int list_sel, int count_sel) {
    const size_t n = (size_t)s->n;
    std::vector<StateArray> a;
    auto add = [&](void *p, size_t bytes) { if (p) a.push_back(StateArray{p, bytes, 0}); };
    auto env = [&](void *p, size_t per_env) { if (p) a.push_back(StateArray{p, n * per_env, per_env}); };
    env(s->d_actions, 4); env(s->d_num_steps, 4); env(s->d_episode, 4); env(s->d_reward, 4);
    env(s->d_done, 1); env(s->d_success, 1); add(s->d_err, 4); add(s->d_reset_partial, ((n + 255) / 256) * 4);
    env(s->d_pos, 4); env(s->d_flags, 1);
    env(s->d_x, 4); env(s->d_y, 4); env(s->d_angle, 4);
    env(s->d_minstd, 4);
    if (s->cfg.game == XWB_XWORLD2D) {
        const size_t cells = (size_t)s->cfg.max_dim * s->cfg.max_dim;
        const XwParams &x = s->xw;
        env(x.grid, cells * 2); env(x.agent_xy, 4); env(x.task_steps, 4); env(x.task_state, 4);
        env(x.task_steps2, 4); env(x.task_state2, 4); env(x.grp_order, 1);
        // (the done list and its counter rotate through two / three buffers: the current ones are saved, a load rewinds the rotation)
        add(x.done_list + (size_t)list_sel * n, n * 4); add(x.done_count + count_sel, 4); env(x.fresh, 1); add(x.perf, 40 * 8);
        env(x.goal_cells, XW_MAX_GOALS); env(x.cand2d, 4); env(x.agent_dir, 1); env(x.sent_names, 4);
        env(x.goal_warp, XW_MAX_GOALS * 6 * sizeof(double));            // goal images are re-warped from these on load
        env(x.cur_level, 1); env(x.cur_counter, 4); env(x.cur_usage, 9 * XW_USAGE_BYTES);
    }
    if (include_obs) env(s->d_obs, s->obs_bytes_per_env);
    return a;
}

// version 3 (round 4): per-workgroup reset counts (d_reset_partial, sized by num_envs) replaced the single counter, the
// exclusive schedule's group order and the task performance counters joined, count_sel lost its rc_sel bit
// version 4 (round 6): ONE done counter (the current one of the rotation) instead of the pair
constexpr uint32_t XWB_STATE_VERSION = 4;
struct StateHeader {
    char magic[8];
    uint32_t version, game, num_envs, include_obs, n_arrays, policy_step, count_sel, list_valid;
    uint64_t obs_bytes_per_env, cfg_hash;
};

// The configuration as one number, in two parts that share one walk over the fields: what shapes an env's state (pointers
// excluded), and -- `identity` -- which envs these are: how many, their seeds and global ids, the reference engine's numbering.
// A state blob belongs to both; two batches can exchange envs (xwb_copy_envs) when the first part agrees.
uint64_t config_hash(const xwb_config &c, bool identity = true) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](const void *p, size_t n) { const uint8_t *b = (const uint8_t *)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
    auto mix_id = [&](const void *p, size_t n) { if (identity) mix(p, n); };
    const int32_t v[] = {c.context, c.max_steps, c.array_size, c.track_type, c.race_full_manouver, c.random,
                         c.difficulty_hard, c.map_kind, c.max_dim, c.dim, c.num_goals, c.num_blocks, c.max_steps_factor, c.task_mode,
                         c.n_tasks, c.color, c.visible_radius, c.obs_format, c.n_icons};
    mix(&c.game, 4); mix_id(&c.num_envs, 4);
    mix(v, sizeof v); mix(c.tasks, sizeof c.tasks);
    mix_id(&c.seed, 4); mix_id(&c.policy_seed, 4); mix_id(&c.env_gid0, 4);
    mix(&c.rng_mode, 4); mix_id(&c.simulator_seed, 4); mix_id(&c.thread_base, 4);
    mix(&c.n_tasks2, 4); mix(c.tasks2, sizeof c.tasks2); mix(&c.task_schedule2, 4); mix(c.task_weights2, sizeof c.task_weights2);
    mix(&c.task_groups_exclusive, 4); mix(&c.task_group_weight, 8); mix(&c.task_group_weight2, 8);
    mix(&c.curriculum, 8); mix(&c.start_level, 4); mix(&c.task_schedule, 4); mix(c.task_weights, sizeof c.task_weights); mix(&c.no_wall_shadow, 4);
    return h;
}
}  // namespace
}  // extern "C++"

int xwb_state_bytes(xwb_sim *s, int32_t include_obs, size_t *bytes) {
    if (!s || !bytes) return fail(XWB_ERR_ARG, "NULL argument");
    size_t total = sizeof(StateHeader);
    for (auto &a : state_arrays(s, include_obs != 0, s->list_sel, s->count_sel)) total += 8 + a.bytes;
    *bytes = total;
    return XWB_OK;
}

int xwb_save_state(xwb_sim *s, int32_t include_obs, uint8_t *out_host, size_t cap) {
    if (!s || !out_host) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    size_t need = 0;
    xwb_state_bytes(s, include_obs, &need);
    if (cap < need) return fail(XWB_ERR_ARG, "buffer smaller than xwb_state_bytes");
    HIP_TRY(hipDeviceSynchronize());
    const auto arrays = state_arrays(s, include_obs != 0, s->list_sel, s->count_sel);
    StateHeader h{};
    memcpy(h.magic, "XWBSTATE", 8);
    h.version = XWB_STATE_VERSION; h.game = (uint32_t)s->cfg.game; h.num_envs = (uint32_t)s->n; h.include_obs = include_obs ? 1u : 0u;
    h.n_arrays = (uint32_t)arrays.size(); h.policy_step = s->policy_step; h.count_sel = 0;
    h.list_valid = (s->list_valid ? 1u : 0u) | (s->autoreset_done ? 2u : 0u); h.obs_bytes_per_env = s->obs_bytes_per_env; h.cfg_hash = config_hash(s->cfg);
    uint8_t *w = out_host;
    memcpy(w, &h, sizeof h); w += sizeof h;
    for (auto &a : arrays) {
        const uint64_t b = a.bytes;
        memcpy(w, &b, 8); w += 8;
        HIP_TRY(hipMemcpy(w, a.ptr, a.bytes, hipMemcpyDeviceToHost));
        w += a.bytes;
    }
    return XWB_OK;
}

int xwb_load_state(xwb_sim *s, const uint8_t *in_host, size_t bytes) {
    if (!s || !in_host) return fail(XWB_ERR_ARG, "NULL argument");
    XWB_ON_DEVICE(s);
    XWB_LIVE(s);
    if (bytes < sizeof(StateHeader)) return fail(XWB_ERR_ARG, "not a state blob");
    StateHeader h;
    memcpy(&h, in_host, sizeof h);
    if (memcmp(h.magic, "XWBSTATE", 8) != 0) return fail(XWB_ERR_ARG, "not a state blob");
    if (h.version != XWB_STATE_VERSION)
        return fail(XWB_ERR_ARG, "state blob version " + std::to_string(h.version) + ", this library reads version " + std::to_string(XWB_STATE_VERSION) +
                                 " (the array layout changed: save again with this library)");
    if (h.game != (uint32_t)s->cfg.game || h.num_envs != (uint32_t)s->n || h.obs_bytes_per_env != s->obs_bytes_per_env ||
        h.cfg_hash != config_hash(s->cfg))
        return fail(XWB_ERR_ARG, "state blob was saved from a batch with another configuration");
    // the whole blob is checked before anything changes: a refused load leaves the batch as it was.  The saved list and counter
    // become the first buffers of the rotation.
    const auto arrays = state_arrays(s, h.include_obs != 0, 0, 0);
    if (arrays.size() != h.n_arrays) return fail(XWB_ERR_ARG, "state blob layout mismatch");
    size_t at = sizeof h;
    for (auto &a : arrays) {
        uint64_t b;
        if (bytes - at < 8) return fail(XWB_ERR_ARG, "truncated state blob");
        memcpy(&b, in_host + at, 8); at += 8;
        if (b != a.bytes || b > bytes - at) return fail(XWB_ERR_ARG, "state blob layout mismatch");
        at += b;
    }
    HIP_TRY(hipDeviceSynchronize());
    step_record_invalidate(s);
    s->count_sel = 0; s->list_sel = 0;
    if (s->xw.done_count) HIP_TRY(hipMemset(s->xw.done_count, 0, 3 * sizeof(int32_t)));
    at = sizeof h;
    for (auto &a : arrays) {
        HIP_TRY(hipMemcpy(a.ptr, in_host + at + 8, a.bytes, hipMemcpyHostToDevice));
        at += 8 + a.bytes;
    }
    s->frame_src = PACK_SRC_LIVE; s->draws_since_pack = 0;
    s->policy_step = h.policy_step; s->list_valid = (h.list_valid & 1u) != 0; s->autoreset_done = (h.list_valid & 2u) != 0;
    s->step_open = s->list_valid;
    if (s->cfg.game == XWB_XWORLD2D) {
        XwParams p = xw_params(s);
        if (p.visible_radius) HIP_TRY(launch_xw_warp_goals(p, false, nullptr));
        if (!h.include_obs) {                           // frames from the state; older context frames start black
            HIP_TRY(hipMemset(s->xw.fresh, 2, (size_t)s->n));
            HIP_TRY(launch_xw_render(p, RENDER_ALL, nullptr));
        }
    }
    else if (!h.include_obs) {                          // the simple games: a frame is a function of the restored state
        if (s->cfg.game == XWB_SIMPLE_GAME) HIP_TRY(launch_simple_game_draw(sg_params(s), nullptr));
        else HIP_TRY(launch_simple_race_draw(race_params(s), nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    return XWB_OK;
}

// ---- copy envs ----
extern "C++" {
namespace {
// the arrays a copy moves: every per-env array of the state, the frames and, for egocentric batches, the derived per-env buffers
// -- the warped goal images travel with the poses they were made from, and what the render cached of the destination env's goal
// cells is dropped.  keep_rng: the destination keeps its episode counter and its engine.
int copy_table(xwb_sim *dst, xwb_sim *src, bool keep_rng, CopyEnvsParams &t) {
    const auto da = state_arrays(dst, true, 0, 0), sa = state_arrays(src, true, 0, 0);
    if (da.size() != sa.size()) return fail(XWB_ERR_ARG, "the two batches do not hold the same state arrays");
    uint32_t chunk = 1;                                             // (chunk 0: the small arrays)
    auto put = [&](void *d, const void *s_, size_t per_env) {
        if (per_env > 0xffffffffu / 2) return false;
        CopyArray a{static_cast<const uint8_t *>(s_), static_cast<uint8_t *>(d), (uint32_t)per_env, 0u};
        if (per_env <= (size_t)COPY_SMALL) {
            if (t.n_small == COPY_MAX_SMALL) return false;
            t.small[t.n_small++] = a;
        } else {
            if (t.n_big == COPY_MAX_BIG) return false;
            a.chunk0 = chunk;
            chunk += (uint32_t)((per_env + COPY_CHUNK - 1) / COPY_CHUNK);
            t.big[t.n_big++] = a;
        }
        return true;
    };
    bool ok = true;
    for (size_t i = 0; i < da.size() && ok; ++i) {
        if (da[i].per_env != sa[i].per_env) return fail(XWB_ERR_ARG, "the two batches do not hold the same state arrays");
        if (!da[i].per_env) continue;
        if (keep_rng && (da[i].ptr == dst->d_episode || da[i].ptr == dst->d_minstd)) continue;
        ok = put(da[i].ptr, sa[i].ptr, da[i].per_env);
    }
    const XwParams &dx = dst->xw, &sx = src->xw;
    if (ok && dx.goal_img && sx.goal_img) ok = put(dx.goal_img, sx.goal_img, (size_t)dx.num_goals * 4096 * sizeof(uint32_t));
    if (ok && dx.ego_cache_valid) ok = put(dx.ego_cache_valid, nullptr, (size_t)dx.ego_cache_words * sizeof(uint32_t));
    if (!ok) return fail(XWB_ERR_ARG, "xwb_copy_envs: more per-env arrays than the kernel's table holds");
    t.chunks = (int)chunk;
    return XWB_OK;
}
}  // namespace
}  // extern "C++"

int xwb_copy_envs(xwb_sim *dst, const int32_t *dst_envs_dev, xwb_sim *src, const int32_t *src_envs_dev, int32_t n, int32_t flags,
                  void *stream) {
    if (!dst || !src || !dst_envs_dev || !src_envs_dev) return fail(XWB_ERR_ARG, "NULL argument");
    if (n < 0) return fail(XWB_ERR_ARG, "n must be >= 0");
    if (flags & ~XWB_COPY_KEEP_RNG) return fail(XWB_ERR_ARG, "unknown flag");
    if ((reinterpret_cast<uintptr_t>(dst_envs_dev) | reinterpret_cast<uintptr_t>(src_envs_dev)) & 3u)
        return fail(XWB_ERR_ARG, "the index lists must be 4-byte aligned");
    if (dst->device != src->device) return fail(XWB_ERR_ARG, "the two batches live on different devices");
    const xwb_config &a = dst->cfg, &b = src->cfg;
    if (a.game != b.game || dst->obs_bytes_per_env != src->obs_bytes_per_env || config_hash(a, false) != config_hash(b, false) ||
        a.track_width != b.track_width || a.track_length != b.track_length || a.track_radius != b.track_radius || a.reward_scale != b.reward_scale)
        return fail(XWB_ERR_ARG, "the two batches were created with different configurations (everything but num_envs, the seeds, env_gid0 "
                                 "and thread_base must agree)");
    XWB_ON_DEVICE(dst);
    XWB_LIVE(dst);
    XWB_LIVE(src);
    if (dst->step_open || src->step_open)
        return fail(XWB_ERR_STATE, "between xwb_step and its xwb_reset_done the terminal frames and the done list describe envs a copy would "
                                   "overwrite: reset the finished envs first");
    if (n == 0) return XWB_OK;
    CopyEnvsParams t{};
    XWB_TRY(copy_table(dst, src, (flags & XWB_COPY_KEEP_RNG) != 0, t));
    t.n_pairs = n; t.n_src = src->n; t.n_dst = dst->n; t.same = dst == src ? 1 : 0;
    t.src_envs = src_envs_dev; t.dst_envs = dst_envs_dev; t.err_count = dst->d_err;
    hipStream_t st = as_stream(stream);
    // what a verb that rewrites live envs owes the step paths (xwb_verbs.hip reset_preamble): a regeneration pass still reads the
    // destination's episode counters; its pre-generated episodes and look-ahead snapshot no longer follow from its envs
    XWB_TRY(join_regen(dst, st));
    if (dst->shadow_ok) dst->shadow_breaks += 1;
    dst->shadow_ok = false; dst->snap_ok = false;
    HIP_TRY(launch_copy_envs(t, st));
    // every env of both batches is live, so every frame shows the live grid; a context ring elsewhere cannot follow a copy
    dst->frame_src = PACK_SRC_LIVE; dst->draws_since_pack += 2;
    // codes that xwb_step_autoreset kept for the caller arrive with their envs: the next xwb_reset_done only clears them
    dst->autoreset_done = dst->autoreset_done || src->autoreset_done;
    for (xwb_sim *s : {dst, src}) {
        // egocentric: the internal queue's later work (a map generator beside a render) follows this kernel, as for xwb_xw_render_view
        if (!s->cfg.visible_radius || (s == src && src == dst)) continue;
        HIP_TRY(hipEventRecord(s->ev_view, st));
        HIP_TRY(hipStreamWaitEvent(s->side, s->ev_view, 0));
    }
    return XWB_OK;
}

}  // extern "C"
