// xwb_create.hip -- host side of libxwb.so, part 1: configuration, set-up of a batch, xwb_create / xwb_destroy
// (SimulatorInterface::SimulatorInterface, simulator_interface.cpp:37-85).
#include "xwb_sim.h"
#include "../../include/xwb_minstd.h"

using namespace xwb;
using namespace xwb::host;

namespace xwb {
namespace host {
namespace { thread_local std::string g_err; }
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
const char *const POISON_MSG = "a device-side queue hand-off was not released within its watchdog (kernels of the batch's two queues did "
                               "not run concurrently, or the device is wedged): the batch is poisoned -- results since the last "
                               "successful xwb_check_errors are void, destroy it (XWB_QUEUE_SYNC=events / xwb_config.queue_sync avoid epochs)";
}  // namespace host
}  // namespace xwb

namespace {

// XWB_DEBUG (include/xwb.h, xwb_config "Debug configuration"): parsed once per process, OR-ed into every batch created
int32_t debug_env_flags() {
    static const int32_t d = [] {
        int32_t flags = 0;
        const char *v = getenv("XWB_DEBUG");
        if (!v) return flags;
        std::string all(v);
        size_t pos = 0;
        while (pos <= all.size()) {
            size_t end = all.find(',', pos);
            if (end == std::string::npos) end = all.size();
            const std::string t = all.substr(pos, end - pos);
            if (t == "no_pregen") flags |= XWB_DEBUG_NO_PREGEN;
            else if (t == "no_lazy") flags |= XWB_DEBUG_NO_LAZY;
            else if (t == "ego_no_cache") flags |= XWB_DEBUG_EGO_NO_CACHE;
            else if (t == "ego_no_span") flags |= XWB_DEBUG_EGO_NO_SPAN;
            else if (t == "ego_no_flat") flags |= XWB_DEBUG_EGO_NO_FLAT;
            else if (t == "no_fused") flags |= XWB_DEBUG_NO_FUSED;
            else if (!t.empty()) fprintf(stderr, "libxwb: XWB_DEBUG: unknown entry '%s' ignored\n", t.c_str());
            pos = end + 1;
        }
        return flags;
    }();
    return d;
}

// ---- host restatement of the SimpleRace constructors (float/double conversion points matter) ----
void race_setup(const xwb_config &c, RaceParams &r) {
    const double PI = 3.1415926;                       // simple_race_simulator.h:39
    r.track_type = c.track_type;
    r.random = c.random;
    r.difficulty_hard = c.difficulty_hard;
    r.reward_scale = c.reward_scale;
    r.delta_ang = (float)(PI / 10);                    // RaceEngine ctor, cpp:257-261
    r.delta_fwd = 1;
    if (c.race_full_manouver) { r.n_legal = 9; for (int i = 0; i < 9; ++i) r.legal[i] = i; }
    else { r.n_legal = 2; r.legal[0] = 4; r.legal[1] = 7; }         // get_action_set, cpp:432-440
    const float cx = (float)(480 / 2), cy = (float)(720 / 2);       // WINDOW_WIDTH/HEIGHT, cpp:34-35,446
    if (c.track_type == 1) {                           // CircleTrack ctor, cpp:55-59
        float r_in = (float)c.track_radius, width = (float)c.track_width;
        r.center_x = cx; r.center_y = cy;
        r.inner_radius = r_in;
        r.width = width;
        r.outer_radius = r_in + r.width;
        r.length = 0; r.mid_x = r.mid_y = r.start_x = r.start_y = r.end_x = r.end_y = 0;
    } else {                                           // StraightTrack ctor, cpp:105-110
        float length = (float)c.track_length, width = (float)c.track_width;
        r.mid_x = cx; r.mid_y = cy;
        r.length = length;
        r.width = width;
        float d0 = (float)(0.4 * (double)r.length), d1 = (float)(0.6 * (double)r.length);
        r.start_x = r.mid_x - 0.0f; r.start_y = r.mid_y - d0;
        r.end_x = r.mid_x + 0.0f;   r.end_y = r.mid_y + d1;
        r.center_x = r.center_y = r.inner_radius = r.outer_radius = 0;
    }
}

int round_half_even(float v) { return (int)lrintf(v); }          // cvRound

}  // namespace

namespace xwb {

// The 12x12 tile of one icon = what cv::resize(INTER_LINEAR) makes of that icon's cell when the
// 64 px/cell canvas is shrunk to 12 px/cell (xworld_simulator.cpp:521-522).  The ratio is 16/3 in
// both axes for every map size, so output pixel k of a cell takes source pixels s_k, s_k+1 of the
// *same* cell with 11-bit weights; OpenCV 3.2 fixed-point arithmetic (imgwarp.cpp): horizontal pass
// in int32, vertical pass (((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2.  Gray: BGR2GRAY
// (B*1868 + G*9617 + R*4899 + 8192) >> 14 applied to the resized BGR tile (cvtColor after resize).
void build_tile_table(const uint8_t *icons64, int n_icons, int channels, uint8_t *out) {
    int tap[12];
    short w0[12], w1[12];
    const double scale = 1.0 / (12.0 / 64.0);
    for (int k = 0; k < 12; ++k) {
        float f = (float)((k + 0.5) * scale - 0.5);
        int s = (int)floorf(f);
        f -= (float)s;
        tap[k] = s;
        w0[k] = (short)round_half_even((1.f - f) * 2048);
        w1[k] = (short)round_half_even(f * 2048);
    }
    for (int ic = 0; ic < n_icons; ++ic) {
        const uint8_t *src = icons64 + (size_t)ic * 64 * 64 * 3;
        uint8_t bgr[12][12][3];
        for (int py = 0; py < 12; ++py)
            for (int px = 0; px < 12; ++px)
                for (int c = 0; c < 3; ++c) {
                    const uint8_t *r0 = src + (size_t)tap[py] * 64 * 3, *r1 = r0 + 64 * 3;
                    int h0 = r0[tap[px] * 3 + c] * w0[px] + r0[(tap[px] + 1) * 3 + c] * w1[px];
                    int h1 = r1[tap[px] * 3 + c] * w0[px] + r1[(tap[px] + 1) * 3 + c] * w1[px];
                    bgr[py][px][c] = (uint8_t)((((w0[py] * (h0 >> 4)) >> 16) + ((w1[py] * (h1 >> 4)) >> 16) + 2) >> 2);
                }
        uint8_t *dst = out + (size_t)ic * channels * 144;
        for (int py = 0; py < 12; ++py)
            for (int px = 0; px < 12; ++px) {
                if (channels == 3) {
                    for (int c = 0; c < 3; ++c) dst[c * 144 + py * 12 + px] = bgr[py][px][c];
                } else {
                    dst[py * 12 + px] = (uint8_t)((bgr[py][px][0] * 1868 + bgr[py][px][1] * 9617 +
                                                   bgr[py][px][2] * 4899 + (1 << 13)) >> 14);
                }
            }
    }
}

}  // namespace xwb

namespace {

bool curriculum_cfg(const xwb_config &c) { return c.curriculum != 0 && c.map_kind == XWB_MAP_NAV; }   // XWorldWalls never reads the flag
// simulator_interface.cpp:46-48: lang_acquisition runs the groups non-exclusively whatever the flag says
bool exclusive_cfg(const xwb_config &c) { return c.task_groups_exclusive && c.task_mode != XWB_TASKMODE_LANG_ACQ; }
bool group2d_cfg(const int32_t *tasks, int n) { return n > 0 && tasks[0] >= XWB_TASK2D_TARGET; }

// name tables (xworld_env.py:247-255): per type, names -> icon variants (icon order = path order)
struct NameTables {
    int n_names[3] = {0, 0, 0}, off[3] = {0, 0, 0};      // off: start of each type's offsets inside `first`
    std::vector<int16_t> first, variants;
};

int name_tables(const xwb_config &c, NameTables &t) {
    for (int i = 0; i < c.n_icons; ++i) {
        const int ty = c.icon_type[i];
        if (ty < 0 || ty > 2 || c.icon_name[i] < 0) return fail(XWB_ERR_ARG, "xworld: bad icon_type / icon_name");
        if (c.icon_name[i] + 1 > t.n_names[ty]) t.n_names[ty] = c.icon_name[i] + 1;
    }
    if (t.n_names[1] < 1 || t.n_names[2] < 1 || t.n_names[0] < 1)
        return fail(XWB_ERR_ARG, "xworld: palette needs at least one goal, one block and one agent icon");
    if (c.map_kind == XWB_MAP_NAV && c.num_goals > t.n_names[0])
        return fail(XWB_ERR_ARG, "xworld: XWorldNav needs num_goals distinct goal names");
    for (int ty = 0; ty < 3; ++ty) {
        t.off[ty] = (int)t.first.size();
        for (int nm = 0; nm < t.n_names[ty]; ++nm) {
            t.first.push_back((int16_t)t.variants.size());
            int cnt = 0;
            for (int i = 0; i < c.n_icons; ++i)
                if (c.icon_type[i] == ty && c.icon_name[i] == nm) { t.variants.push_back((int16_t)i); cnt++; }
            if (cnt == 0) return fail(XWB_ERR_ARG, "xworld: name ids of a type must be dense");
        }
        t.first.push_back((int16_t)t.variants.size());
    }
    return XWB_OK;
}

// a task group's list (known ids, all of one family) and its schedule: two checks, because xw_check_config's order -- which
// decides what a configuration with two mistakes reports -- has other checks between the first group's two
int check_task_ids(const int32_t *tasks, int n) {
    for (int i = 0; i < n; ++i)
        if (tasks[i] < XWB_TASK_TARGET || tasks[i] > XWB_TASK2D_BETWEEN) return fail(XWB_ERR_ARG, "xworld: unknown task id");
    for (int i = 1; i < n; ++i)
        if ((tasks[i] >= XWB_TASK2D_TARGET) != (tasks[0] >= XWB_TASK2D_TARGET))
            return fail(XWB_ERR_ARG, "xworld: a task group holds XWorld3DNav* tasks or 2-D-native XWorldNav* tasks, not both");
    return XWB_OK;
}
int check_task_schedule(int schedule, const double *weights, int n, const char *unknown) {
    if (schedule != XWB_SCHEDULE_RANDOM && schedule != XWB_SCHEDULE_WEIGHTED) return fail(XWB_ERR_ARG, unknown);
    if (schedule == XWB_SCHEDULE_WEIGHTED)
        for (int i = 0; i < n; ++i)
            if (!(weights[i] > 0)) return fail(XWB_ERR_ARG, "A task must have a positive weight");   // teaching_task.cpp:148
    return XWB_OK;
}

// every check of an XWorld2D configuration, no device call; leaves the name tables it has to build on the way
int xw_check_config(const xwb_config &c, NameTables &names) {
    if (c.max_dim < 1 || c.max_dim > XW_MAX_DIM || c.dim < 1 || c.dim > c.max_dim)
        return fail(XWB_ERR_ARG, "xworld: need 1 <= dim <= max_dim <= 16");
    if (c.num_goals < 1 || c.num_goals > XW_MAX_GOALS) return fail(XWB_ERR_ARG, "xworld: need 1 <= num_goals <= 16");
    if (c.task_schedule == XWB_SCHEDULE_WEIGHTED && c.n_tasks < 1) return fail(XWB_ERR_ARG, "xworld: the weighted schedule needs the task list");
    XWB_TRY(check_task_schedule(c.task_schedule, c.task_weights, c.n_tasks, "xworld: unknown task_schedule"));
    if (curriculum_cfg(c)) {
        // XWorldNav.py:27-30: six levels, dims 3 .. max_h -- the class asserts n_levels == 6, i.e. its 8x8 world
        if (c.max_dim != 8) return fail(XWB_ERR_ARG, "xworld: curriculum != 0 needs XWorldNav's 8x8 world (max_dim 8)");
        if (c.start_level < 0 || c.start_level > 5) return fail(XWB_ERR_ARG, "xworld: start_level must be in 0..5");
    }
    if (c.n_icons < 1 || !c.icons64 || !c.icon_type || !c.icon_name)
        return fail(XWB_ERR_ARG, "xworld: icons64 / icon_type / icon_name are required (the reference loads item_path images)");
    if (c.n_icons > 4000) return fail(XWB_ERR_ARG, "xworld: too many icons");
    if (c.n_tasks < 0 || c.n_tasks > 8) return fail(XWB_ERR_ARG, "xworld: need 0 <= n_tasks <= 8");
    XWB_TRY(check_task_ids(c.tasks, c.n_tasks));
    if (c.n_tasks2 < 0 || c.n_tasks2 > 8) return fail(XWB_ERR_ARG, "xworld: need 0 <= n_tasks2 <= 8");
    if (c.n_tasks2 > 0) {
        if (c.n_tasks < 1) return fail(XWB_ERR_ARG, "xworld: a second task group needs a first one");
        XWB_TRY(check_task_ids(c.tasks2, c.n_tasks2));
        if (group2d_cfg(c.tasks2, c.n_tasks2) == group2d_cfg(c.tasks, c.n_tasks))
            return fail(XWB_ERR_ARG, "xworld: two task groups: one must hold XWorld3DNav* tasks, the other the 2-D-native ones");
        XWB_TRY(check_task_schedule(c.task_schedule2, c.task_weights2, c.n_tasks2, "xworld: unknown task_schedule2"));
    }
    if (!(c.task_group_weight >= 0) || !(c.task_group_weight2 >= 0)) return fail(XWB_ERR_ARG, "xworld: task group weights must be >= 0");
    // goal_cells holds one byte per goal slot with 0xff = "no goal": cell 255 only exists on a 16x16 map.  The step kernel, the
    // expert and the egocentric readers tell the two apart (xwb_common.h, xw_goal_slot_empty); the 2-D-native group's candidate
    // tables do not
    if (c.max_dim > 15 && (group2d_cfg(c.tasks, c.n_tasks) || group2d_cfg(c.tasks2, c.n_tasks2)))
        return fail(XWB_ERR_ARG, "xworld: max_dim 16 is not available with the 2-D-native task group (<= 15)");
    XWB_TRY(name_tables(c, names));
    // free cells / block capacity checks the reference leaves to Python asserts
    if (c.map_kind == XWB_MAP_NAV) {
        int X = c.dim % 2 == 0 ? c.dim - 1 : c.dim;
        int nodes = ((X + 1) / 2) * ((X + 1) / 2);
        int hashes = X * X - nodes - (nodes - 1) + (c.dim % 2 == 0 ? (X / 2) + (c.dim / 2) : 0);
        if (c.num_blocks > hashes) return fail(XWB_ERR_ARG, "xworld: too many blocks for a valid maze");
        int free_cells = c.dim * c.dim - hashes;
        if (c.num_goals + 1 > free_cells) return fail(XWB_ERR_ARG, "xworld: not enough free cells");
        if (nodes > 64) return fail(XWB_ERR_ARG, "xworld: maze node lattice larger than 8x8");
    } else {
        int walls = std::min(c.num_blocks, c.dim) + std::min(std::max(c.num_blocks - c.dim, 0), c.dim - 1);
        if (c.num_goals + 1 + walls > c.dim * c.dim) return fail(XWB_ERR_ARG, "xworld: not enough free cells");
    }
    return XWB_OK;
}

// the scalar parameters: what the kernels need to know of the configuration
void xw_fill_scalars(xwb_sim *s, const NameTables &names) {
    const xwb_config &c = s->cfg;
    XwParams &p = s->xw;
    p.n = s->n; p.context = c.context; p.max_steps = c.max_steps; p.act_rep = 1;
    p.map_kind = c.map_kind; p.max_dim = c.max_dim; p.dim = c.dim;
    // under the curriculum the levels place 2 or 4 goals whatever cfg.num_goals says (XWorldNav.py:27-34): the per-env
    // goal-image cache and every kernel that indexes it use the levels' maximum
    p.num_goals = curriculum_cfg(c) ? 4 : c.num_goals;
    p.num_blocks = c.num_blocks; p.max_steps_factor = c.max_steps_factor; p.task_mode = c.task_mode;
    p.channels = c.color ? 3 : 1; p.n_icons = c.n_icons;
    p.obs_f32 = c.obs_format == XWB_OBS_F32 ? 1 : 0;
    p.curriculum = curriculum_cfg(c) ? c.curriculum : 0.0;
    p.visible_radius = c.visible_radius; p.out_dim = s->out_h; p.no_wall_shadow = c.no_wall_shadow;
    p.n_tasks = c.n_tasks; p.group2d = group2d_cfg(c.tasks, c.n_tasks);
    p.task_weighted = c.task_schedule == XWB_SCHEDULE_WEIGHTED;
    p.n_tasks2 = c.n_tasks2; p.group2d_2 = group2d_cfg(c.tasks2, c.n_tasks2);
    p.task_weighted2 = c.task_schedule2 == XWB_SCHEDULE_WEIGHTED;
    for (int i = 0; i < 8; ++i) {
        p.tasks[i] = i < c.n_tasks ? c.tasks[i] : 0;
        p.tasks2[i] = i < c.n_tasks2 ? c.tasks2[i] : 0;
        p.task_acc[i] = (i ? p.task_acc[i - 1] : 0.0) + (i < c.n_tasks && p.task_weighted ? c.task_weights[i] : 0.0);
        p.task_acc2[i] = (i ? p.task_acc2[i - 1] : 0.0) + (i < c.n_tasks2 && p.task_weighted2 ? c.task_weights2[i] : 0.0);
    }
    p.exclusive = exclusive_cfg(c) ? 1 : 0;
    p.group_weight[0] = c.task_group_weight; p.group_weight[1] = c.task_group_weight2;
    p.policy_seed = c.policy_seed; p.env_gid0 = c.env_gid0; p.seed = c.seed;
    for (int t = 0; t < 3; ++t) { p.n_names[t] = names.n_names[t]; p.name_first_off[t] = names.off[t]; }
    p.name_first_len = (int)names.first.size(); p.name_variants_len = (int)names.variants.size();
    p.wait_slot = SYNC_RESET;
}

// s->xw's copies of the buffers all three games share (xwb_create made them).  obs and packed are not here: the caller can
// move them between calls (xwb_bind_obs, the results ring), so xw_params fills them in per launch.
void xw_bind_shared(xwb_sim *s) {
    XwParams &p = s->xw;
    p.actions_out = s->d_actions; p.num_steps = s->d_num_steps; p.episode = s->d_episode; p.success = s->d_success;
    p.reward = s->d_reward; p.done = s->d_done; p.err_count = s->d_err; p.minstd = s->d_minstd;
}

// the live state, then the pre-generated next episodes and the look-ahead snapshots where the configuration allows them
int xw_alloc_state(xwb_sim *s) {
    const xwb_config &c = s->cfg;
    XwParams &p = s->xw;
    const size_t n = (size_t)s->n, cells = (size_t)c.max_dim * c.max_dim;
    const bool exclusive2 = p.exclusive && c.n_tasks2 > 0;
    XWB_TRY(dev_alloc(s, &p.grid, n * cells));
    XWB_TRY(dev_alloc(s, &p.agent_xy, n));
    XWB_TRY(dev_alloc(s, &p.task_steps, n));
    XWB_TRY(dev_alloc(s, &p.task_state, n));
    if (c.n_tasks2 > 0) {
        XWB_TRY(dev_alloc(s, &p.task_state2, n)); XWB_TRY(dev_alloc(s, &p.task_steps2, n));
    }
    if (exclusive2) {
        XWB_TRY(dev_alloc(s, &p.grp_order, n));
        XWB_TRY(dev_alloc(s, &p.idle_list, n)); XWB_TRY(dev_alloc(s, &p.idle_count, 3));
    }
    XWB_TRY(dev_alloc(s, &p.perf, 40));
    // Pre-generated next episodes: possible where an env's next episode is a pure function of (seed, global id, episode + 1)
    // and the render reads nothing but the grid -- full observation, no curriculum (the level depends on the results so far),
    // no per-env reference engine (its state depends on the draws so far), no exclusive group order carried across resets.
    // (float32 frames stay on the classic paths: their plain whole-batch render variant measured 5-8 % slower than the
    // variants the classic paths use -- 416 vs 385 / 394 us on the C4-sized batch)
    s->pregen = c.visible_radius == 0 && !curriculum_cfg(c) && c.rng_mode != XWB_RNG_MINSTD && !exclusive2 &&
                c.obs_format == XWB_OBS_U8 && !(c.debug_flags & XWB_DEBUG_NO_PREGEN);
    if (s->pregen) {
        XWB_TRY(dev_alloc(s, &p.sh_ep, n));
        XWB_TRY(dev_alloc(s, &p.sh_grid, 2 * n * cells));                      // two slots per env
        XWB_TRY(dev_alloc(s, &p.sh_agent_xy, 2 * n));
        XWB_TRY(dev_alloc(s, &p.sh_task_state, 2 * n)); XWB_TRY(dev_alloc(s, &p.sh_task_state2, 2 * n));
        XWB_TRY(dev_alloc(s, &p.sh_sent_names, 2 * n)); XWB_TRY(dev_alloc(s, &p.sh_cand2d, 2 * n));
        XWB_TRY(dev_alloc(s, &p.sh_goal_cells, 2 * n * XW_MAX_GOALS));
        // the default loop's xwb_step as ONE launch (XwParams::snap_*): frames without a context ring only
        if (c.context == 1 && !(c.debug_flags & XWB_DEBUG_NO_FUSED))
            for (int k = 0; k < 2; ++k) XWB_TRY(dev_alloc(s, &s->d_snap_grid[k], n * cells));
    }
    XWB_TRY(dev_alloc(s, &p.done_list, 2 * n));                                // two lists, three counters: xwb_sim.h count_sel
    XWB_TRY(dev_alloc(s, &p.done_ep, 2 * n));
    XWB_TRY(dev_alloc(s, &p.done_count, 3));
    XWB_TRY(dev_alloc(s, &p.fresh, n));
    XWB_TRY(dev_alloc(s, &p.goal_cells, n * XW_MAX_GOALS, 0xff));
    XWB_TRY(dev_alloc(s, &p.cand2d, n));
    XWB_TRY(dev_alloc(s, &p.sent_names, n, 0xff));
    if (curriculum_cfg(c)) {
        XWB_TRY(dev_alloc(s, &p.cur_level, n, c.start_level));
        XWB_TRY(dev_alloc(s, &p.cur_counter, n)); XWB_TRY(dev_alloc(s, &p.cur_usage, n * 9 * XW_USAGE_BYTES));
    }
    XWB_TRY(dev_alloc(s, &p.term_grid, n * cells)); XWB_TRY(dev_alloc(s, &p.term_flag, n));
    XWB_TRY(dev_alloc(s, &p.agent_dir, n, 1));                                 // heading "down": yaw 1.5707963
    return XWB_OK;
}

// the palette: host copies for the getters, the icon and name tables, the 12-px tile table the full-observation render and the
// egocentric frame's consumers read, and under full observation the 64-px images of xwb_xw_render_view
int xw_upload_palette(xwb_sim *s, const NameTables &names) {
    const xwb_config &c = s->cfg;
    XwParams &p = s->xw;
    const size_t ni = (size_t)c.n_icons;
    s->icon_type_h.assign(c.icon_type, c.icon_type + ni);
    s->icon_name_h.assign(c.icon_name, c.icon_name + ni);
    s->icon_colored_h.assign(ni, 0);
    if (c.icon_colored) s->icon_colored_h.assign(c.icon_colored, c.icon_colored + ni);
    std::vector<uint8_t> types(ni), colored(ni);
    std::vector<int16_t> name_ids(ni);
    for (size_t i = 0; i < ni; ++i) {
        types[i] = (uint8_t)c.icon_type[i]; name_ids[i] = (int16_t)c.icon_name[i]; colored[i] = s->icon_colored_h[i] ? 1 : 0;
    }
    XWB_TRY(dev_upload(s, &p.icon_type, types, (ni + 3) & ~(size_t)3));        // the step kernel stages it dword-wise
    XWB_TRY(dev_upload(s, &p.icon_colored, colored));
    XWB_TRY(dev_upload(s, &p.icon_name, name_ids));
    XWB_TRY(dev_upload(s, &p.name_first, names.first));
    XWB_TRY(dev_upload(s, &p.name_variants, names.variants));
    // tile table: entry 0 = empty cell (canvas fill 255, xmap.cpp:129-132), entry i+1 = icon i
    const size_t tile = (size_t)p.channels * 144;
    s->tile_table.assign(ni * tile, 0);
    build_tile_table(c.icons64, c.n_icons, p.channels, s->tile_table.data());
    std::vector<uint8_t> atlas((ni + 1) * tile, 255);
    memcpy(atlas.data() + tile, s->tile_table.data(), s->tile_table.size());
    if (p.obs_f32) {
        // py_simulator.cpp:262-272: `float scale = 1 / 255.0` then pixel * scale, a float32 product
        std::vector<float> af(atlas.size());
        const float scale = (float)(1 / 255.0);
        for (size_t i = 0; i < atlas.size(); ++i) af[i] = (float)atlas[i] * scale;
        XWB_TRY(dev_upload(s, &p.atlas, af));
    } else {
        XWB_TRY(dev_upload(s, &p.atlas, atlas));
    }
    if (c.visible_radius == 0) {
        // xwb_xw_render_view gathers whole 16-byte pieces from the item images as the view stores them: 3 bytes per pixel
        const size_t cell = 64 * 64 * 3;
        std::vector<uint8_t> a3((ni + 1) * cell, 255);
        memcpy(a3.data() + cell, c.icons64, ni * cell);
        XWB_TRY(dev_upload(s, &s->d_view_atlas, a3));
    }
    return XWB_OK;
}

// the internal queue, the events and sync words of its hand-overs with the caller's queue, the watchdog's poison word
int xw_queue_objects(xwb_sim *s) {
    // (a high-priority side queue was tried: no gain beside the renders, and batches created after another one in the same
    // process then failed their resume tests -- left at the default priority)
    HIP_TRY(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
    for (hipEvent_t *ev : {&s->ev_step, &s->ev_reset, &s->ev_term, &s->ev_cells})
        HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming | hipEventDisableSystemFence));
    XWB_TRY(dev_alloc(s, &s->xw.sync, 16));
    // the watchdog's host-visible word (read at the top of every verb, no sync)
    void *hp = nullptr, *dp = nullptr;
    HIP_TRY(hipHostMalloc(&hp, 64, hipHostMallocMapped));
    memset(hp, 0, 64);
    s->h_poison = static_cast<uint32_t *>(hp);
    HIP_TRY(hipHostGetDevicePointer(&dp, hp, 0));
    s->xw.poison_host = static_cast<uint32_t *>(dp);
    return XWB_OK;
}

// the 64-px images the egocentric render samples: 4 bytes per pixel, one white and one black pixel behind the icons, then
// the turned copies of the agent icons (rot_off: where each agent icon's copies start)
void ego_atlas64(const xwb_config &c, std::vector<uint8_t> &a4, std::vector<uint32_t> &rot_off) {
    const size_t npx = (size_t)c.n_icons * 64 * 64;
    a4.assign((npx + 2) * 4, 0);
    for (size_t i = 0; i < npx; ++i) for (int k = 0; k < 3; ++k) a4[i * 4 + k] = c.icons64[i * 3 + k];
    for (int k = 0; k < 3; ++k) a4[npx * 4 + k] = 255;            // white pixel, then a black one
    // XItem::get_item_image turns the agent's icon by 90 - yaw degrees about (32, 32) with a white border: the three
    // quarter turns are exact integer maps (source index 64 falls outside): heading right, left, up
    rot_off.assign(c.n_icons, 0);
    for (int ic = 0; ic < c.n_icons; ++ic) {
        if (c.icon_type[ic] != XWB_ICON_AGENT) continue;
        rot_off[ic] = (uint32_t)(a4.size() / 4);
        for (int h = 0; h < 3; ++h)
            for (int py = 0; py < 64; ++py)
                for (int px = 0; px < 64; ++px) {
                    const int ix = h == 0 ? 64 - py : (h == 1 ? py : 64 - px), iy = h == 0 ? px : (h == 1 ? 64 - px : 64 - py);
                    const bool in = ix >= 0 && ix < 64 && iy >= 0 && iy < 64;
                    for (int k = 0; k < 3; ++k) a4.push_back(in ? c.icons64[(((size_t)ic * 64 + iy) * 64 + ix) * 3 + k] : 255);
                    a4.push_back(0);
                }
    }
}

// The goal-cell cache of the egocentric render, [env][goal slot][view cell][heading]: ~340 KB per env at r = 3 (11 GB for a
// C4-sized batch; the GPU has 288 GB).  Taken only if it leaves at least half of the free memory to the caller; without it
// (p.ego_cache stays null) every goal cell is evaluated every frame.
int ego_cache_alloc(xwb_sim *s) {
    XwParams &p = s->xw;
    const int r = p.visible_radius;
    size_t entry = xw_ego_cache_entry_bytes(p, s->ego_cell_edge);
    if (p.ego_span && xw_ego_square_entry_bytes(p) > entry) entry = xw_ego_square_entry_bytes(p);   // (the span path's layout)
    const size_t per_env = (size_t)p.num_goals * r * r * 4, words = (per_env + 31) / 32;
    const size_t bytes = (size_t)p.n * per_env * entry;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || bytes >= free_b / 2 || words > 64) return XWB_OK;
    void *q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return XWB_OK; }
    s->allocs.push_back(q);
    p.ego_cache = static_cast<uint8_t *>(q);
    XWB_TRY(dev_alloc(s, &p.ego_cache_valid, (size_t)p.n * words));
    p.ego_cache_entry = (uint32_t)entry; p.ego_cache_words = (uint32_t)words;
    return XWB_OK;
}

// The span path's tables (kernels_xworld_ego_span.hip), where the geometry and the palette allow the path: it reads the cache.
// Leaves p.ego_cellinfo null otherwise.
int ego_span_alloc(xwb_sim *s) {
    const xwb_config &c = s->cfg;
    XwParams &p = s->xw;
    // classes of the images every env shares (everything but goals)
    std::vector<uint8_t> cls((size_t)c.n_icons + 2, 0xff);
    std::vector<uint16_t> cls_icon;
    for (int i = 0; i < c.n_icons + 2; ++i)
        if (i >= c.n_icons || c.icon_type[i] != 0) { cls[i] = (uint8_t)(cls_icon.size() < 255 ? cls_icon.size() : 0); cls_icon.push_back((uint16_t)i); }
    if (!p.ego_span || (c.debug_flags & XWB_DEBUG_EGO_NO_SPAN) || p.n_icons >= 8000 || cls_icon.size() > 16) return XWB_OK;
    p.ego_ncls = (int)cls_icon.size();                                          // (the sizes below depend on it)
    if (xw_ego_square_tab_bytes(p) > ((size_t)1 << 27)) return XWB_OK;          // (its offsets are 23 bits of 16-byte units)
    const size_t rr = (size_t)c.visible_radius * c.visible_radius, n = (size_t)p.n;
    const size_t misses = n * ((size_t)p.num_goals < rr ? (size_t)p.num_goals : rr);
    XWB_TRY(dev_alloc(s, &p.ego_cellinfo, n * rr));
    XWB_TRY(dev_alloc(s, &p.ego_cellsrc, n * rr));
    XWB_TRY(dev_alloc(s, &p.ego_cellsrc_list, n * rr));
    XWB_TRY(dev_alloc(s, &p.ego_miss_list, misses)); XWB_TRY(dev_alloc(s, &p.ego_miss_count_list, 4));
    XWB_TRY(dev_alloc(s, &p.ego_miss, misses)); XWB_TRY(dev_alloc(s, &p.ego_miss_count, 4));
    XWB_TRY(dev_upload(s, &p.ego_cls, cls));
    XWB_TRY(dev_upload(s, &p.ego_cls_icon, cls_icon));
    XWB_TRY(dev_alloc(s, &p.ego_tab3, xw_ego_square_tab_bytes(p) + 16));       // these three: filled by launch_xw_ego_build_squares
    XWB_TRY(dev_alloc(s, &p.ego_xtab, xw_ego_xtab_bytes(p) / sizeof(uint32_t)));
    XWB_TRY(dev_alloc(s, &p.ego_clsimg, (size_t)4 * 16));
    return XWB_OK;
}

// Which squares of the span path's table are one flat colour (empty cells: 255; outside the map / shadow: 0): found by looking
// at the table itself, so the shortcut the gather takes for them (XwParams::ego_flat) cannot change a byte
int ego_flat_scan(xwb_sim *s) {
    const xwb_config &c = s->cfg;
    XwParams &p = s->xw;
    const int r = c.visible_radius, U = ego_square(r).U, UP = ego_square(r).UP, RR = r * r, nc = p.ego_ncls;
    const size_t CBP = (size_t)ego_square(r).plane, PBP = (size_t)RR * CBP, keys = (size_t)4 * nc * nc * nc;
    std::vector<uint8_t> tab(xw_ego_square_tab_bytes(p)), flat(keys * RR, 0);
    HIP_TRY(hipMemcpy(tab.data(), p.ego_tab3, tab.size(), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < keys; ++k)
        for (int f = 0; f < RR; ++f) {
            const uint8_t v0 = tab[k * p.channels * PBP + (size_t)f * CBP];
            bool same = v0 == 0 || v0 == 255;
            for (int chn = 0; chn < p.channels && same; ++chn)
                for (int y = 0; y < U && same; ++y) {
                    const uint8_t *row = tab.data() + (k * p.channels + chn) * PBP + (size_t)f * CBP + (size_t)y * UP;
                    for (int x = 0; x < U; ++x) if (row[x] != v0) { same = false; break; }
                }
            flat[k * RR + f] = same && !(c.debug_flags & XWB_DEBUG_EGO_NO_FLAT) ? (v0 == 255 ? 1 : 2) : 0;
        }
    XWB_TRY(dev_upload(s, &p.ego_flat, flat));
    uint8_t *constline = nullptr;
    XWB_TRY(dev_alloc(s, &constline, 256));
    HIP_TRY(hipMemset(constline, 0xff, 128));
    p.ego_constline = constline;
    return XWB_OK;
}

// the egocentric view: goal poses and images, the 64-px atlas, the tap tables of the geometry, the table of whole frames, then
// the goal-cell cache and the span path where they fit; the tables the device builds itself are built here
int xw_ego_setup(xwb_sim *s) {
    const xwb_config &c = s->cfg;
    XwParams &p = s->xw;
    const size_t n = (size_t)s->n;
    XWB_TRY(dev_alloc(s, &p.goal_warp, n * XW_MAX_GOALS * 6));
    XWB_TRY(dev_alloc(s, &p.goal_img, n * p.num_goals * 4096));
    std::vector<uint8_t> a4;
    std::vector<uint32_t> rot_off;
    ego_atlas64(c, a4, rot_off);
    XWB_TRY(dev_upload(s, &p.atlas64, a4));
    XWB_TRY(dev_upload(s, &p.ego_agent_rot, rot_off));
    EgoTap *taps = nullptr;
    HIP_TRY(xw_ego_tables(c.visible_radius, c.max_dim, s->out_h, &taps, &p.ego_fast, &s->ego_cell_edge, &p.ego_span));
    s->allocs.push_back(taps);
    p.ego_taps = taps;
    HIP_TRY(hipEventCreateWithFlags(&s->ev_view, hipEventDisableTiming | hipEventDisableSystemFence));
    XWB_TRY(dev_alloc(s, &p.ego_tab, xw_ego_tab_bytes(p)));                     // filled by launch_xw_ego_build_tab
    if (p.ego_fast && !(c.debug_flags & XWB_DEBUG_EGO_NO_CACHE)) XWB_TRY(ego_cache_alloc(s));
    if (p.ego_cache) XWB_TRY(ego_span_alloc(s));
    HIP_TRY(launch_xw_ego_build_tab(p, nullptr));
    if (p.ego_cellinfo) HIP_TRY(launch_xw_ego_build_squares(p, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    if (p.ego_cellinfo) XWB_TRY(ego_flat_scan(s));
    return XWB_OK;
}

int xw_setup(xwb_sim *s) {
    NameTables names;
    XWB_TRY(xw_check_config(s->cfg, names));
    xw_fill_scalars(s, names);
    xw_bind_shared(s);
    XWB_TRY(xw_alloc_state(s));
    XWB_TRY(xw_upload_palette(s, names));
    XWB_TRY(xw_queue_objects(s));
    if (s->cfg.visible_radius > 0) XWB_TRY(xw_ego_setup(s));
    return XWB_OK;
}

}  // namespace

// (xwb_comm.hip reports its errors through the same per-thread message)
extern "C" __attribute__((visibility("hidden"))) int xwb_internal_fail(int code, const char *msg) { return fail(code, msg); }

// =============================================================== C ABI =====
extern "C" {

const char *xwb_last_error(void) { return g_err.c_str(); }
const char *xwb_version(void) { return "xwb 0.1 (gfx950)"; }

int xwb_default_config(int32_t game, xwb_config *c) {
    if (!c) return fail(XWB_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof *c);
    c->abi_version = XWB_ABI_VERSION;
    c->game = game;
    c->num_envs = 1;
    c->seed = 0xC0FFEEu;
    c->policy_seed = 0x5EEDu;
    c->context = 1;                 // simulator.cpp:21
    c->max_steps = 0;               // simulator.cpp:22
    c->array_size = 6;              // simple_game_simulator.cpp:19
    c->track_type = 0;              // simple_race_simulator.cpp:17
    c->track_width = 20.0f; c->track_length = 100.0f; c->track_radius = 30.0f;   // :18-20
    c->reward_scale = 1.0;          // :26
    c->map_kind = XWB_MAP_NAV; c->max_dim = 8; c->dim = 8; c->num_goals = 4; c->num_blocks = 16;  // XWorldNav.py:8-13,27-39
    c->max_steps_factor = 10;       // simulator.cpp:23
    c->task_mode = XWB_TASKMODE_LANG_ACQ;   // xworld_simulator.cpp:33-37
    c->color = 0;                   // simulator.cpp:25
    if (game < 0 || game > 2) return fail(XWB_ERR_ARG, "unknown game");
    return XWB_OK;
}

int xwb_create(const xwb_config *cfg, xwb_sim **out) {
    if (!cfg || !out) return fail(XWB_ERR_ARG, "NULL argument");
    if (cfg->abi_version != XWB_ABI_VERSION) return fail(XWB_ERR_ARG, "abi_version mismatch");
    if (cfg->num_envs < 1) return fail(XWB_ERR_ARG, "num_envs must be >= 1");
    if (cfg->context < 1) return fail(XWB_ERR_ARG, "context must be >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(XWB_ERR_HIP, "no HIP device: libxwb.so has no CPU path");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(XWB_ERR_ARG, "bad device ordinal");
    DeviceGuard _device_guard(cfg->device);           // the caller's current device is restored on return
    if (cfg->debug_flags & ~63) return fail(XWB_ERR_ARG, "unknown debug_flags bit");
    xwb_sim *s = new xwb_sim();
    s->cfg = *cfg;
    s->cfg.debug_flags |= debug_env_flags();          // the process-wide override (XWB_DEBUG), see xwb.h
    s->device = cfg->device;
    s->n = cfg->num_envs;
    const int n = s->n;
    int rc = XWB_OK;
    auto bail = [&](int code) { xwb_destroy(s); return code; };
    switch (cfg->game) {
        case XWB_SIMPLE_GAME:
            if (cfg->array_size < 1) return bail(fail(XWB_ERR_ARG, "array_size must be >= 1"));
            s->out_h = 1; s->out_w = cfg->array_size; s->out_c = 1;       // simple_game_simulator.cpp:118-124
            s->obs_bytes_per_env = (size_t)cfg->context * cfg->array_size;
            s->num_actions = 2;
            break;
        case XWB_SIMPLE_RACE:
            if (cfg->track_type != 0 && cfg->track_type != 1) return bail(fail(XWB_ERR_ARG, "track_type must be 0 or 1"));
            s->out_h = 1; s->out_w = 4; s->out_c = 1;                     // simple_race_simulator.cpp:492-501
            s->obs_bytes_per_env = (size_t)cfg->context * 4 * sizeof(float);
            race_setup(*cfg, s->race);
            s->num_actions = s->race.n_legal;
            break;
        case XWB_XWORLD2D:
            s->out_h = cfg->max_dim * 12; s->out_w = cfg->max_dim * 12; s->out_c = cfg->color ? 3 : 1;   // xworld_simulator.cpp:53-61,106-112
            if (cfg->obs_format != XWB_OBS_U8 && cfg->obs_format != XWB_OBS_F32) return bail(fail(XWB_ERR_ARG, "xworld: unknown obs_format"));
            s->num_actions = 4;                                           // xitem.cpp:82-83
            if (cfg->visible_radius < 0) return bail(fail(XWB_ERR_ARG, "xworld: visible_radius must be >= 0"));
            if (cfg->visible_radius > 0) {
                // xworld_simulator.cpp:62-68: clamp to the map, frame edge r * (84 / r); xmap.cpp:277: r must be odd
                if (s->cfg.visible_radius > cfg->max_dim) s->cfg.visible_radius = cfg->max_dim;
                const int r = s->cfg.visible_radius;
                if (r % 2 != 1) return bail(fail(XWB_ERR_ARG, "xworld: visible_radius must be an odd int (xmap.cpp:277)"));
                if (cfg->map_kind != XWB_MAP_NAV)
                    return bail(fail(XWB_ERR_ARG, "xworld: visible_radius > 0 needs a maze map (XWorldNav): without maze "
                                                  "generation the reference's set_property rejects the agent's default yaw "
                                                  "(xworld_env.py:208-210, py_util.py:27-29)"));
                s->out_h = s->out_w = r * (84 / r);
                s->num_actions = 6;                                       // xitem.cpp:84-86
            }
            s->obs_bytes_per_env = (size_t)cfg->context * s->out_c * s->out_h * s->out_w * (cfg->obs_format == XWB_OBS_F32 ? 4 : 1);
            break;
        default:
            return bail(fail(XWB_ERR_ARG, "Unrecognized game type"));     // simulator_interface.cpp:82
    }
    if (cfg->rng_mode != XWB_RNG_PHILOX && cfg->rng_mode != XWB_RNG_MINSTD) return bail(fail(XWB_ERR_ARG, "unknown rng_mode"));
    if (cfg->queue_sync < XWB_QUEUE_SYNC_AUTO || cfg->queue_sync > XWB_QUEUE_SYNC_EPOCHS) return bail(fail(XWB_ERR_ARG, "unknown queue_sync"));
    if (cfg->rng_mode == XWB_RNG_MINSTD) {
        // the reference seeds an engine per thread only when FLAGS_simulator_seed != 0 (simulator_util.cpp:44-52); with 0
        // its engines start from hash(thread id), which nobody can replay
        if (cfg->simulator_seed == 0) return bail(fail(XWB_ERR_ARG, "rng_mode minstd needs simulator_seed != 0"));
        if (cfg->thread_base < 0) return bail(fail(XWB_ERR_ARG, "thread_base must be >= 0"));
        std::vector<uint32_t> st((size_t)n);
        for (int e = 0; e < n; ++e)
            st[(size_t)e] = xwb_minstd_seed_thread(cfg->simulator_seed, cfg->thread_base + (int32_t)(cfg->env_gid0 + (uint32_t)e) + 1);
        if ((rc = dev_upload(s, &s->d_minstd, st))) return bail(rc);
    }
    if ((rc = dev_alloc(s, &s->d_actions, n, 0xff))) return bail(rc);
    if ((rc = dev_alloc(s, &s->d_actions_in, n, 0xff))) return bail(rc);
    if ((rc = dev_alloc(s, &s->d_mask, n))) return bail(rc);
    if ((rc = dev_alloc(s, &s->d_num_steps, n))) return bail(rc);
    if ((rc = dev_alloc(s, &s->d_err, 1))) return bail(rc);
    if ((rc = dev_alloc(s, &s->d_reset_partial, (size_t)(n + 255) / 256))) return bail(rc);
    if ((rc = dev_alloc(s, &s->d_episode, n, 0xff))) return bail(rc);      // first reset -> episode 0
    if ((rc = dev_alloc(s, &s->d_reward, n))) return bail(rc);
    if ((rc = dev_alloc(s, &s->d_done, n))) return bail(rc);
    if ((rc = dev_alloc(s, &s->d_success, n, 1))) return bail(rc);         // last_action_success_(true), simulator.cpp:33-34
    {
        uint8_t *obs = nullptr;
        if ((rc = dev_alloc(s, &obs, (size_t)n * s->obs_bytes_per_env))) return bail(rc);
        s->d_obs = s->d_obs_owned = obs;
    }
    if (cfg->game == XWB_SIMPLE_GAME) {
        if ((rc = dev_alloc(s, &s->d_pos, n))) return bail(rc);
        if ((rc = dev_alloc(s, &s->d_flags, n))) return bail(rc);
    } else if (cfg->game == XWB_SIMPLE_RACE) {
        if ((rc = dev_alloc(s, &s->d_x, n))) return bail(rc);
        if ((rc = dev_alloc(s, &s->d_y, n))) return bail(rc);
        if ((rc = dev_alloc(s, &s->d_angle, n))) return bail(rc);
    } else {
        if ((rc = xw_setup(s))) return bail(rc);
    }
    // the reference constructors leave a reset game behind (SimpleGame ctor cpp:82-85, SimpleRaceGame
    // ctor cpp:457, XWorld ctor xworld.cpp:106); screens_ stays empty until reset_game -> init_screen.
    s->cfg.icons64 = nullptr; s->cfg.icon_type = nullptr; s->cfg.icon_name = nullptr;   // not owned
    s->cfg.icon_colored = nullptr;
    rc = xwb_reset(s, nullptr);
    if (rc) return bail(rc);
    HIP_TRY(hipDeviceSynchronize());
    if (s->xw.sync) {
        // the default stream is probed now (other streams: xwb_queue_sync_mode); the probe also re-selects the internal stream
        // when it shares the caller's hardware queue (side_beside, xwb_verbs.hip).  Forced modes and tools skip the probe in
        // use_epochs: the internal stream is still chosen, unless a tool serialises kernels (nothing would pass).
        int why = 0, reason = 0;
        const bool tool = queue_sync_env(&why) == 0 && why == XWB_SYNC_REASON_TOOL;
        (void)use_epochs(s, nullptr, true);
        const int verdict = s->sync_reason;
        const bool probed = verdict == XWB_SYNC_REASON_PROBE_OK || verdict == XWB_SYNC_REASON_PROBE_FAILED || verdict == XWB_SYNC_REASON_PROBE_ERROR;
        if (!probed && !tool) (void)side_beside(s, nullptr, &reason);
        s->sync_reason = verdict;
    }
    *out = s;
    return XWB_OK;
}

int xwb_destroy(xwb_sim *s) {
    if (!s) return XWB_OK;
    XWB_ON_DEVICE(s);
    for (void *p : s->allocs) (void)hipFree(p);
    if (s->d_sent_tab) (void)hipFree(s->d_sent_tab);
    if (s->h_poison) (void)hipHostFree(s->h_poison);
    if (s->side) (void)hipStreamDestroy(s->side);
    for (hipEvent_t ev : {s->ev_step, s->ev_reset, s->ev_term, s->ev_cells, s->ev_results, s->ev_view})
        if (ev) (void)hipEventDestroy(ev);
    for (KernelTimer *t : {&s->t_render, &s->t_step, &s->t_reset, &s->t_list})
        for (auto &ep : t->pool) { (void)hipEventDestroy(ep.a); (void)hipEventDestroy(ep.b); }
    delete s;
    return XWB_OK;
}

}  // extern "C"
