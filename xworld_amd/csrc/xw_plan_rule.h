// xw_plan_rule.h -- the XWorld2D step rule as a PURE device function: what xwb_step(actions, act_rep) does to one env whose only
// task group holds XWorld3DNav* tasks, restated over a read-only grid for xwb_xw_evaluate_plans (kernels_xworld_plans.hip).
//
// The step kernels' own statements of the rule write global state and counters and cannot be called from a reader:
//   xw_move        kernels_xworld.hip:196-243   XAgent::act x act_rep, XMap::move_item; headings and turns in egocentric mode
//   xw_teach_store kernels_xworld.hip:245-330   "is the item bumped into a goal" (:253-261), the teacher's reward as a float
//                                               (:319-321), the stores
//   teach_group    kernels_xworld.hip:74-170    the task FSM; restated here: its XWorld3DNav* branch (:120-157)
//   done_code      xw_device.h:134-143          max_steps and, in lang_acquisition only, the task's event
// Whoever changes one of those changes this file with it: tests/test_gpu_plans.py holds the two against each other (forks of a
// batch stepped by the real kernels) and both against the oracle.
//
// Under such a group a step draws no random number and moves nothing but the agent, so a plan reads the env's grid as it found
// it, with one exception: the agent's ORIGINAL cell, which is empty once the agent has left it (and which the agent itself can
// re-enter).  Everything a step changes beyond that is a handful of registers (PlanState).
#pragma once
#include "xw_device.h"

namespace xwb {

// the scalars of XwParams the rule reads (the kernel-argument block of the plans kernel carries these instead of all of XwParams)
struct PlanRule {
    int max_dim, dim, max_steps, max_steps_factor, task_mode, visible_radius, n_icons;
    int curriculum;              // XwParams::curriculum != 0
    const uint8_t *icon_type;    // [n_icons]
};

// what a plan reads of its env and never changes
struct PlanEnv {
    const uint16_t *lg;          // the env's max_dim^2 cell codes (target bits included), as the plan's first step finds them
    int cell0;                   // the agent's cell in lg: reads as empty
    int level;                   // curriculum level (0 without curriculum)
    uint4 gc;                    // the env's goal-slot table (goal_cells)
};

// what a step changes
struct PlanState {
    int ax, ay, dir;             // the agent's cell and heading (dir: XwParams::agent_dir; stays 1 under full observation)
    int ts, tsteps, steps;       // task_state, task_steps, num_steps
};

__device__ __forceinline__ int plan_cell(const PlanEnv &v, int cell) { return cell == v.cell0 ? 0 : (int)v.lg[cell]; }

// One xwb_step call for one env: action a (legal: 0 .. 3, 0 .. 5 in egocentric mode) x act_rep.  Updates st; *reward = the float
// the step stores in reward[e]; returns the game-over code it stores in done[e].
__device__ __forceinline__ int plan_step(const PlanRule &p, const PlanEnv &v, PlanState &st, int a, int act_rep, float *reward) {
    const int D = p.max_dim;
    // ---- xw_move (kernels_xworld.hip:198-243) ----
    int ax = st.ax, ay = st.ay, dir = st.dir;
    int ddx = a == 2 ? -1 : (a == 3 ? 1 : 0);               // MOVE_LEFT / MOVE_RIGHT
    int ddy = a == 0 ? -1 : (a == 1 ? 1 : 0);               // MOVE_UP / MOVE_DOWN
    int vx = 0, vy = 1;                                     // full observation: the heading stays +y
    int hit = 0, hit_cell = 0;
    for (int i = 0; i < act_rep; ++i) {
        if (p.visible_radius) {                             // :210-224: relative to the heading; a turn changes it, every repeat
            if (a == 4) dir = (dir + 3) & 3;
            else if (a == 5) dir = (dir + 1) & 3;
            vx = dir == 0 ? 1 : (dir == 2 ? -1 : 0);
            vy = dir == 1 ? 1 : (dir == 3 ? -1 : 0);
            const int lx = vy, ly = -vx;
            ddx = a == 0 ? vx : (a == 1 ? -vx : (a == 2 ? lx : (a == 3 ? -lx : 0)));
            ddy = a == 0 ? vy : (a == 1 ? -vy : (a == 2 ? ly : (a == 3 ? -ly : 0)));
            if (a >= 4) continue;                           // :227 a turn: no move, no contact
        }
        const int tx = ax + ddx, ty = ay + ddy;
        if (tx >= 0 && ty >= 0 && tx < D && ty < D) {
            const int code = plan_cell(v, ty * D + tx);
            if (code == 0) { ax = tx; ay = ty; }            // :230-235 XMap::move_item: empty cell -> move
            else { hit = code; hit_cell = ty * D + tx; }    // :236-239 contact (kept over the repeats that follow)
        }
    }
    // (last_action_success, the move's other output, feeds the 2-D-native tasks only)
    // ---- xw_teach_store (kernels_xworld.hip:247-330) ----
    const int steps = st.steps + 1;                         // :249 GameSimulator::take_actions: once per call
    bool hit_is_goal = false;                               // :253-261 both forms
    if (hit != 0) {
        if (D > 15) {
            const uint32_t icon = (uint32_t)(hit & CELL_ICON_MASK) - 1u;
            hit_is_goal = icon < (uint32_t)p.n_icons && p.icon_type[icon] == 0;
        } else {
            const uint32_t rep = (uint32_t)hit_cell * 0x01010101u;
            auto has = [&](uint32_t w) { const uint32_t x = w ^ rep; return ((x - 0x01010101u) & ~x & 0x80808080u) != 0u; };
            hit_is_goal = has(v.gc.x) || has(v.gc.y) || has(v.gc.z) || has(v.gc.w);
        }
    }
    // ---- teach_group<0>, XWorld3DNav* branch (kernels_xworld.hip:120-157) ----
    const int target = task_target(st.ts), kind = task_kind(st.ts);
    int stage = task_stage(st.ts), tsteps = st.tsteps, event = EV_NONE;
    double rew = 0.0;
    if (stage == STAGE_NAV) {
        rew = -0.01;                                        // :126 time_penalty
        tsteps += 1;
        const int dim = p.curriculum ? 3 + v.level : p.dim; // :128 env.get_dims()
        if (tsteps >= dim * dim * p.max_steps_factor) {     // :129-133
            event = EV_TIMEUP;
            stage = STAGE_TERMINAL;
        } else if (hit != 0 && ddx == vx && ddy == vy && hit_is_goal) {   // :134-151 _reach_object along the heading
            bool good = kind != TASK_BETWEEN && (hit & CELL_TARGET_BIT);
            if (kind == TASK_DIRECTION && target >= 0) {
                const int rc = target & 0xff, word = (target >> 8) & 7;
                const int v2x = rc % D - hit_cell % D, v2y = rc / D - hit_cell / D;
                const int cs = vx * v2x + vy * v2y, sn = vy * v2x - vx * v2y;
                const int dirw = cs > 0 ? DIR_FRONT : (cs < 0 ? DIR_BEHIND : (sn > 0 ? DIR_RIGHT : DIR_LEFT));
                good = v2x * v2x + v2y * v2y == 1 && dirw == word;
            }
            if (good) { event = EV_CORRECT; rew += 1.0; }
            else { event = EV_WRONG; rew += -1.0; }
            stage = STAGE_TERMINAL;
        } else if (kind == TASK_BETWEEN && ay * D + ax == target) {       // :152-157
            event = EV_CORRECT; rew += 1.0;
            stage = STAGE_TERMINAL;
        }
    }
    // (an idle or terminal stage: reward 0, no event -- :120-124 defers a mid-episode idle stage, which one group never reaches)
    float r = 0.0f;                                         // :319-321 SimulatorInterface::take_actions
    r += 0.0f;
    r = (float)((double)r + rew);
    *reward = r;
    st.ax = ax; st.ay = ay; st.dir = dir;
    st.ts = pack_task(target, stage, event, kind);
    st.tsteps = tsteps;
    st.steps = steps;
    // ---- done_code (xw_device.h:134-143) ----
    int code = (p.max_steps > 0 && steps >= p.max_steps) ? MAX_STEP : ALIVE;
    if (p.task_mode == 0) {
        if (event == EV_CORRECT) code |= SUCCESS;
        else if (event == EV_WRONG) code |= DEAD;
        else if (event == EV_TIMEUP) code |= MAX_STEP;
    }
    return code;
}

}  // namespace xwb
