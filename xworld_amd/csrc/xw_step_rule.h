// xw_step_rule.h -- the XWorld2D step rule, stated once: what xwb_step(actions, act_rep) does to one env, as PURE device functions
// over scalars and small structs.  None of them takes XwParams, writes global memory or touches a counter: the step kernels
// (kernels_xworld.hip) add the stores, the counters and the task groups that draw random numbers; xwb_xw_evaluate_plans
// (kernels_xworld_plans.hip) composes the same pieces over a read-only grid; the expert (kernels_xworld_expert.hip) takes its
// goal test and direction word from here.
//   xw_move        XAgent::act x act_rep (xitem.cpp:89-155), XMap::move_item (xmap.cpp:76-101)
//   hit_is_goal    "the item bumped into is a goal"
//   nav_stage_3d   the navigation stage of the XWorld3DNav* tasks (XWorld3DNavTarget.py:45-60, xworld3d_task.py:451-482)
//   step_reward    SimulatorInterface::take_actions' float
//   done_code      AgentSpecificSimulator::game_over
#pragma once
#include "xw_device.h"

namespace xwb {

// the scalars of XwParams the rule reads
struct StepRule {
    int max_dim, dim, max_steps, max_steps_factor, task_mode, visible_radius, n_icons;
    int curriculum;              // XwParams::curriculum != 0
    const uint8_t *icon_type;    // [n_icons]
};
__host__ __device__ inline StepRule step_rule(const XwParams &q) {
    return StepRule{q.max_dim, q.dim, q.max_steps, q.max_steps_factor, q.task_mode, q.visible_radius, q.n_icons,
                    q.curriculum != 0 ? 1 : 0, q.icon_type};
}

// the cell an action of full observation moves the agent along: MOVE_UP, MOVE_DOWN, MOVE_LEFT, MOVE_RIGHT
__device__ __forceinline__ void action_delta(int a, int &ddx, int &ddy) {
    ddx = a == 2 ? -1 : (a == 3 ? 1 : 0);
    ddy = a == 0 ? -1 : (a == 1 ? 1 : 0);
}

// What a call's move leaves: the agent's cell and heading (dir: XwParams::agent_dir, stays 1 under full observation), the last
// contact (hit = the cell code bumped into, 0: none), the last repeat's delta and heading vector, and last_action_success.
struct Move {
    int ax, ay, dir, hit, hit_cell, ddx, ddy, vx, vy;
    bool success;
};

// XAgent::act x act_rep with XMap::move_item for action a (legal: 0 .. 3, 0 .. 5 in egocentric mode).  `cells` answers
// code(cell) and is told moved(from, to) when the agent changes its cell.
template <typename Cells>
__device__ __forceinline__ Move xw_move(const StepRule &p, int a, int act_rep, int ax, int ay, int dir, Cells &cells) {
    const int D = p.max_dim;
    Move m;
    m.ax = ax; m.ay = ay; m.dir = dir;
    action_delta(a, m.ddx, m.ddy);
    m.vx = 0; m.vy = 1;                                  // heading: entities keep yaw 1.5707963 (+y) under full observation
    m.hit = 0; m.hit_cell = 0;
    m.success = false;
    // egocentric: cells along the heading and to its left (MOVE_FORWARD, MOVE_BACKWARD, MOVE_LEFT_FPV, MOVE_RIGHT_FPV; a turn: none).
    // Products instead of a chain of selects: the compiler turns such a chain into divergent branches inside the repeat loop
    const int along = a == 0 ? 1 : (a == 1 ? -1 : 0), left = a == 2 ? 1 : (a == 3 ? -1 : 0);
    for (int i = 0; i < act_rep; ++i) {
        if (p.visible_radius) {
            // xitem.cpp:103-155: MOVE_FORWARD, MOVE_BACKWARD, MOVE_LEFT_FPV, MOVE_RIGHT_FPV relative to the heading; TURN_LEFT /
            // TURN_RIGHT change the yaw, on every repeat, and "move" onto the agent's own cell, which XMap::move_item refuses: a
            // turn is an unsuccessful action without contacts (the contact of an earlier repeat is kept)
            if (a == 4) m.dir = (m.dir + 3) & 3;
            else if (a == 5) m.dir = (m.dir + 1) & 3;
            m.vx = m.dir == 0 ? 1 : (m.dir == 2 ? -1 : 0);
            m.vy = m.dir == 1 ? 1 : (m.dir == 3 ? -1 : 0);
            m.ddx = along * m.vx + left * m.vy;         // left of the heading (vx, vy) is (vy, -vx): right->up, down->right,
            m.ddy = along * m.vy - left * m.vx;         // left->down, up->left
        }
        const int tx = m.ax + m.ddx, ty = m.ay + m.ddy;
        m.success = false;
        if (p.visible_radius && a >= 4) continue;       // a turn
        if (tx >= 0 && ty >= 0 && tx < D && ty < D) {
            const int to = ty * D + tx, code = cells.code(to);
            if (code == 0) {                             // XMap::move_item: empty cell -> move
                cells.moved(m.ay * D + m.ax, to);
                m.ax = tx; m.ay = ty;
                m.success = true;
            } else {
                m.hit = code;                            // contact_list -> "collision:<id>" event
                m.hit_cell = to;
            }
        }
    }
    return m;
}

// The built-in policy's look-ahead: the same move on the cell codes `lg` under full observation, contacts ignored (blocked once =
// blocked for good).  Returns the agent's new cell; *from = its old one (equal: no move).
__device__ __forceinline__ int xw_predict_move(const uint16_t *lg, int D, int axy, int a, int act_rep, int *from) {
    int ax = axy & 0xffff, ay = axy >> 16, ddx, ddy;
    *from = ay * D + ax;
    action_delta(a, ddx, ddy);
    for (int i = 0; i < act_rep; ++i) {
        const int tx = ax + ddx, ty = ay + ddy;
        if (tx < 0 || ty < 0 || tx >= D || ty >= D || lg[ty * D + tx] != 0) break;
        ax = tx; ay = ty;
    }
    return ay * D + ax;
}

// "The item with cell code `code` (not 0) on `cell` is a goal": the cell is in the env's goal-slot table gc (goal_cells; 0xff = no
// goal -- cell 255 exists on a 16 x 16 map only, where the icon's type is looked up instead).
__device__ __forceinline__ bool hit_is_goal(const StepRule &p, int code, int cell, const uint4 &gc) {
    if (p.max_dim > 15) {
        const uint32_t icon = (uint32_t)(code & CELL_ICON_MASK) - 1u;
        return icon < (uint32_t)p.n_icons && p.icon_type[icon] == 0;
    }
    const uint32_t rep = (uint32_t)cell * 0x01010101u;    // a zero byte in w ^ rep = a slot that holds the cell
    auto has = [&](uint32_t w) { const uint32_t x = w ^ rep; return ((x - 0x01010101u) & ~x & 0x80808080u) != 0u; };
    return has(gc.x) || has(gc.y) || has(gc.z) || has(gc.w);
}

// NavTargetDirection's word for an offset (v2x, v2y) seen along the heading (vx, vy): direction(g, referent, yaw)
__device__ __forceinline__ int direction_word(int vx, int vy, int v2x, int v2y) {
    const int cs = vx * v2x + vy * v2y, sn = vy * v2x - vx * v2y;
    return cs > 0 ? DIR_FRONT : (cs < 0 ? DIR_BEHIND : (sn > 0 ? DIR_RIGHT : DIR_LEFT));
}

// What one teach() call makes of an XWorld3DNav* task: the reward it adds to the teacher buffer, the event it leaves there, the
// task's stage and task_steps, and what the step adds to the task's tallies (record: -1 nothing, 0 failure, 1 success; timeup).
struct NavStage {
    double rew;
    int event, stage, tsteps, record;
    bool timeup;
};
// ts / tsteps: the task's state word and task_steps; is_goal: hit_is_goal of m's contact; level: the curriculum level.  Any stage
// but STAGE_NAV: reward 0, no event, nothing changes.
__device__ __forceinline__ NavStage nav_stage_3d(const StepRule &p, const Move &m, bool is_goal, int ts, int tsteps, int level) {
    const int D = p.max_dim, target = task_target(ts), kind = task_kind(ts);
    NavStage s{0.0, EV_NONE, task_stage(ts), tsteps, -1, false};
    if (s.stage != STAGE_NAV) return s;
    s.rew = -0.01;                                      // time_penalty
    s.tsteps += 1;
    const int dim = p.curriculum ? 3 + level : p.dim;   // env.get_dims()
    if (s.tsteps >= dim * dim * p.max_steps_factor) {
        s.event = EV_TIMEUP;
        s.record = 0;
        s.timeup = true;
        s.stage = STAGE_TERMINAL;
    } else if (m.hit != 0 && m.ddx == m.vx && m.ddy == m.vy && is_goal) {
        // _reach_object: id in collisions and |theta| < pi/4, i.e. the goal was bumped into along the heading: MOVE_DOWN under
        // full observation, MOVE_FORWARD in egocentric mode.  Target / Near / Avoid: the reached goal is in self.target (cell bit
        // 15, set by the idle stage) -> correct, else wrong.  Between: any reached goal is wrong.  Direction: the referent is one
        // cell from the goal and (direction(g, referent, agent.yaw), near) holds for the current heading.
        bool good = kind != TASK_BETWEEN && (m.hit & CELL_TARGET_BIT);
        if (kind == TASK_DIRECTION && target >= 0) {    // (a replayed map may carry the bits only)
            const int rc = target & 0xff, word = (target >> 8) & 7;
            const int v2x = rc % D - m.hit_cell % D, v2y = rc / D - m.hit_cell / D;
            good = v2x * v2x + v2y * v2y == 1 && direction_word(m.vx, m.vy, v2x, v2y) == word;
        }
        if (good) { s.event = EV_CORRECT; s.rew += 1.0; }
        else { s.event = EV_WRONG; s.rew += -1.0; }
        s.record = good ? 1 : 0;                        // _successful_goal / _failed_goal
        s.stage = STAGE_TERMINAL;
    } else if (kind == TASK_BETWEEN && m.ay * D + m.ax == target) {
        // XWorld3DNavTargetBetween.navigation_reward: dist(agent, middle) < threshold / 2
        s.event = EV_CORRECT; s.rew += 1.0;
        s.record = 1;
        s.stage = STAGE_TERMINAL;
    }
    return s;
}

// the float a step stores in reward[e] for the teacher's (double) reward
__device__ __forceinline__ float step_reward(double rew) {
    float r = 0.0f;                                     // SimulatorInterface::take_actions
    r += 0.0f;                                          // XWorldSimulator::take_action returns 0
    r = (float)((double)r + rew);                       // r += teacher_->give_reward() (double)
    return r;
}

// AgentSpecificSimulator::game_over = GameSimulator::game_over | XWorldSimulator::game_over
__device__ __forceinline__ int done_code(const StepRule &p, int num_steps, int event) {
    int code = (p.max_steps > 0 && num_steps >= p.max_steps) ? MAX_STEP : ALIVE;
    if (p.task_mode == 0) {       // lang_acquisition, xworld_simulator.cpp:166-177
        if (event == EV_CORRECT) code |= SUCCESS;
        else if (event == EV_WRONG) code |= DEAD;
        else if (event == EV_TIMEUP) code |= MAX_STEP;
    }
    return code;
}

}  // namespace xwb
