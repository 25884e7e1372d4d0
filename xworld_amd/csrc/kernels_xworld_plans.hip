// kernels_xworld_plans.hip -- xwb_xw_evaluate_plans (include/xwb.h): what the step rule would pay for K action sequences of
// length H per env, read off the env's current state without writing a byte of it.
//
// The rule is xw_step_rule.h's, the one the step kernels run: plan_step below composes its move, goal test, XWorld3DNav* stage,
// reward conversion and game-over code for a batch whose one task group holds XWorld3DNav* tasks.  A plan is a chain of H
// dependent steps of a few dozen integer instructions each, on an LDS grid and ~10 registers: the kernel is bound by that chain
// and by the one memory round trip in front of it, not by bandwidth (it reads n * K * H plan bytes and one grid per env, and
// writes up to 13 bytes per plan).
//
// Shape: one wavefront per workgroup, as the step and expert kernels.  The 64 lanes are cut into slots of L = min(64, K rounded
// up to a power of two) lanes; a slot owns one row i (one env) and its lanes take that row's plans, one each -- 64 / L rows per
// workgroup when K is small.  When K > 64 the plans of a row are spread over gridDim.y workgroups of 64 and, beyond 65 535 of
// those, over passes of a loop.  Round trip 1 fetches everything: the row's env index comes first (one dependent load when an
// index list is given), then the env's scalars -- every lane of a slot loads its env's own, the same addresses, so a slot costs
// one cache line -- and the grids, which the lanes copy into LDS together as aligned dwords.  An env's grid starts on a 2-byte
// boundary only (49 cells at 7 x 7): the copy starts at the dword that holds its first cell and the slot remembers the one-cell
// shift.  The LDS pitch of a slot is odd in dwords, so lanes of different slots that read "their" cell do not share a bank.
// Plan bytes: a lane reads its plan front to back in pieces of 16, 4 or 1 bytes -- the widest that divides H and the buffer's
// alignment --, the next piece requested when the current one is begun.
#include "xwb_common.h"
#include "xw_step_rule.h"

namespace xwb {

namespace {

// Under an XWorld3DNav* group a step draws no random number and moves nothing but the agent, so a plan reads the env's grid as it
// found it, with one exception: the agent's ORIGINAL cell, which is empty once the agent has left it (and which the agent itself
// can re-enter).  Everything a step changes beyond that is a handful of registers (PlanState).
// What a plan reads of its env and never changes; the cells xw_move sees
struct PlanEnv {
    const uint16_t *lg;          // the env's max_dim^2 cell codes (target bits included), as the plan's first step finds them
    int cell0;                   // the agent's cell in lg: reads as empty
    int level;                   // curriculum level (0 without curriculum)
    uint4 gc;                    // the env's goal-slot table (goal_cells)
    __device__ __forceinline__ int code(int cell) const { return cell == cell0 ? 0 : (int)lg[cell]; }
    __device__ __forceinline__ void moved(int, int) const {}
};

// what a step changes
struct PlanState {
    int ax, ay, dir;             // the agent's cell and heading (dir: XwParams::agent_dir; stays 1 under full observation)
    int ts, tsteps, steps;       // task_state, task_steps, num_steps
};

// One xwb_step call for one env: action a (legal: 0 .. 3, 0 .. 5 in egocentric mode) x act_rep.  Updates st; *reward = the float
// the step stores in reward[e]; returns the game-over code it stores in done[e].
__device__ __forceinline__ int plan_step(const StepRule &p, const PlanEnv &v, PlanState &st, int a, int act_rep, float *reward) {
    const Move m = xw_move(p, a, act_rep, st.ax, st.ay, st.dir, v);
    const NavStage s = nav_stage_3d(p, m, m.hit != 0 && hit_is_goal(p, m.hit, m.hit_cell, v.gc), st.ts, st.tsteps, v.level);
    *reward = step_reward(s.rew);
    st.ax = m.ax; st.ay = m.ay; st.dir = m.dir;
    st.ts = pack_task(task_target(st.ts), s.stage, s.event, task_kind(st.ts));
    st.tsteps = s.tsteps;
    st.steps += 1;                                          // GameSimulator::take_actions: once per call
    return done_code(p, st.steps, s.event);
}

struct PlanArgs {
    StepRule rule;
    int n_envs;                  // num_envs of the batch
    int n, n_plans, horizon, act_rep;
    int ignore_done;             // the last verb was xwb_step_autoreset: the envs whose codes are set have been reset already
    float gamma;
    const int32_t *envs;         // nullable: row i is env i
    const int8_t *plans;         // [n][n_plans][horizon]
    // the batch's state, read only
    const uint16_t *grid;
    const int32_t *agent_xy, *task_state, *task_steps, *num_steps;
    const uint8_t *agent_dir, *cur_level, *done, *goal_cells;
    int32_t *err_count;
    // outputs [n][n_plans], each nullable
    float *ret;
    int32_t *steps;
    uint8_t *code;
    int32_t *last;
};

// dwords of LDS one slot's grid takes: the env's cells, one more for a grid that starts in the upper half of a dword; odd
__host__ __device__ inline int plan_pitch_dw(int max_dim) { return ((max_dim * max_dim + 1) / 2 + 1) | 1; }

template <int W> struct PlanPiece;
template <> struct PlanPiece<1> { typedef int8_t T; };
template <> struct PlanPiece<4> { typedef uint32_t T; };
template <> struct PlanPiece<16> { typedef u32x4 T; };        // (a vector, not HIP's uint4 struct: that one ends up in scratch here)
__device__ __forceinline__ int piece_byte(int8_t v, int) { return v; }
__device__ __forceinline__ int piece_byte(uint32_t v, int j) { return (int)(int8_t)(v >> (8 * j)); }
__device__ __forceinline__ int piece_byte(u32x4 v, int j) {
    const uint32_t w = j < 8 ? (j < 4 ? v.x : v.y) : (j < 12 ? v.z : v.w);
    return (int)(int8_t)(w >> (8 * (j & 3)));
}

// W: bytes of a plan read at once (16, 4: horizon is a multiple and the buffer aligned to it)
template <int W>
__global__ __launch_bounds__(64) void xw_plans_kernel(PlanArgs x, int lanes_per_row) {
    typedef typename PlanPiece<W>::T Piece;
    extern __shared__ uint32_t s_grid_dw[];                // [rows of this workgroup][pitch_dw]
    const StepRule &p = x.rule;
    const int lane = threadIdx.x;
    const int L = lanes_per_row, rows = 64 / L;
    const int D = p.max_dim, cells = D * D, pitch = plan_pitch_dw(D);
    const int slot = lane / L, sub = lane - slot * L;
    const long long row0 = (long long)blockIdx.x * rows;
    const long long i = row0 + slot;
    const bool have_row = i < (long long)x.n;

    // round trip 1: the row's env, then everything of that env that does not depend on another load
    int e = -1;
    if (have_row) e = x.envs ? x.envs[i] : (int)i;
    const bool env_ok = have_row && (unsigned)e < (unsigned)x.n_envs;
    PlanState st0{0, 0, 1, 0, 0, 0};
    PlanEnv v{nullptr, 0, 0, make_uint4(~0u, ~0u, ~0u, ~0u)};
    int code_done = 0;
    if (env_ok) {
        const int axy = x.agent_xy[e];
        st0.ax = axy & 0xffff; st0.ay = (axy >> 16) & 0xffff;
        st0.ts = x.task_state[e]; st0.tsteps = x.task_steps[e]; st0.steps = x.num_steps[e];
        if (p.visible_radius) st0.dir = x.agent_dir[e] & 3;
        if (p.curriculum) v.level = x.cur_level[e];
        code_done = x.done[e];
        v.gc = reinterpret_cast<const uint4 *>(x.goal_cells)[e];
    }
    // the rows' grids -> LDS: slot r's env starts at u16 index e * cells of the batch's array; the dwords that hold its cells are
    // copied, the first of them possibly holding one cell of the env before (shift = 1).  Nothing outside the array is read: its
    // last dword may be half a dword, which is then read as one cell.
    const long long total_u16 = (long long)x.n_envs * cells;
    for (int r = 0; r < rows; ++r) {
        const int er = __shfl(e, r * L);                   // (wave-uniform: the slot's first lane holds its env)
        if ((unsigned)er >= (unsigned)x.n_envs) continue;
        const long long first = (long long)er * cells;     // u16 index
        const long long dw0 = first >> 1, dw1 = (first + cells - 1) >> 1;
        const int ndw = (int)(dw1 - dw0) + 1;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(x.grid);
        for (int d = lane; d < ndw; d += 64) {
            const long long g = dw0 + d;
            uint32_t w;
            if (2 * g + 1 < total_u16) w = src[g];
            else w = x.grid[2 * g];
            s_grid_dw[r * pitch + d] = w;
        }
    }
    __syncthreads();
    const int shift = env_ok ? (int)(((long long)e * cells) & 1) : 0;
    v.lg = reinterpret_cast<const uint16_t *>(s_grid_dw + slot * pitch) + shift;
    v.cell0 = st0.ay * D + st0.ax;
    const bool finished = code_done != 0 && !x.ignore_done;     // game over, not reset yet: the expert's rule
    const int NA = p.visible_radius ? 6 : 4;                   // XAgent legal_actions_, xitem.cpp:80-87
    const int H = x.horizon, K = x.n_plans;
    const int heading0 = p.visible_radius ? st0.dir : 0;       // (the expert's field has one plane under full observation)

    if (have_row && !env_ok && sub == 0 && blockIdx.y == 0) atomicAdd(x.err_count, 1);   // once per bad index
    if (!have_row) return;
    for (long long k = (long long)blockIdx.y * L + sub; k < K; k += (long long)gridDim.y * L) {
        const size_t o = (size_t)i * (size_t)K + (size_t)k;
        int n_steps = 0, code = 0, last = -1;
        float ret = 0.0f;
        if (!env_ok) {
            n_steps = -1;
        } else if (finished) {
            code = code_done;
            last = (heading0 << 16) | v.cell0;
        } else {
            PlanState st = st0;
            float g = 1.0f;
            const Piece *src = reinterpret_cast<const Piece *>(x.plans + o * (size_t)H);
            const int pieces = H / W;
            Piece cur = src[0], nxt = cur;
            for (int t = 0; t < H; ++t) {
                const int j = t & (W - 1);
                if (j == 0) {                                          // a new piece; the one after it is requested now
                    cur = nxt;
                    const int c = t / W;
                    nxt = src[c + 1 < pieces ? c + 1 : c];
                }
                const int a = piece_byte(cur, j);
                if ((unsigned)a >= (unsigned)NA) {
                    // XWB_ACTION_SKIP pads a ragged plan; any other id outside the legal range is counted.  Neither is a step.
                    if (a != ACTION_SKIP) atomicAdd(x.err_count, 1);
                    break;
                }
                float r;
                code = plan_step(p, v, st, a, x.act_rep, &r);
                ret = __fadd_rn(ret, __fmul_rn(g, r));                 // ret = ret + g * r_t, two roundings
                g = __fmul_rn(g, x.gamma);
                n_steps += 1;
                if (code != ALIVE) break;
            }
            last = ((p.visible_radius ? st.dir : 0) << 16) | (st.ay * D + st.ax);
        }
        if (x.ret) x.ret[o] = ret;
        if (x.steps) x.steps[o] = n_steps;
        if (x.code) x.code[o] = (uint8_t)code;
        if (x.last) x.last[o] = last;
    }
}

}  // namespace

hipError_t launch_xw_plans(const XwParams &q, const int32_t *envs, int n, const int8_t *plans, int n_plans, int horizon, int act_rep,
                           float gamma, float *ret, int32_t *steps, uint8_t *code, int32_t *last, bool ignore_done, hipStream_t s) {
    PlanArgs x{};
    x.rule = step_rule(q);
    x.n_envs = q.n; x.n = n; x.n_plans = n_plans; x.horizon = horizon; x.act_rep = act_rep;
    x.ignore_done = ignore_done ? 1 : 0;
    x.gamma = gamma;
    x.envs = envs; x.plans = plans;
    x.grid = q.grid; x.agent_xy = q.agent_xy; x.task_state = q.task_state; x.task_steps = q.task_steps; x.num_steps = q.num_steps;
    x.agent_dir = q.agent_dir; x.cur_level = q.cur_level; x.done = q.done; x.goal_cells = q.goal_cells;
    x.err_count = q.err_count;
    x.ret = ret; x.steps = steps; x.code = code; x.last = last;
    int L = 1;
    while (L < 64 && L < n_plans) L <<= 1;
    const int rows = 64 / L;
    const long long gx = ((long long)n + rows - 1) / rows;
    long long gy = L == 64 ? ((long long)n_plans + 63) / 64 : 1;
    if (gy > 65535) gy = 65535;
    if (gx < 1 || gx > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)gy), block(64);
    const size_t lds = (size_t)rows * plan_pitch_dw(q.max_dim) * 4;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(plans);
    if (horizon % 16 == 0 && (addr & 15u) == 0) hipLaunchKernelGGL(xw_plans_kernel<16>, grid, block, lds, s, x, L);
    else if (horizon % 4 == 0 && (addr & 3u) == 0) hipLaunchKernelGGL(xw_plans_kernel<4>, grid, block, lds, s, x, L);
    else hipLaunchKernelGGL(xw_plans_kernel<1>, grid, block, lds, s, x, L);
    return hipGetLastError();
}

}  // namespace xwb
