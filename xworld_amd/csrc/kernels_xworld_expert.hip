// kernels_xworld_expert.hip -- the shortest-path expert of an XWorld2D batch (xwb_xw_expert, include/xwb.h): for every env
// the fewest xwb_step calls (act_rep 1) after which its XWorld3DNav* task group records "correct_goal", the first action of
// such a sequence, and on request the same number for every cell and heading the agent could stand on.
//
// "Success" is what nav_stage_3d (xw_step_rule.h) rewards, read off the code, not re-derived; "is a goal" and the direction word
// are that header's hit_is_goal and direction_word:
//   Target / Near / Avoid   a move along the heading into a goal whose cell code carries the target bit
//   Direction               ... into a goal one cell from the referent, the direction word holding for the heading of the bump
//                           (target < 0, a replayed map: the target-bit rule)
//   Between                 the call ends with the agent on the middle cell and without a goal bumped along the heading: a move
//                           onto it, or ANY action that leaves the agent standing on it (a turn, a blocked move)
// A goal bumped along the heading that is not a winning one ends the episode ("wrong_goal"): such a bump is no edge of the graph.
// Everything else either moves the agent one cell (the cell is inside the map and empty) or leaves the node unchanged.
//
// Algorithm: one backward, multi-source, level-synchronous search per env.  A board is a bit set -- ONE 64-bit word when
// max_dim <= 8 (rows 8 bits apart), four when it is larger (rows 16 bits apart) -- so "every cell from which one move
// reaches the set" is four shifts, three ORs and an AND with the free cells; the egocentric graph has four such boards, one
// per heading, and a turn is an OR with the two neighbouring headings' boards.  Level 1 is the set of nodes that win at
// once; level k + 1 = predecessors of level k that have not been reached.  The level at which the agent's own node turns up is
// `dist`; the lowest action id whose successor lies in the level before it is `action`.
// A LANE owns an env (64 envs per wavefront, one wavefront per workgroup, like xw_step_kernel): the whole search of a 7 x 7
// egocentric env is 4 boards x 3 sets = 12 words in registers and ~40 bit operations per level, no LDS traffic and no
// cross-lane step inside the loop; a wavefront per env would spend a barrier-separated LDS round trip per level on 49 cells.
// The grids reach the lanes as in the step kernel: the wavefront's 64 grids are one contiguous block, read with 16-byte loads
// into LDS (padded to an odd dword pitch where the pitch would put every lane on one bank), then each lane scans its own.
// The field leaves as 2-byte stores, one per reached node, over a 0xFFFF fill the wavefront stores first with 16-byte stores.
// Every loop is bounded: the scan by max_dim^2, the search by headings * max_dim^2 levels, a level's stores by 64 per word.
#include "xwb_common.h"
#include "xw_step_rule.h"

namespace xwb {

namespace {

typedef unsigned long long u64;

// W words of 64 cells; bit (y << SH) + x
template <int W> struct Board {
    u64 w[W];
    static constexpr int SH = W == 1 ? 3 : 4, S = 1 << SH, RPW = 64 >> SH;
    static constexpr u64 COL0 = W == 1 ? 0x0101010101010101ull : 0x0001000100010001ull;
    static constexpr u64 COLN = COL0 << (S - 1);
};

#define XE_EACH for (int i = 0; i < W; ++i)

template <int W> __device__ __forceinline__ Board<W> b_zero() { Board<W> r; _Pragma("unroll") XE_EACH r.w[i] = 0; return r; }
template <int W> __device__ __forceinline__ Board<W> b_or(Board<W> a, Board<W> b) { _Pragma("unroll") XE_EACH a.w[i] |= b.w[i]; return a; }
template <int W> __device__ __forceinline__ Board<W> b_and(Board<W> a, Board<W> b) { _Pragma("unroll") XE_EACH a.w[i] &= b.w[i]; return a; }
template <int W> __device__ __forceinline__ Board<W> b_andn(Board<W> a, Board<W> b) { _Pragma("unroll") XE_EACH a.w[i] &= ~b.w[i]; return a; }
template <int W> __device__ __forceinline__ bool b_any(Board<W> a) { u64 r = 0; _Pragma("unroll") XE_EACH r |= a.w[i]; return r != 0; }
template <int W> __device__ __forceinline__ bool b_test(Board<W> a, int idx) {
    u64 v = 0;
    _Pragma("unroll") XE_EACH v |= a.w[i] & (0ull - (u64)((idx >> 6) == i));
    return (v >> (idx & 63)) & 1ull;
}
template <int W> __device__ __forceinline__ Board<W> b_bit(int idx) {
    Board<W> r;
    _Pragma("unroll") XE_EACH r.w[i] = (idx >> 6) == i ? 1ull << (idx & 63) : 0ull;
    return r;
}
// the set moved one cell along (dx, dy); what leaves the 8- or 16-column board is dropped (the map's own edge is the caller's mask)
template <int W> __device__ __forceinline__ Board<W> b_xp(Board<W> a) { _Pragma("unroll") XE_EACH a.w[i] = (a.w[i] << 1) & ~Board<W>::COL0; return a; }
template <int W> __device__ __forceinline__ Board<W> b_xm(Board<W> a) { _Pragma("unroll") XE_EACH a.w[i] = (a.w[i] >> 1) & ~Board<W>::COLN; return a; }
template <int W> __device__ __forceinline__ Board<W> b_yp(Board<W> a) {
    constexpr int S = Board<W>::S;
    Board<W> r;
    _Pragma("unroll") XE_EACH r.w[i] = (a.w[i] << S) | (i > 0 ? a.w[i > 0 ? i - 1 : 0] >> (64 - S) : 0ull);
    return r;
}
template <int W> __device__ __forceinline__ Board<W> b_ym(Board<W> a) {
    constexpr int S = Board<W>::S;
    Board<W> r;
    _Pragma("unroll") XE_EACH r.w[i] = (a.w[i] >> S) | (i + 1 < W ? a.w[i + 1 < W ? i + 1 : 0] << (64 - S) : 0ull);
    return r;
}
// heading / direction d: 0 +x, 1 +y, 2 -x, 3 -y (XwParams::agent_dir)
template <int W> __device__ __forceinline__ Board<W> b_shift(Board<W> a, int d) {
    return d == 0 ? b_xp(a) : (d == 1 ? b_yp(a) : (d == 2 ? b_xm(a) : b_ym(a)));
}
template <int W> __device__ __forceinline__ Board<W> b_around(Board<W> a) { return b_or(b_or(b_xp(a), b_xm(a)), b_or(b_yp(a), b_ym(a))); }
// a[h] for a per-lane h, as masks: a select chain over the array is turned into an indexed load, which puts the boards in scratch
template <int W> __device__ __forceinline__ Board<W> b_pick(const Board<W> (&a)[4], int h) {
    Board<W> r = b_zero<W>();
    _Pragma("unroll") for (int k = 0; k < 4; ++k) {
        const u64 m = 0ull - (u64)(h == k);
        _Pragma("unroll") XE_EACH r.w[i] |= a[k].w[i] & m;
    }
    return r;
}
template <int W> __device__ __forceinline__ Board<W> b_pick(const Board<W> (&a)[1], int) { return a[0]; }

__device__ __forceinline__ int dir_dx(int d) { return d == 0 ? 1 : (d == 2 ? -1 : 0); }
__device__ __forceinline__ int dir_dy(int d) { return d == 1 ? 1 : (d == 3 ? -1 : 0); }

// the direction an action moves the agent along, -1: a turn.  Full observation: MOVE_UP, MOVE_DOWN, MOVE_LEFT, MOVE_RIGHT;
// egocentric: forward, backward, left, right of the heading (xw_move: left of +x is -y)
template <bool EGO> __device__ __forceinline__ int action_dir(int a, int heading) {
    if (!EGO) return a == 0 ? 3 : (a == 1 ? 1 : (a == 2 ? 2 : 0));
    return a == 0 ? heading : (a == 1 ? (heading + 2) & 3 : (a == 2 ? (heading + 3) & 3 : (a == 3 ? (heading + 1) & 3 : -1)));
}

struct ExpertArgs {
    int32_t *actions;            // nullable
    int32_t *dist;               // nullable
    uint16_t *field;             // nullable: [n][headings][max_dim^2]
    int no_path_action;
    int ignore_done;             // the last verb was xwb_step_autoreset: the envs whose codes are set have been reset already
};

template <int W, bool EGO>
__global__ __launch_bounds__(64) void xw_expert_kernel(XwParams p, ExpertArgs x) {
    typedef Board<W> B;
    constexpr int H = EGO ? 4 : 1, SH = B::SH, S = B::S, RPW = B::RPW;
    extern __shared__ uint4 s_dyn[];
    uint16_t *s_grid = reinterpret_cast<uint16_t *>(s_dyn);
    uint32_t *s_dw = reinterpret_cast<uint32_t *>(s_dyn);
    const int lane = threadIdx.x, e0 = blockIdx.x * 64, e = e0 + lane;
    const int D = p.max_dim, cells = D * D;
    const int n_here = p.n - e0 < 64 ? p.n - e0 : 64;
    const bool live = lane < n_here;

    // round trip 1: everything that does not depend on another load
    int axy = 0, ts = 0, dir0 = 1, code_done = 0;
    uint4 gc = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (live) {
        axy = p.agent_xy[e];
        ts = p.task_state[e];                                           // the XWorld3DNav* group is the batch's first (the verb refuses others)
        code_done = p.done[e];
        if (EGO) dir0 = p.agent_dir[e] & 3;
        gc = reinterpret_cast<const uint4 *>(p.goal_cells)[e];
    }
    // the wavefront's grids -> LDS.  Pitch: max_dim^2 cells, two more where max_dim % 4 == 0 (a pitch of 8, 32, 72 or 128 dwords
    // would put the 64 lanes' reads on one or two banks).  max_dim 6, 10, 14 keep an even pitch of 18 / 50 / 98 dwords: pairs of
    // lanes share a bank during the scan there -- a cost in time only, not measured.
    const bool pad = (D & 3) == 0;
    const int pitch = cells + (pad ? 2 : 0);
    {
        const uint16_t *src = p.grid + (size_t)e0 * cells;
        const int total = n_here * cells;
        if (!pad) {
            const int full = total / 8;
            for (int c = lane; c < full; c += 64) s_dyn[c] = reinterpret_cast<const uint4 *>(src)[c];
            for (int k = full * 8 + lane; k < total; k += 64) s_grid[k] = src[k];
        } else {
            const int cpe = cells / 8, full = n_here * cpe;             // 16-byte chunks per env (cells % 16 == 0)
            for (int c = lane; c < full; c += 64) {
                const uint4 v = reinterpret_cast<const uint4 *>(src)[c];
                const int env = c / cpe, off = c - env * cpe;
                uint32_t *d = s_dw + env * (pitch / 2) + off * 4;
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            }
        }
    }
    if (x.field) {
        // the field of the wavefront's envs starts out "no path": one contiguous block, 16-byte stores
        uint16_t *dst = x.field + (size_t)e0 * H * cells;
        const int total = n_here * H * cells, full = total / 8;
        const uint4 ones = make_uint4(~0u, ~0u, ~0u, ~0u);
        for (int c = lane; c < full; c += 64) reinterpret_cast<uint4 *>(dst)[c] = ones;
        for (int k = full * 8 + lane; k < total; k += 64) dst[k] = 0xffffu;
        __threadfence();                                                // the lanes' per-node stores below land on top of the fill
    }
    __syncthreads();

    const int kind = task_kind(ts), target = task_target(ts);
    const int ax = axy & 0xffff, ay = (axy >> 16) & 0xffff;
    bool search = live && task_stage(ts) == STAGE_NAV && (x.ignore_done || code_done == 0) && ax < D && ay < D;
    const int c0 = (ay << SH) + ax;

    // the env's boards: cells inside the map, occupied cells, goals, goals that carry the target bit
    B inb = b_zero<W>(), occ = b_zero<W>(), goal = b_zero<W>(), tgt = b_zero<W>();
    if (search) {
        const StepRule rule = step_rule(p);
        const uint16_t *lg = s_grid + lane * pitch;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            u64 m_in = 0, m_occ = 0, m_goal = 0, m_tgt = 0;
            for (int r = 0; r < RPW; ++r) {
                const int y = i * RPW + r;
                if (y >= D) break;
                for (int xx = 0; xx < D; ++xx) {
                    const int cell = y * D + xx;
                    const uint32_t code = lg[cell];
                    const u64 bit = 1ull << ((r << SH) + xx);
                    m_in |= bit;
                    if (code == 0) continue;
                    m_occ |= bit;
                    const bool is_goal = hit_is_goal(rule, (int)code, cell, gc);
                    if (is_goal) m_goal |= bit;
                    if (is_goal && (code & CELL_TARGET_BIT)) m_tgt |= bit;
                }
            }
            inb.w[i] = m_in; occ.w[i] = m_occ; goal.w[i] = m_goal; tgt.w[i] = m_tgt;
        }
    }
    // where the agent can stand: the empty cells and its own (with the agent placed elsewhere, its cell is empty)
    const B free = search ? b_or(b_andn(inb, occ), b_bit<W>(c0)) : b_zero<W>();

    const bool between = kind == TASK_BETWEEN;
    const bool direction = kind == TASK_DIRECTION && target >= 0;
    const int mid = between && target >= 0 && target < cells ? ((target / D) << SH) + target % D : -1;
    const bool mid_ok = search && mid >= 0 && b_test(free, mid);
    const B midb = mid_ok ? b_bit<W>(mid) : b_zero<W>();

    // goals whose bump with heading d wins
    auto winning_goals = [&](int d) -> B {
        if (between) return b_zero<W>();
        if (!direction) return b_and(goal, tgt);
        // (direction(g, referent, yaw), near): the referent one cell from g, the word that of the referent seen from g
        const int rc = target & 0xff, word = (target >> 8) & 7;
        B r = b_zero<W>();
        if (rc >= cells) return r;
        const int rx = rc % D, ry = rc / D, vx = dir_dx(d), vy = dir_dy(d);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int v2x = dir_dx(o), v2y = dir_dy(o), gx = rx - v2x, gy = ry - v2y;
            if (direction_word(vx, vy, v2x, v2y) == word && (unsigned)gx < (unsigned)D && (unsigned)gy < (unsigned)D) r = b_or(r, b_bit<W>((gy << SH) + gx));
        }
        return b_and(r, goal);
    };
    // does leaving the agent on `cell` with heading d by action a count as "stays put without a wrong goal"?
    auto harmless_stay = [&](int cell, int d, int a) -> bool {
        const int md = action_dir<EGO>(a, d);
        if (md < 0) return true;                                        // a turn
        const int tx = (cell & (S - 1)) + dir_dx(md), ty = (cell >> SH) + dir_dy(md);
        if ((unsigned)tx >= (unsigned)D || (unsigned)ty >= (unsigned)D) return true;
        const int t = (ty << SH) + tx;
        if (b_test(free, t)) return false;                              // it moves
        return !(md == d && b_test(goal, t));                           // blocked: harmless unless a goal is bumped along the heading
    };

    // level 1: the nodes that win at once
    B front[H], seen[H];
#pragma unroll
    for (int hs = 0; hs < H; ++hs) {
        const int d = EGO ? hs : 1;
        B s1 = b_shift(winning_goals(d), (d + 2) & 3);                  // the cell in front of which the goal lies
        if (mid_ok) {
            s1 = b_or(s1, b_around(midb));
            bool stay = EGO;                                            // a turn on the middle cell
            if (!EGO) for (int a = 0; a < 4; ++a) stay = stay || harmless_stay(mid, d, a);
            if (stay) s1 = b_or(s1, midb);
        }
        front[hs] = seen[hs] = b_and(s1, free);
    }

    const int hs0 = EGO ? dir0 : 0;
    constexpr int NA = EGO ? 6 : 4;
    int dist = EXPERT_NO_PATH, action = x.no_path_action;
    uint16_t *fld = x.field ? x.field + (size_t)e * H * cells : nullptr;
    auto store_level = [&](const B (&set)[H], int level) {
        if (!fld) return;
#pragma unroll
        for (int hs = 0; hs < H; ++hs)
#pragma unroll
            for (int i = 0; i < W; ++i) {
                u64 w = set[hs].w[i];
                for (int k = 0; k < 64 && w; ++k) {
                    const int b = __ffsll((long long)w) - 1 + i * 64;
                    w &= w - 1;
                    fld[hs * cells + (b >> SH) * D + (b & (S - 1))] = (uint16_t)level;
                }
            }
    };

    if (search && b_test(b_pick(front, hs0), c0)) {
        // the lowest action that wins now: the forward rule, action by action
        dist = 1;
        const B win0 = winning_goals(dir0);
        for (int a = NA - 1; a >= 0; --a) {
            const int md = action_dir<EGO>(a, dir0);
            bool wins;
            if (md < 0) wins = c0 == mid;
            else {
                const int tx = ax + dir_dx(md), ty = ay + dir_dy(md);
                const bool inside = (unsigned)tx < (unsigned)D && (unsigned)ty < (unsigned)D;
                const int t = inside ? (ty << SH) + tx : c0;
                if (inside && b_test(free, t)) wins = t == mid;
                else if (inside && md == dir0 && b_test(goal, t)) wins = b_test(win0, t);
                else wins = c0 == mid;
            }
            if (wins) action = a;
        }
    }
    store_level(front, 1);

    const int max_levels = H * cells;                                   // a node enters one level at most
    for (int level = 2; level <= max_levels; ++level) {
        bool more = false;
#pragma unroll
        for (int hs = 0; hs < H; ++hs) more = more || b_any(front[hs]);
        if (!more || (!fld && dist >= 0)) break;
        B next[H];
#pragma unroll
        for (int hs = 0; hs < H; ++hs) {
            B n = b_around(front[hs]);
            if (EGO) n = b_or(n, b_or(front[(hs + 1) & 3], front[(hs + 3) & 3]));
            next[hs] = b_andn(b_and(n, free), seen[hs]);
        }
        if (dist < 0 && b_test(b_pick(next, hs0), c0)) {
            // the agent's node: the lowest action whose successor is one level closer
            dist = level;
            for (int a = NA - 1; a >= 0; --a) {
                const int md = action_dir<EGO>(a, dir0);
                bool closer;
                if (md < 0) closer = b_test(b_pick(front, (dir0 + (a == 4 ? 3 : 1)) & 3), c0);
                else {
                    const int tx = ax + dir_dx(md), ty = ay + dir_dy(md);
                    const bool inside = (unsigned)tx < (unsigned)D && (unsigned)ty < (unsigned)D;
                    const int t = inside ? (ty << SH) + tx : c0;
                    closer = inside && b_test(free, t) && b_test(b_pick(front, hs0), t);
                }
                if (closer) action = a;
            }
        }
#pragma unroll
        for (int hs = 0; hs < H; ++hs) { seen[hs] = b_or(seen[hs], next[hs]); front[hs] = next[hs]; }
        store_level(front, level);
    }
    if (live) {
        if (x.actions) x.actions[e] = action;
        if (x.dist) x.dist[e] = dist;
    }
}

}  // namespace

hipError_t launch_xw_expert(const XwParams &p, int32_t *actions, int32_t *dist, uint16_t *field, int no_path_action, bool ignore_done,
                            hipStream_t s) {
    const ExpertArgs x{actions, dist, field, no_path_action, ignore_done ? 1 : 0};
    const dim3 grid((p.n + 63) / 64), block(64);
    const int cells = p.max_dim * p.max_dim, pitch = cells + ((p.max_dim & 3) == 0 ? 2 : 0);
    const size_t lds = ((size_t)64 * pitch * 2 + 15) & ~(size_t)15;
    const bool small = p.max_dim <= 8;
    if (p.visible_radius) {
        if (small) hipLaunchKernelGGL((xw_expert_kernel<1, true>), grid, block, lds, s, p, x);
        else hipLaunchKernelGGL((xw_expert_kernel<4, true>), grid, block, lds, s, p, x);
    } else {
        if (small) hipLaunchKernelGGL((xw_expert_kernel<1, false>), grid, block, lds, s, p, x);
        else hipLaunchKernelGGL((xw_expert_kernel<4, false>), grid, block, lds, s, p, x);
    }
    return hipGetLastError();
}

}  // namespace xwb
