// kernels_xworld_reset.hip -- XWorld2D reset path (map generation + teacher idle stage) for gfx950.
//
// Replaces, per environment of the compacted "done" list (or of the whole batch):
//   XWorld::reset (xworld/xworld.cpp:109-151), XWorldEnv.reset / __instantiate_entities / __padding_walls /
//   cpp_get_entities (maps/xworld_env.py:95-101,376-384,412-493), XWorldNav._configure (maps/XWorldNav.py:16-67),
//   XWorldWalls._configure (maps/XWorldWalls.py:14-36), spanning_tree_maze_generator (python/maze2d.py:74-114),
//   XWorld3DNavTarget.idle (xworld3d/tasks/XWorld3DNavTarget.py:28-43) with _reachable / bfs
//   (xworld3d_task.py:328-342, maze2d.py:43-71), XWorldSimulator::reset_game (xworld_simulator.cpp:143-157).
//
// One lane generates one map (decision order "xwb-mapgen-v1").  Only ~0.35 % of the envs
// finish per step, so this kernel is latency-bound: every per-cell set (maze walls, free cells, flooded
// cells) is a bit mask held in registers (NW x 64 bits for D*D cells), "k-th free cell in row-major order"
// is a rank-select on the mask, the flood fill is shift-and-mask on whole rows, and the only indexed
// storage -- the DFS stack, the shuffled wall list and a few per-goal words -- lives in LDS laid out
// [index][lane] so the 64 lanes of the wavefront never share a bank row entry.  Cells are written to the
// env's grid row in HBM with fire-and-forget stores.
// one out-of-line copy of the Philox block function: this kernel runs on a couple of wavefronts whose
// instruction fetches miss all the way to L2 while render_all saturates the memory system
#define XWB_PHILOX_ATTR __noinline__
#include <type_traits>
#include "xwb_common.h"
#include "xw_step_rule.h"
#include "xw_board.h"
#include "../../include/xwb_trig.h"

namespace xwb {

struct IconTables {
    const int16_t *first[3];
    const int16_t *variants;
    __device__ __forceinline__ int nv(int type, int name) const { return first[type][name + 1] - first[type][name]; }
    __device__ __forceinline__ int icon(int type, int name, int k) const { return variants[first[type][name] + k]; }
};

// per-lane indexed storage in LDS: element i of lane l at [i * 64 + l]
struct LaneLds {
    uint32_t *stack;     // [64]  DFS frames: node | perm << 8 | next << 16 (the maze generator's: the reset kernel only)
    uint8_t *blk;        // [cells] shuffled '#' cells
    uint16_t *gname;     // [XW_MAX_GOALS]
    uint8_t *gcell;      // [XW_MAX_GOALS]
    uint16_t *ov_idx;    // [XW_MAX_GOALS]
    uint16_t *ov_val;    // [XW_MAX_GOALS]
    uint16_t *gicon;     // [XW_MAX_GOALS] (aliases ov_idx: the name overrides are dead once the goals are placed)
    int lane;
    __device__ __forceinline__ int at(int i) const { return i * 64 + lane; }
    // the one layout, [stack] gname ov_idx ov_val gcell blk, from the dynamic LDS base; returns the first byte behind it
    __device__ __forceinline__ uint8_t *carve(uint32_t *lds32, bool with_stack, int cells) {
        lane = threadIdx.x;
        stack = lds32;                                                              // 64 x 64 x 4 B
        gname = reinterpret_cast<uint16_t *>(lds32 + (with_stack ? 64 * 64 : 0));   // 16 x 64 x 2 B
        ov_idx = gname + XW_MAX_GOALS * 64;
        ov_val = ov_idx + XW_MAX_GOALS * 64;
        gicon = ov_idx;
        gcell = reinterpret_cast<uint8_t *>(ov_val + XW_MAX_GOALS * 64);            // 16 x 64 B
        blk = gcell + XW_MAX_GOALS * 64;                                            // cells x 64 B
        return blk + cells * 64;
    }
    // bytes of that layout (what the launcher asks for): the stack, 2 + 2 + 2 + 1 B per goal slot, 1 B per cell, x 64 lanes
    static size_t bytes(bool with_stack, int cells) { return (with_stack ? 64 * 64 * 4 : 0) + (7 * XW_MAX_GOALS + (size_t)cells) * 64; }
};
// cells of the largest board an env of the batch may hold (a curriculum env may be at any level): sizes blk, picks NW
__host__ __device__ __forceinline__ int xw_board_cells(const XwParams &p) { const int d = p.curriculum != 0 ? p.max_dim : p.dim; return d * d; }

// maze2d.spanning_tree_maze_generator: bit c set = '#'.  Randomised DFS over the n x n node lattice with an
// explicit stack; each node shuffles [(-1,0),(1,0),(0,1),(0,-1)] by Fisher-Yates i = 3..1, j = below(i+1).
template <int NW>
__device__ __forceinline__ Mask<NW> xw_maze(Stream &s, int D, const LaneLds &L) {
    int X = D;
    const bool pad = (X % 2) == 0;
    if (pad) X -= 1;
    const int n = (X + 1) / 2;
    Mask<NW> mz;
    mz.clear();
    for (int y = 0; y < X; ++y)
        for (int x = 0; x < X; ++x)
            if (!(x % 2 == 0 && y % 2 == 0)) mz.set(y * D + x);
    // The k-th *visited* node consumes draws 3k..3k+2 whatever the DFS path is, so all n*n shuffles are drawn
    // up front in a loop every lane runs in lock step (the DFS below is divergent in time across lanes and
    // must stay cheap per iteration).  perm table: L.blk is free until the '#' list is built.
    for (int k = 0; k < n * n; ++k) {
        int m0 = 0, m1 = 1, m2 = 2, m3 = 3;
        {   // i = 3
            const int j = (int)s.below(4u);
            const int vj = j == 0 ? m0 : (j == 1 ? m1 : (j == 2 ? m2 : m3));
            const int vi = m3;
            if (j == 0) m0 = vi; else if (j == 1) m1 = vi; else if (j == 2) m2 = vi;
            m3 = vj;
        }
        {   // i = 2
            const int j = (int)s.below(3u);
            const int vj = j == 0 ? m0 : (j == 1 ? m1 : m2);
            const int vi = m2;
            if (j == 0) m0 = vi; else if (j == 1) m1 = vi;
            m2 = vj;
        }
        {   // i = 1
            const int j = (int)s.below(2u);
            const int vj = j == 0 ? m0 : m1;
            const int vi = m1;
            if (j == 0) m0 = vi;
            m1 = vj;
        }
        L.blk[L.at(k)] = (uint8_t)(m0 | (m1 << 2) | (m2 << 4) | (m3 << 6));
    }
    uint64_t visited = 0;
    int sp = 1, n_visited = 0;
    L.stack[L.at(0)] = 0u | (0xffu << 16);
    while (sp > 0) {
        const int top = sp - 1;
        uint32_t f = L.stack[L.at(top)];
        const int node = f & 0xff;
        int perm = (f >> 8) & 0xff, next = (f >> 16) & 0xff;
        const int cx = node % n, cy = node / n;
        if (next == 0xff) {
            visited |= 1ull << node;
            perm = L.blk[L.at(n_visited++)];
            next = 0;
        }
        if (next >= 4) { sp--; continue; }
        const int m = (perm >> (2 * next)) & 3;
        next += 1;
        L.stack[L.at(top)] = (uint32_t)node | ((uint32_t)perm << 8) | ((uint32_t)next << 16);
        const int dx = m == 0 ? -1 : (m == 1 ? 1 : 0);
        const int dy = m == 2 ? 1 : (m == 3 ? -1 : 0);
        const int nx = cx + dx, ny = cy + dy;
        if (nx >= 0 && nx < n && ny >= 0 && ny < n && !((visited >> (ny * n + nx)) & 1ull)) {
            mz.reset((cy + ny) * D + (cx + nx));                 // open the wall between the two nodes
            L.stack[L.at(sp)] = (uint32_t)(ny * n + nx) | (0xffu << 16);
            sp++;
        }
    }
    if (pad) {
        for (int i = 0; i < X; ++i) if (i % 2) mz.set(X * D + i);
        for (int i = 0; i < D; ++i) if (i % 2) mz.set(i * D + X);
    }
    return mz;
}

// An episode in the making: what the generators fill in, the idle stages may rearrange and xw_commit writes out.  The goal
// slots (cell, name, icon; entity order) are the LDS columns L.gcell / L.gname / L.gicon; cells are indices of the actual dims.
template <int NW>
struct Draft {
    Mask<NW> occupied;                                     // blocks and goals
    int agent_cell, agent_icon, ng;                        // ng: goal slots in use
    uint32_t target_bits = 0;                              // goal slot i belongs to self.target
    int sent_a = 0xffff, sent_b = 0xffff;                  // names bound into the teacher's grammar (G / G1, G2)
    int between = -1;                                      // NavTargetBetween's middle cell
    __device__ __forceinline__ explicit Draft(int ng_) : ng(ng_) { occupied.clear(); }
};

// goal slot -> grid cell (the egocentric render finds a goal's pose by it; the 2-D-native idle stages read it)
template <int NW>
__device__ __forceinline__ void xw_write_goal_table(const Board<NW> &B, const LaneLds &L, int ng, uint8_t *gc) {
    for (int i = 0; i < XW_MAX_GOALS; ++i) gc[i] = i < ng ? (uint8_t)B.grid_index(L.gcell[L.at(i)]) : (uint8_t)0xff;
}

// The draft's write-out, shared by the reset and by a mid-episode idle stage: goal cells carry bit 15 when the goal belongs to
// the target set (the step kernel's whole reward rule); `table`: goal_cells is not already written by a 2-D idle stage.
template <int NW>
__device__ __forceinline__ void xw_commit(const XwParams &p, const Board<NW> &B, const LaneLds &L, const Draft<NW> &d, uint16_t *g,
                                          size_t ew, bool table) {
    for (int i = 0; i < d.ng; ++i)
        g[B.grid_index(L.gcell[L.at(i)])] = (uint16_t)((L.gicon[L.at(i)] + 1) | (((d.target_bits >> i) & 1u) ? 0x8000u : 0u));
    if (table) xw_write_goal_table(B, L, d.ng, p.goal_cells + ew * XW_MAX_GOALS);
    p.agent_xy[ew] = (d.agent_cell % B.D + B.off) | ((d.agent_cell / B.D + B.off) << 16);
    p.sent_names[ew] = (uint32_t)d.sent_a | ((uint32_t)d.sent_b << 16);
}

// ---- The idle stage of an XWorld3DNav* task on one env's board (decision order "xwb-taskgen-v1"): shared by the
// reset kernel (the episode's first teach()) and by xw_idle3d_kernel (exclusive group scheduling: an idle XWorld3DNav* group
// picked in mid-episode, teacher.cpp:209-220).  Its stages, in the order xw_idle_stage_3d runs them:

// XWorld3DNavTarget.idle / XWorld3DNavTargetAvoid.idle: pick a goal reachable from the agent (_reachable / bfs) with blocks and
// the other goals as obstacles -- flood the empty cells from the agent; a goal is reachable iff one of its 4-neighbours is
// flooded --, then the target set
template <int NW>
__device__ __forceinline__ void idle3d_pick_reachable(Stream &s, const Board<NW> &B, const LaneLds &L, Draft<NW> &d, int kind, int &tf) {
    const int ng = d.ng;
    const Mask<NW> reach = B.flood(d.agent_cell, B.valid.andnot(d.occupied));   // agent cell included: it is the seed
    int nc = 0;
    uint32_t cand_bits = 0;                                      // the reachable goals' slots
    for (int i = 0; i < ng; ++i)
        if ((B.neighbours(Mask<NW>(L.gcell[L.at(i)])) & reach).any()) { cand_bits |= 1u << i; nc++; }
    if (nc == 0) return;                                         // assert targets, "map too crowded?"
    int k = (int)s.below((uint32_t)nc);                          // sel_goal = random.choice(targets)
    int pick = 0;
    for (int i = 0; i < ng; ++i)
        if ((cand_bits >> i) & 1u) { if (k == 0) { pick = i; break; } k--; }
    const int selname = L.gname[L.at(pick)];
    if (kind == TASK_TARGET) {
        tf = selname;
        d.sent_a = selname;
        for (int i = 0; i < ng; ++i) if (L.gname[L.at(i)] == selname) d.target_bits |= 1u << i;
    } else {
        int nr = 0;
        for (int i = 0; i < ng; ++i) if (L.gname[L.at(i)] != selname) nr++;
        if (nr == 0) return;                                     // assert referents
        int r = (int)s.below((uint32_t)nr);                      // referent = random.choice(referents)
        int refname = 0;
        for (int i = 0; i < ng; ++i)
            if (L.gname[L.at(i)] != selname) { if (r == 0) { refname = L.gname[L.at(i)]; break; } r--; }
        for (int i = 0; i < ng; ++i) if (L.gname[L.at(i)] != refname) d.target_bits |= 1u << i;
        d.sent_a = refname;
    }
}

// _get_p_tiles (Near) / _get_t_tiles (Between) / _get_l_tiles (Direction) over the available cells A: mask M[m] holds the
// anchor cells of the tiles of shape m.  Every kind fills all six (shapes it lacks stay empty): the caller's array is written
// at the same constant indices on every path, which keeps it in registers.
template <int NW>
__device__ __forceinline__ void idle3d_tile_masks(const Board<NW> &B, const Mask<NW> &A, int kind, Mask<NW> M[6]) {
    const int D = B.D;
    auto from_right = [&](const Mask<NW> &m) { return m.andnot(B.col0).shr(1); };   // bit c = m[c+1], x < D-1
    const Mask<NW> Nl = A.andnot(B.colN).shl(1) & B.valid, Nr = from_right(A), Nu = A.shl(D) & B.valid, Nd = A.shr(D);
    Mask<NW> T[6];
    for (int m = 0; m < 6; ++m) T[m].clear();
    if (kind == TASK_NEAR) {                                     // _get_p_tiles
        const Mask<NW> C1 = Nl | Nr | Nu | Nd;
        const Mask<NW> C2 = (Nl & Nr) | (Nl & Nu) | (Nl & Nd) | (Nr & Nu) | (Nr & Nd) | (Nu & Nd);
        const Mask<NW> Hb = A & Nr, Vb = A & Nd, Db = A & from_right(A.shr(D));
        T[0] = Hb & from_right(C2); T[1] = Hb & C2;
        T[2] = Vb & C2.shr(D);      T[3] = Vb & C2;
        T[4] = Db & from_right(C1.shr(D)); T[5] = Db & C1;
    } else if (kind == TASK_BETWEEN) {                           // _get_t_tiles
        T[0] = A & Nl & Nr & (Nu | Nd);
        T[1] = A & Nu & Nd & (Nl | Nr);
    } else {                                                     // _get_l_tiles
        const Mask<NW> Tv = A & Nd & A.shr(2 * D);
        const Mask<NW> Th = A & Nr & from_right(Nr);
        T[0] = Tv; T[1] = Tv; T[2] = Th; T[3] = Th;
    }
    for (int m = 0; m < 6; ++m) M[m] = T[m];
}

template <int NW>
__device__ __forceinline__ int idle3d_tiles_below(const Mask<NW> M[6], int c) {      // tiles anchored at the cells below c
    int pre = 0;
    for (int m = 0; m < 6; ++m) pre += M[m].count_below(c);
    return pre;
}

// tiles[t0] of the shuffled tile list: tiles are listed cell-major, the shapes in order inside a cell -- find the cell tc,
// then the shape tm
template <int NW>
__device__ __forceinline__ void idle3d_pick_tile(const Board<NW> &B, const Mask<NW> M[6], int t0, int &tc, int &tm) {
    int lo = 0, hi = B.D * B.D;                                  // smallest c with tiles_below(c + 1) > t0
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (idle3d_tiles_below(M, mid + 1) > t0) hi = mid; else lo = mid + 1;
    }
    tc = lo; tm = 0;
    int r = t0 - idle3d_tiles_below(M, tc);
    for (int m = 0; m < 6; ++m) if (M[m].test(tc)) { if (r == 0) { tm = m; break; } r--; }
}

// the two goal cells (l1, l2) of the tile of shape tm anchored at cell tc
__device__ __forceinline__ void idle3d_tile_cells(int kind, int D, int tc, int tm, int &l1, int &l2) {
    if (kind == TASK_NEAR) {
        const int other = tm < 2 ? tc + 1 : (tm < 4 ? tc + D : tc + D + 1);
        l1 = (tm & 1) ? other : tc; l2 = (tm & 1) ? tc : other;
    } else if (kind == TASK_BETWEEN) {
        l1 = tm == 0 ? tc - 1 : tc - D; l2 = tm == 0 ? tc + 1 : tc + D;
    } else {
        const int st = tm < 2 ? D : 1;
        l1 = (tm & 1) ? tc + st : tc; l2 = (tm & 1) ? tc + 2 * st : tc + st;
    }
}

// _propagate_agent: flood fill from the seed over cells that hold neither blocks nor goals, the agent goes to a random cell of
// it; false: nowhere to go (assert new_a)
template <int NW>
__device__ __forceinline__ bool idle3d_place_agent(Stream &s, const Board<NW> &B, const LaneLds &L, const Mask<NW> &occupied, int seed,
                                                   bool inclusive, int &al) {
    const Mask<NW> fl = B.flood(seed, B.valid.andnot(occupied));
    const int na = (inclusive ? 0 : -1) + fl.count();            // the seed itself only counts when inclusive
    if (na <= 0) return false;
    const int ka = (int)s.below((uint32_t)na);                   // agent.loc, _ = random.choice(new_a)
    al = seed;
    if (inclusive && ka == 0) return true;
    // new_a is in BFS discovery order (moves left, right, up, down): replay the BFS up to entry ka
    const int want = inclusive ? ka - 1 : ka, D = B.D;
    Mask<NW> seen(seed);
    int head = 0, tail = 0, count = 0;
    L.blk[L.at(tail++)] = (uint8_t)seed;
    while (head < tail) {
        const int c = L.blk[L.at(head++)];
        const int cx = c % D, cy = c / D;
        for (int m = 0; m < 4; ++m) {
            const int nx = cx + (m == 0 ? -1 : (m == 1 ? 1 : 0)), ny = cy + (m == 2 ? -1 : (m == 3 ? 1 : 0));
            if (nx < 0 || ny < 0 || nx >= D || ny >= D) continue;
            const int nc2 = ny * D + nx;
            if (seen.test(nc2) || occupied.test(nc2)) continue;
            seen.set(nc2);
            L.blk[L.at(tail++)] = (uint8_t)nc2;
            if (count++ == want) { al = nc2; return true; }
        }
    }
    return true;
}

// REORDER (only where a later idle stage enumerates the goals: a batch with a 2-D-native group beside this one).
// env.entities: g1 and g2 were deleted and set again, so they now follow the other goals, in that order
// (xworld_env.py _delete_entity / _set_entity_inst).  A later idle stage that enumerates the goals -- the
// 2-D-native group's random.choice(targets) -- sees that order, so the goal slots take it too; the
// egocentric poses travel with their goals.
__device__ __forceinline__ void idle3d_reorder_slots(const XwParams &p, int e, const LaneLds &L, int ng, int g1, int g2) {
    const uint8_t c1 = L.gcell[L.at(g1)], c2 = L.gcell[L.at(g2)];
    const uint16_t i1 = L.gicon[L.at(g1)], i2 = L.gicon[L.at(g2)], n1 = L.gname[L.at(g1)], n2 = L.gname[L.at(g2)];
    double *gw = p.visible_radius ? p.goal_warp + (size_t)e * XW_MAX_GOALS * 6 : nullptr;
    double w1[6], w2[6];
    if (gw) for (int q = 0; q < 6; ++q) { w1[q] = gw[g1 * 6 + q]; w2[q] = gw[g2 * 6 + q]; }
    int k = 0;
    for (int i = 0; i < ng; ++i) {
        if (i == g1 || i == g2) continue;
        if (k != i) {
            L.gcell[L.at(k)] = L.gcell[L.at(i)]; L.gicon[L.at(k)] = L.gicon[L.at(i)]; L.gname[L.at(k)] = L.gname[L.at(i)];
            if (gw) for (int q = 0; q < 6; ++q) gw[k * 6 + q] = gw[i * 6 + q];
        }
        ++k;
    }
    L.gcell[L.at(k)] = c1; L.gicon[L.at(k)] = i1; L.gname[L.at(k)] = n1;
    L.gcell[L.at(k + 1)] = c2; L.gicon[L.at(k + 1)] = i2; L.gname[L.at(k + 1)] = n2;
    if (gw) for (int q = 0; q < 6; ++q) { gw[k * 6 + q] = w1[q]; gw[(k + 1) * 6 + q] = w2[q]; }
}

// self.target of Near / Between / Direction once the goals stand at l1, l2 (rl: the referent's cell, Direction only)
template <int NW>
__device__ __forceinline__ void idle3d_target_bits(const XwParams &p, int e, const Board<NW> &B, const LaneLds &L, Draft<NW> &d, int kind,
                                                   int l1, int l2, int rl, int direction, int &tf) {
    const int D = B.D;
    if (kind == TASK_NEAR) {
        // _get_surrounding_goals(refer=g1.loc): dist < 1.5 + 1e-3 = the 8-neighbourhood, goals AT g1.loc skipped
        for (int i = 0; i < d.ng; ++i) {
            const int c = L.gcell[L.at(i)];
            const int ddx = c % D - l1 % D, ddy = c / D - l1 / D;
            if (c != l1 && ddx >= -1 && ddx <= 1 && ddy >= -1 && ddy <= 1) d.target_bits |= 1u << i;
        }
    } else if (kind == TASK_BETWEEN) {
        d.between = (l1 + l2) / 2;
    } else {
        // navigation_reward: a reached goal g wins iff direction(g, referent) seen along the agent's constant
        // yaw 1.5707963 (heading +y) equals `direction` and g is within 1.0 + 1e-3 of the referent
        // (the step kernel evaluates the same test with the heading at that time -- it changes in egocentric
        // mode; the bits below are the answer for the heading at reset)
        const int hd = p.visible_radius ? p.agent_dir[e] : 1;
        const int hx = hd == 0 ? 1 : (hd == 2 ? -1 : 0), hy = hd == 1 ? 1 : (hd == 3 ? -1 : 0);
        for (int i = 0; i < d.ng; ++i) {
            const int c = L.gcell[L.at(i)];
            const int v2x = rl % D - c % D, v2y = rl / D - c / D;
            if (v2x * v2x + v2y * v2y != 1) continue;             // dist == 0 -> False; dist > 1.001 -> far
            if (direction_word(hx, hy, v2x, v2y) == direction) d.target_bits |= 1u << i;
        }
        tf = B.grid_index(rl) | (direction << 8);
    }
}

// g: the env's grid row.  REORDER: a 2-D-native group runs beside this one (idle3d_reorder_slots)
template <int NW, bool REORDER>
__device__ __forceinline__ void xw_idle_stage_3d(const XwParams &p, int e, Stream &s, const Board<NW> &B, const LaneLds &L, uint16_t *g,
                                                 Draft<NW> &d, int kind, int &tf) {
    const int D = B.D, ng = d.ng;
    if (kind == TASK_TARGET || kind == TASK_AVOID) {
        idle3d_pick_reachable(s, B, L, d, kind, tf);
    } else if (ng >= 2) {
        // ---- Near / Between / Direction: delete the agent and two goals, put the goals on a tile, re-place the agent
        Mask<NW> A = B.valid.andnot(d.occupied);                     // available_grids after _delete_entity(agent)
        const int d0 = (int)s.below((uint32_t)ng);                   // random.shuffle(goals); g1, g2 = goals[:2]
        const int d1 = (int)s.below((uint32_t)(ng - 1));
        const int g1 = d0, g2 = d1 < d0 ? d1 : d1 + 1;
        const int c1o = L.gcell[L.at(g1)], c2o = L.gcell[L.at(g2)];
        A.set(c1o); A.set(c2o);
        Mask<NW> M[6];
        idle3d_tile_masks(B, A, kind, M);
        int nt = 0;
        for (int m = 0; m < 6; ++m) nt += M[m].count();
        bool ok = nt > 0;                                            // assert tiles, "map too crowded?"
        int l1 = 0, l2 = 0, al = 0, direction = 0, tgt = g1, ref = g2;
        if (ok) {
            const int t0 = (int)s.below((uint32_t)nt);               // random.shuffle(tiles); tiles[0]
            if (nt >= 2) (void)s.below((uint32_t)(nt - 1));
            int tc, tm;
            idle3d_pick_tile(B, M, t0, tc, tm);
            idle3d_tile_cells(kind, D, tc, tm, l1, l2);
            d.occupied.reset(c1o); d.occupied.reset(c2o);
            d.occupied.set(l1); d.occupied.set(l2);                  // _set_entity_inst(g1), (g2)
            A.reset(l1); A.reset(l2);
            int seed = l2;
            bool inclusive = false;                                  // _propagate_agent([g2.loc]): the seed is no candidate
            if (kind == TASK_BETWEEN) {
                seed = (l1 + l2) / 2;                                // _middle_loc: same row or same column
            } else if (kind == TASK_DIRECTION) {
                Mask<NW> Ne = B.neighbours(Mask<NW>(l1)) & A;        // empty 4-neighbours of g1 ...
                if (!Ne.any()) { Ne = B.neighbours(Mask<NW>(l2)) & A; tgt = g2; ref = g1; }     // ... else of g2
                const int ne = Ne.count();
                if (ne == 0) ok = false;                             // assert empty_grids
                else {
                    const int ec = Ne.select((int)s.below((uint32_t)ne));    // random.choice(empty_grids), row-major
                    const int tl = tgt == g1 ? l1 : l2, rl = ref == g1 ? l1 : l2;
                    // __compute_triple_direction(target, referent, e): view = e -> target, v2 = target -> referent
                    const int v1x = tl % D - ec % D, v1y = tl / D - ec / D;
                    const int v2x = rl % D - tl % D, v2y = rl / D - tl / D;
                    direction = direction_word(v1x, v1y, v2x, v2y);
                    seed = ec; inclusive = true;                     // _propagate_agent([e], inclusive=True)
                }
            }
            if (ok) ok = idle3d_place_agent(s, B, L, d.occupied, seed, inclusive, al);
        }
        if (ok) {
            // the env changed: XWorld::reset(false).  Clear the three old cells, then write the new ones.
            g[B.grid_index(c1o)] = 0; g[B.grid_index(c2o)] = 0; g[B.grid_index(d.agent_cell)] = 0;
            L.gcell[L.at(g1)] = (uint8_t)l1; L.gcell[L.at(g2)] = (uint8_t)l2;
            g[B.grid_index(al)] = (uint16_t)(d.agent_icon + 1);
            d.agent_cell = al;
            d.sent_a = L.gname[L.at(kind == TASK_DIRECTION ? ref : g1)];
            if (kind == TASK_BETWEEN) d.sent_b = L.gname[L.at(g2)];
            if (REORDER) idle3d_reorder_slots(p, e, L, ng, g1, g2);
            idle3d_target_bits(p, e, B, L, d, kind, l1, l2, ref == g1 ? l1 : l2, direction, tf);
        }
    }
    if (kind == TASK_BETWEEN && d.between >= 0) tf = B.grid_index(d.between);
}

// ---- The idle stage of the 2-D-native group (rule D14b).  XWorldTask._reachable: bfs with the BLOCKS as the only obstacles;
// the agent never leaves its component and nothing else moves, so the candidate sets of every later idle stage of this episode
// are fixed here: goal_cells + cand2d are what the step kernel's idle stage reads.  draw: this stage also picks its target
// (else it only refreshes the tables after a 3-D stage rearranged the map).
template <int NW>
__device__ __forceinline__ void xw_idle_stage_2d(const XwParams &p, Stream &s, const Board<NW> &B, const LaneLds &L, const Draft<NW> &d,
                                                 size_t ew, int kind, bool draw, int &tf, int &st0) {
    Mask<NW> goalm; goalm.clear();
    for (int i = 0; i < d.ng; ++i) goalm.set(L.gcell[L.at(i)]);
    const Mask<NW> r2 = B.flood(d.agent_cell, B.valid.andnot(d.occupied.andnot(goalm)));
    uint32_t cand = 0;
    for (int i = 0; i < d.ng; ++i)
        if (r2.test(L.gcell[L.at(i)])) cand |= (1u << i) | (p.icon_colored[L.gicon[L.at(i)]] ? (1u << (16 + i)) : 0u);
    uint8_t *gc = p.goal_cells + ew * XW_MAX_GOALS;
    xw_write_goal_table(B, L, d.ng, gc);
    p.cand2d[ew] = cand;
    if (draw) {
        int tsteps0;
        idle_2d(kind, cand, gc, [&](uint32_t n) { return s.below(n); }, tf, st0, tsteps0);
    }
}

// ---- Map generation (decision order "xwb-mapgen-v1"), in the stages xw_reset_env runs ----

// XWorldNav._configure: level -> dims, goals, blocks (XWorldNav.py:27-34); XWorldWalls and a batch without curriculum: the conf's
template <int KIND>
__device__ __forceinline__ void xw_level(const XwParams &p, int e, int &dim, int &goals, int &blocks) {
    dim = p.dim; goals = p.num_goals; blocks = p.num_blocks;
    if (KIND != 0 || p.curriculum == 0) return;
    const int level = curriculum_configure(p, e);
    dim = 3 + level; goals = level < 3 ? 2 : 4; blocks = level == 5 ? 16 : 3 * level;
}

// random.choice(available_grids) over the free cells in row-major order; the cell leaves the set
template <int NW>
__device__ __forceinline__ int xw_take_free_cell(Stream &s, Mask<NW> &avail, int &na) {
    const int c = avail.select((int)s.below((uint32_t)na));
    avail.reset(c); na--;
    return c;
}

// Place one entity of `type` (0 goal, 1 block, 2 agent) on cell c: its name (drawn among the type's names unless given), one of
// the name's icon variants, the cell's code; returns the icon
template <int NW>
__device__ __forceinline__ int xw_place(const XwParams &p, const IconTables &T, Stream &s, const Board<NW> &B, uint16_t *g, int c, int type,
                                        int nm = -1) {
    if (nm < 0) nm = (int)s.below((uint32_t)p.n_names[type]);
    const int v = (int)s.below((uint32_t)T.nv(type, nm));
    const int ic = T.icon(type, nm, v);
    g[B.grid_index(c)] = (uint16_t)(ic + 1);
    return ic;
}

// The pose of a goal's icon in egocentric mode.  xworld_env.py:211-223: yaw ~ U[0, 4 * PI_2), scale ~ U[0.5, 1], offset ~
// U[0, 1 - scale]; random.uniform(a, b) = a + (b - a) * random() with random() = unit().  XItem::get_item_image
// (xitem.cpp:33-63) then warps the icon by getRotationMatrix2D(centre, 90 - yaw * 180 / M_PI, scale) plus the translation
// (offset + scale / 2 - 0.5) * 64; cv::warpAffine inverts that matrix: the inverse is what the egocentric render needs, so
// it is stored (gw: the goal slot's six doubles).
__device__ __forceinline__ void xw_goal_pose(Stream &s, double *gw) {
    const double u0 = (double)s.unit(), u1 = (double)s.unit(), u2 = (double)s.unit();
    const double yaw = 0 + (1.5707963 * 4 - 0) * u0;
    const double scale = 0.5 + (1 - 0.5) * u1;
    const double offset = 0 + ((1 - scale) - 0) * u2;
    const double angle = (90 - yaw * 180 / 3.14159265358979323846) * 3.1415926535897932384626433832795 / 180;
    double sn, cs;                                  // include/xwb_trig.h: the same bits on the host's checker
    xwb_sincos(angle, &sn, &cs);
    const double alpha = cs * scale, beta = sn * scale;
    double M[6] = {alpha, beta, (1 - alpha) * 32.0 - beta * 32.0, -beta, alpha, beta * 32.0 + (1 - alpha) * 32.0};
    M[2] += (offset + scale / 2 - 0.5) * 64;
    M[5] += (offset + scale / 2 - 0.5) * 64;
    double Dt = M[0] * M[4] - M[1] * M[3];
    Dt = Dt != 0 ? 1. / Dt : 0;
    const double A11 = M[4] * Dt, A22 = M[0] * Dt;
    M[0] = A11; M[1] *= -Dt; M[3] *= -Dt; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5], b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
    for (int k = 0; k < 6; ++k) gw[k] = M[k];
}

// XWorldNav: distinct goal names (shuffle + pop), maze, shuffled '#' list, placement of goals, blocks, agent
template <int NW>
__device__ __forceinline__ void xw_gen_nav(const XwParams &p, const IconTables &T, const LaneLds &L, Stream &s, const Board<NW> &B,
                                           uint16_t *g, int e, int n_blocks, Draft<NW> &d) {
    const int M = p.n_names[0];
    int n_ov = 0;
    for (int i = 0; i < d.ng; ++i) {
        const int j = (int)s.below((uint32_t)(M - i));
        int vj = j, vl = M - 1 - i, at_j = -1;
        for (int k = 0; k < n_ov; ++k) {
            const int idx = L.ov_idx[L.at(k)];
            if (idx == j) { vj = L.ov_val[L.at(k)]; at_j = k; }
            if (idx == M - 1 - i) vl = L.ov_val[L.at(k)];
        }
        L.gname[L.at(i)] = (uint16_t)vj;
        if (at_j >= 0) L.ov_val[L.at(at_j)] = (uint16_t)vl;               // names[j] = names[M-1-i]
        else { L.ov_idx[L.at(n_ov)] = (uint16_t)j; L.ov_val[L.at(n_ov)] = (uint16_t)vl; n_ov++; }
    }
    const Mask<NW> mz = xw_maze<NW>(s, B.D, L);
    int nb = 0;
#pragma unroll
    for (int wi = 0; wi < NW; ++wi) {                     // '#' cells in row-major order
        uint64_t v = mz.w[wi];
        while (v) {
            const int b = __ffsll((long long)v) - 1;
            L.blk[L.at(nb++)] = (uint8_t)(wi * 64 + b);
            v &= v - 1;
        }
    }
    Mask<NW> avail = B.valid.andnot(mz);
    int na = B.D * B.D - nb;
    for (int i = nb - 1; i >= 1; --i) {                   // random.shuffle(blocks)
        const int j = (int)s.below((uint32_t)(i + 1));
        const uint8_t a = L.blk[L.at(i)], b = L.blk[L.at(j)];
        L.blk[L.at(i)] = b; L.blk[L.at(j)] = a;
    }
    for (int i = 0; i < d.ng; ++i) {
        const int c = xw_take_free_cell(s, avail, na);
        const int ic = xw_place(p, T, s, B, g, c, 0, L.gname[L.at(i)]);
        d.occupied.set(c);
        L.gcell[L.at(i)] = (uint8_t)c;
        L.gicon[L.at(i)] = (uint16_t)ic;
        if (p.visible_radius) xw_goal_pose(s, p.goal_warp + ((size_t)e * XW_MAX_GOALS + i) * 6);
    }
    for (int i = 0; i < n_blocks; ++i) {
        const int c = L.blk[L.at(--nb)];                   // blocks.pop()
        xw_place(p, T, s, B, g, c, 1);
        d.occupied.set(c);
    }
    d.agent_cell = xw_take_free_cell(s, avail, na);
    d.agent_icon = xw_place(p, T, s, B, g, d.agent_cell, 2);
    // xworld_env.py:208-210: yaw = random.choice(range(-1, 3)) * PI_2 -> heading up, right, down, left
    if (p.visible_radius) p.agent_dir[e] = (uint8_t)((s.below(4u) + 3u) & 3u);
}

// XWorldWalls: one full brick row, a partial brick column, then agent, goals, blocks
template <int NW>
__device__ __forceinline__ void xw_gen_walls(const XwParams &p, const IconTables &T, const LaneLds &L, Stream &s, const Board<NW> &B,
                                             uint16_t *g, int n_blocks, Draft<NW> &d) {
    const int D = B.D;
    Mask<NW> avail = B.valid;
    int nb = 0;
    const int row = (int)s.below((uint32_t)D);
    const int first = n_blocks < D ? n_blocks : D;
    for (int i = 0; i < first; ++i) L.blk[L.at(nb++)] = (uint8_t)(row * D + i);
    n_blocks -= first;
    const int column = (int)s.below((uint32_t)D);
    const int lim = n_blocks < D - 1 ? n_blocks : D - 1;
    for (int i = 0, j = 0; j < lim; ++i) if (i != row) { L.blk[L.at(nb++)] = (uint8_t)(i * D + column); j++; }
    for (int i = 0; i < nb; ++i) avail.reset(L.blk[L.at(i)]);
    int na = D * D - nb;
    d.agent_cell = xw_take_free_cell(s, avail, na);
    d.agent_icon = xw_place(p, T, s, B, g, d.agent_cell, 2);
    for (int i = 0; i < d.ng; ++i) {
        const int c = xw_take_free_cell(s, avail, na);
        const int nm = (int)s.below((uint32_t)p.n_names[0]);
        const int ic = xw_place(p, T, s, B, g, c, 0, nm);
        d.occupied.set(c);
        L.gcell[L.at(i)] = (uint8_t)c;
        L.gname[L.at(i)] = (uint16_t)nm;
        L.gicon[L.at(i)] = (uint16_t)ic;
    }
    for (int i = 0; i < nb; ++i) {
        const int c = L.blk[L.at(i)];
        xw_place(p, T, s, B, g, c, 1);
        d.occupied.set(c);
    }
}

// Group scheduling at reset -- the teacher's idle stage (TaskGroup::run_stage samples one task of the group per episode, then
// its idle()): decision order "xwb-taskgen-v1" (DESIGN.md).  Nothing is written to the grid before a stage has succeeded, so
// the "map too crowded?" cases (the reference asserts) simply keep the generated map.
// One or two task groups (conf order), each: TaskGroup::run_stage draws a task, Task::reset, its idle stage.  The 3-D-family
// stage may rearrange the map; the 2-D-family stage only reads it (its candidate tables are refreshed when it ran before a
// rearrangement: every later idle stage of the episode sees the final map).  kindv / tfv / st0v: per group, conf order.
// GM (task groups, compile time so that the usual one-group batch carries none of the other paths): 0 = one XWorld3DNav*
// group, 1 = one 2-D-native group, 2 = two groups
template <int NW, int GM>
__device__ __forceinline__ void xw_schedule_groups(const XwParams &p, int e, uint32_t ep, size_t ew, Stream &s, const Board<NW> &B,
                                                   const LaneLds &L, uint16_t *g, Draft<NW> &d, int kindv[2], int tfv[2], int st0v[2]) {
    int tf_unused, st_unused;
    const bool first_2d = GM == 1 || (GM == 2 && p.group2d);
    if (GM == 2 && p.exclusive) {
        // Teacher::teach's exclusive branch at reset (teacher.cpp:209-220 after reset_after_game_reset): the groups are
        // re-sorted, nobody is busy, so the group that now heads the list runs its idle stage -- the other one stays idle
        // until a later teach() picks it (an XWorld3DNav* group then rearranges the map in mid-episode: xw_idle3d_kernel).
        const int pick = xw_sort_groups(p, e, ep, 0u, p.grp_order[e] & 1), other = pick ^ 1;
        const bool pick_2d = pick == 0 ? first_2d : !first_2d;
        const int tsel = pick ? sample_task<1>(p, s, e) : sample_task<0>(p, s, e);
        kindv[pick] = pick ? task_at<1>(p, tsel) : task_at<0>(p, tsel);
        kindv[other] = TASK_TARGET; tfv[other] = -1; st0v[other] = STAGE_IDLE;       // TaskGroup::reset: no busy task
        if (pick_2d) {
            xw_idle_stage_2d(p, s, B, L, d, ew, kindv[pick], true, tfv[pick], st0v[pick]);
        } else {
            xw_idle_stage_3d<NW, true>(p, e, s, B, L, g, d, kindv[pick], tfv[pick]);
            xw_idle_stage_2d(p, s, B, L, d, ew, TASK2D_TARGET, false, tf_unused, st_unused);   // the 2-D group's candidate tables, from the final map
        }
        p.grp_order[e] = (uint8_t)(pick | (pick << 1));
        return;
    }
    if (p.exclusive && GM != 2 && p.minstd) {             // one group: the sort still draws once from the reference's engine
        uint32_t x = p.minstd[e];
        (void)xwb_minstd_rand_range_state(&x, (float)p.group_weight[0]);
        p.minstd[e] = x;
    }
    const int tsel0 = sample_task<0>(p, s, e);
    kindv[0] = p.n_tasks > 0 ? task_at<0>(p, tsel0) : TASK_TARGET;
    if (GM != 0 && first_2d) xw_idle_stage_2d(p, s, B, L, d, ew, kindv[0], true, tfv[0], st0v[0]);
    if (GM != 1 && !first_2d) xw_idle_stage_3d<NW, GM == 2>(p, e, s, B, L, g, d, kindv[0], tfv[0]);
    if (GM == 2) {
        const int tsel1 = sample_task<1>(p, s, e);
        kindv[1] = task_at<1>(p, tsel1);
        if (!first_2d) xw_idle_stage_2d(p, s, B, L, d, ew, kindv[1], true, tfv[1], st0v[1]);
        else xw_idle_stage_3d<NW, true>(p, e, s, B, L, g, d, kindv[1], tfv[1]);
        if (first_2d) xw_idle_stage_2d(p, s, B, L, d, ew, kindv[0], false, tf_unused, st_unused);
    }
}

template <int NW, int KIND, int GM>
__device__ void xw_reset_env(const XwParams &p, const IconTables &T, const LaneLds &L, int e, bool keep_done,
                             const uint4 *pre_draws, uint32_t n_pre_draws, int mode_all) {
    int level_dim, level_goals, level_blocks;
    xw_level<KIND>(p, e, level_dim, level_goals, level_blocks);
    const Board<NW> B(level_dim, p.max_dim);
    const int MD = B.MD, D = B.D, off = B.off;
    // shadow (a pre-generated episode): the one after the newest this env already holds -- sh_ep counts them, so the number
    // does not depend on whether the live counter has been bumped yet by whoever installs the previous one; written into
    // shadow slot (episode & 1) of the swapped-in arrays (index ew), the live counters and flags are left alone
    const uint32_t ep = (p.shadow && mode_all == 0 ? p.sh_ep[e] : p.episode[e]) + 1;
    if (!p.shadow) p.episode[e] = ep;
    else p.sh_ep[e] = ep;
    const size_t ew = p.shadow ? (size_t)(ep & 1u) * (size_t)p.n + (size_t)e : (size_t)e;
    Stream s;
    s.init(p.seed, p.env_gid0 + (uint32_t)e, ep, 0);
    s.pre = (Stream::lds_block_ptr)pre_draws; s.npre = n_pre_draws;

    // grid row: brick padding outside the actual dims, empty inside; entity cells are overwritten below
    // (same lane, program order).  cpp_get_entities shifts by the padding offset, __padding_walls adds bricks.
    const uint16_t brick = (uint16_t)(T.icon(1, 0, 0) + 1);      // self.items["block"]["brick"][0]
    uint16_t *g = p.grid + ew * MD * MD;
    for (int y = 0; y < MD; ++y)
        for (int x = 0; x < MD; ++x) {
            const int lx = x - off, ly = y - off;
            g[y * MD + x] = (lx >= 0 && ly >= 0 && lx < D && ly < D) ? (uint16_t)0 : brick;
        }
    Draft<NW> d(level_goals);
    if constexpr (KIND == 0) xw_gen_nav(p, T, L, s, B, g, e, level_blocks, d);
    else xw_gen_walls(p, T, L, s, B, g, level_blocks, d);

    int kindv[2] = {TASK_TARGET, TASK_TARGET}, tfv[2] = {-1, -1}, st0v[2] = {STAGE_NAV, STAGE_NAV};
    xw_schedule_groups<NW, GM>(p, e, ep, ew, s, B, L, g, d, kindv, tfv, st0v);
    xw_commit(p, B, L, d, g, ew, GM == 0);                // (GM != 0: the 2-D idle stage wrote goal_cells from the final map)
    p.task_state[ew] = pack_task(tfv[0], st0v[0], EV_NONE, kindv[0]);
    if (GM == 2) { p.task_state2[ew] = pack_task(tfv[1], st0v[1], EV_NONE, kindv[1]); if (!p.shadow) p.task_steps2[e] = 0; }
    if (p.shadow) return;                                 // a pre-generated episode: installed later (xw_step_kernel / the list render)
    p.task_steps[e] = 0;
    p.num_steps[e] = 0;
    p.fresh[e] = 2;                                       // render: init_screen (zero the older context frames)
    atomicAdd(p.perf + 36, 1ull);                         // games reset
    if (!keep_done) p.done[e] = (uint8_t)done_code(step_rule(p), 0, EV_NONE);
}

template <int NW, int KIND, int GM>
__global__ __launch_bounds__(64) void xw_reset_kernel(XwParams p, int mode, int keep_done, const int32_t *count_now) {
    extern __shared__ uint32_t lds32[];
    // a handful of latency-bound wavefronts that run beside render_all's 16 waves per CU
    __builtin_amdgcn_s_setprio(3);
    // Envs per wavefront: map generation is data-dependent serial code and a wavefront runs the union of its lanes' paths,
    // so the list is spread as thinly as the grid allows -- one env per wavefront for the usual fraction of a percent of
    // the batch (C4 loop: 64 / 16 / 4 / 1 envs per wavefront = 0.1346 / 0.1296 / 0.1264 / 0.1243 ms per step), more lanes
    // per wavefront when many envs finish together (fixed-length episodes), 64 when the whole batch is reset.
    const int total = mode == MODE_RESET_ALL ? p.n : *count_now;
    int per_wave = (total + (int)gridDim.x - 1) / (int)gridDim.x;
    per_wave = per_wave < 1 ? 1 : (per_wave > 64 ? 64 : per_wave);
    if ((int)blockIdx.x * per_wave < total) {                          // else: whole wavefront idle
        LaneLds L;
        // name -> icon-variant tables staged in LDS once per wavefront: every lookup afterwards is an LDS read
        // instead of a dependent chain of global loads queued behind render_all's write stream
        int16_t *t_first = reinterpret_cast<int16_t *>(L.carve(lds32, true, xw_board_cells(p)));
        int16_t *t_var = t_first + ((p.name_first_len + 1) & ~1);
        for (int k = threadIdx.x; k < p.name_first_len; k += 64) t_first[k] = p.name_first[k];
        for (int k = threadIdx.x; k < p.name_variants_len; k += 64) t_var[k] = p.name_variants[k];
        __syncthreads();
        IconTables T;
        for (int t = 0; t < 3; ++t) T.first[t] = t_first + p.name_first_off[t];
        T.variants = t_var;
        // One env per wavefront (the usual case): 63 lanes would idle while one walks the serial map generation, a large
        // part of whose instructions are Philox rounds.  The blocks of a counter-based stream are independent: every lane
        // computes one block of this env's reset stream up front, the serial lane then reads its draws from LDS.
        const bool solo = per_wave == 1;
        uint4 *s_pre = reinterpret_cast<uint4 *>((reinterpret_cast<uintptr_t>(t_var + p.name_variants_len) + 15) & ~(uintptr_t)15);
        // the grid is capped (a short list should not cost the dispatch of one workgroup per env of the batch): loop
        for (int base = blockIdx.x * per_wave; base < total; base += gridDim.x * per_wave) {
            const int i = base + (solo ? 0 : (int)threadIdx.x);
            const bool mine = (solo ? threadIdx.x == 0 : (int)threadIdx.x < per_wave) && i < total;
            const int e = i < total ? (mode == MODE_RESET_ALL ? i : p.done_list[i]) : 0;
            if (solo) {
                const uint32_t ep = (p.shadow && mode != MODE_RESET_ALL ? p.sh_ep[e] : p.episode[e]) + 1;   // (lane 0 bumps it below; read before that)
                __builtin_amdgcn_wave_barrier();
                s_pre[threadIdx.x] = philox4x32_10(threadIdx.x, ep, 0u, 0u, p.seed, p.env_gid0 + (uint32_t)e);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
            if (mine) xw_reset_env<NW, KIND, GM>(p, T, L, e, keep_done != 0, solo ? s_pre : nullptr, solo ? 64u : 0u, mode == MODE_RESET_ALL);
            if (solo) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    }
    // (The epoch that tells the other queue's list render "every env of this launch is regenerated" is published by a
    // one-thread kernel queued behind this one.  Publishing it from here -- a release fence per writing wavefront, the last
    // one through stores the epoch -- saves that kernel's 5 us but the L2 write-backs cost the render running beside it 6 %:
    // 0.122 -> 0.127 ms per step on C4.)
}

// ---- exclusive scheduling of two task groups: an idle XWorld3DNav* group picked in mid-episode (teacher.cpp:209-220) ----
// TaskGroup::run_stage (teaching_task.cpp:204-222) for the envs the step kernel listed: draw a task, run its idle stage on the
// env's CURRENT map -- the board is rebuilt from the grid row, the goal slots from goal_cells (entity order) --, write the
// rearranged map back.  Decisions: the successive words of stream 5 | num_steps << 8 of the episode ("xwb-taskgen-v1").
// One env per wavefront (lane 0): the list holds a handful of envs per step at most.
template <int NW>
__device__ void xw_idle3d_env(const XwParams &p, const LaneLds &L, int e) {
    const Board<NW> B(p.curriculum != 0 ? 3 + p.cur_level[e] : p.dim, p.max_dim);
    const int MD = B.MD, D = B.D;
    const int G3 = p.group2d ? 1 : 0;                      // conf index of the XWorld3DNav* group
    uint16_t *g = p.grid + (size_t)e * MD * MD;
    Draft<NW> d(0);
    const int axy = p.agent_xy[e];
    d.agent_cell = B.cell_at(axy & 0xffff, axy >> 16);
    d.agent_icon = (int)(g[(axy >> 16) * MD + (axy & 0xffff)] & CELL_ICON_MASK) - 1;
    for (int c = 0; c < D * D; ++c)
        if (c != d.agent_cell && (g[B.grid_index(c)] & CELL_ICON_MASK)) d.occupied.set(c);
    const uint8_t *gc = p.goal_cells + (size_t)e * XW_MAX_GOALS;
    for (int i = 0; i < XW_MAX_GOALS; ++i) {
        const int mc = gc[i];
        if (xw_goal_slot_empty(gc, i, MD, g, p.icon_type)) break;
        const int icon = (int)(g[mc] & CELL_ICON_MASK) - 1;
        if (icon < 0) break;                               // (cannot happen: the table lists cells that hold goals)
        L.gcell[L.at(i)] = (uint8_t)B.cell_at(mc % MD, mc / MD);
        L.gicon[L.at(i)] = (uint16_t)icon;
        L.gname[L.at(i)] = (uint16_t)p.icon_name[icon];
        d.ng++;
    }
    Stream s;
    s.init(p.seed, p.env_gid0 + (uint32_t)e, p.episode[e], 5u | ((uint32_t)p.num_steps[e] << 8));
    const int tsel = G3 ? sample_task<1>(p, s, e) : sample_task<0>(p, s, e);
    const int kind = G3 ? task_at<1>(p, tsel) : task_at<0>(p, tsel);
    int tf = -1;
    xw_idle_stage_3d<NW, true>(p, e, s, B, L, g, d, kind, tf);
    xw_commit(p, B, L, d, g, (size_t)e, true);
    (G3 ? p.task_state2 : p.task_state)[e] = pack_task(tf, STAGE_NAV, EV_NONE, kind);
    (G3 ? p.task_steps2 : p.task_steps)[e] = 0;
    // the step that picked the group may also have ended the game (FLAGS_max_steps): its terminal frame shows the new map
    if (!p.visible_radius && p.term_flag[e]) {
        uint16_t *t = p.term_grid + (size_t)e * MD * MD;
        for (int k = 0; k < MD * MD; ++k) t[k] = g[k];
    }
}

template <int NW>
__global__ __launch_bounds__(64) void xw_idle3d_kernel(XwParams p, const int32_t *count_now) {
    extern __shared__ uint32_t lds32[];
    const int total = *count_now;
    if ((int)blockIdx.x >= total) return;
    LaneLds L;
    L.carve(lds32, false, xw_board_cells(p));
    for (int i = blockIdx.x; i < total; i += gridDim.x)
        if (threadIdx.x == 0) xw_idle3d_env<NW>(p, L, p.idle_list[i]);
}

// NW by the largest board of the batch: f(std::integral_constant<int, NW>)
template <typename F>
static void xw_dispatch_nw(int cells, F f) {
    if (cells <= 64) f(std::integral_constant<int, 1>());
    else if (cells <= 128) f(std::integral_constant<int, 2>());
    else f(std::integral_constant<int, 4>());
}

hipError_t launch_xw_idle3d(const XwParams &p, hipStream_t s) {
    const int cells = xw_board_cells(p);
    const size_t lds = LaneLds::bytes(false, cells);
    dim3 grid(p.n < 256 ? p.n : 256);
    const int32_t *cnt = p.idle_count;
    xw_dispatch_nw(cells, [&](auto nw) { hipLaunchKernelGGL((xw_idle3d_kernel<decltype(nw)::value>), grid, dim3(64), lds, s, p, cnt); });
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    // egocentric: the goal slots of those envs were re-ordered (poses travel with their goals): their images are redrawn
    // slot by slot, which also drops the envs' cached goal cells
    if (p.visible_radius) {
        XwParams q = p;
        q.done_list = p.idle_list; q.done_count = p.idle_count;
        return launch_xw_warp_goals(q, true, s);
    }
    return hipSuccess;
}

template <int NW>
static void launch_reset_nw(const XwParams &p, int mode, dim3 grid, size_t lds, hipStream_t s) {
    const int32_t *cnt = p.done_count;
    const int gm = p.n_tasks2 > 0 ? 2 : (p.group2d ? 1 : 0);
#define XW_RESET_LAUNCH(KINDV, GMV) hipLaunchKernelGGL((xw_reset_kernel<NW, KINDV, GMV>), grid, dim3(64), lds, s, p, mode, p.auto_reset, cnt)
    if (p.map_kind == 0) { if (gm == 0) XW_RESET_LAUNCH(0, 0); else if (gm == 1) XW_RESET_LAUNCH(0, 1); else XW_RESET_LAUNCH(0, 2); }
    else { if (gm == 0) XW_RESET_LAUNCH(1, 0); else if (gm == 1) XW_RESET_LAUNCH(1, 1); else XW_RESET_LAUNCH(1, 2); }
#undef XW_RESET_LAUNCH
}

hipError_t launch_xw_reset(const XwParams &p, int mode, hipStream_t s) {
    // n / 64 wavefronts in every mode (at least 256 for small batches): the whole batch = 64 envs per wavefront, a short
    // list = one env per wavefront, and the kernel fills the lanes in between as the list grows.  Whole C4 batch
    // finishing together every 8th step (tools/mass_reset.py): 0.183 ms per step with this grid, 0.323 with 2048
    // wavefronts, 0.458 with one per env -- there the machine is throughput-bound and idle lanes cost.
    const int all = (p.n + 63) / 64;
    const int want = all > 256 ? all : (p.n < 256 ? p.n : 256);
    dim3 grid(mode == MODE_RESET_ALL ? all : want);
    const int cells = xw_board_cells(p);
    // behind the lane columns: the two icon tables, alignment slack, the pre-drawn Philox blocks
    const size_t lds = LaneLds::bytes(true, cells) + 2 * (size_t)(p.name_first_len + 2 + p.name_variants_len) + 32 + 64 * sizeof(uint4);
    if (lds > 65536) return hipErrorInvalidValue;
    xw_dispatch_nw(cells, [&](auto nw) { launch_reset_nw<decltype(nw)::value>(p, mode, grid, lds, s); });
    return hipGetLastError();
}

}  // namespace xwb
