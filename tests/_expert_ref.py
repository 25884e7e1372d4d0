"""A plain-Python restatement of the shortest-path expert's contract (include/xwb.h, xwb_xw_expert): the step rule of an
XWorld3DNav* task in its navigation stage as ONE forward transition function, and searches over the node graph it defines.
It shares no code with the kernel; tests/test_expert_ref.py pins it to hand-worked maps, to the reference's own bfs and to the
oracle's step rule, tests/test_gpu_expert.py compares the kernel with it.

Coordinates are (x, y), y growing downwards; headings 0 +x, 1 +y, 2 -x, 3 -y (full observation: always 1)."""
import math
from collections import deque

import numpy as np

TARGET, NEAR, BETWEEN, DIRECTION, AVOID = range(5)
FRONT, BEHIND, LEFT, RIGHT = 1, 2, 3, 4
DX = (1, 0, -1, 0)
DY = (0, 1, 0, -1)
WIN, LOSE = "win", "lose"
NO_PATH = -1


class State:
    """What the next step reads of one env.  occupied / is_goal / is_target: [D, D] arrays indexed [y, x]; the agent's own cell
    is NOT occupied.  between: the middle cell (x, y) or None; direction: (referent x, referent y, word) or None."""

    def __init__(self, occupied, is_goal, is_target, agent, heading=1, ego=False, kind=TARGET, between=None, direction=None,
                 active=True):
        self.occ = np.asarray(occupied, bool)
        self.goal = np.asarray(is_goal, bool)
        self.tgt = np.asarray(is_target, bool)
        self.D = self.occ.shape[0]
        self.agent = (int(agent[0]), int(agent[1]))
        self.ego = bool(ego)
        self.heading = int(heading) if ego else 1
        self.kind = kind
        self.between = tuple(between) if between is not None and between[0] >= 0 else None
        self.direction = tuple(direction) if direction is not None and direction[0] >= 0 else None
        self.active = active            # the group is in its navigation stage and the env is not finished
        assert not self.occ[self.agent[1], self.agent[0]]

    @property
    def n_actions(self):
        return 6 if self.ego else 4

    @property
    def headings(self):
        return (0, 1, 2, 3) if self.ego else (1,)


def _direction_word(h, v2x, v2y):
    vx, vy = DX[h], DY[h]
    cs, sn = vx * v2x + vy * v2y, vy * v2x - vx * v2y
    return FRONT if cs > 0 else (BEHIND if cs < 0 else (RIGHT if sn > 0 else LEFT))


def _good_goal(st, gx, gy, h):
    if st.kind == BETWEEN:
        return False
    if st.kind == DIRECTION and st.direction is not None:
        rx, ry, word = st.direction
        v2x, v2y = rx - gx, ry - gy
        return v2x * v2x + v2y * v2y == 1 and _direction_word(h, v2x, v2y) == word
    return bool(st.tgt[gy, gx])


def transition(st, x, y, h, a):
    """One xwb_step (act_rep 1) with the agent on (x, y), heading h: WIN ("correct_goal"), LOSE ("wrong_goal") or the node
    (x, y, h) the call leaves."""
    move = None
    if st.ego:
        if a == 4:
            h = (h + 3) & 3
        elif a == 5:
            h = (h + 1) & 3
        else:
            move = (h, (h + 2) & 3, (h + 3) & 3, (h + 1) & 3)[a]     # forward, backward, left, right of the heading
    else:
        move = (3, 1, 2, 0)[a]                                        # MOVE_UP, MOVE_DOWN, MOVE_LEFT, MOVE_RIGHT
    hit = None
    if move is not None:
        tx, ty = x + DX[move], y + DY[move]
        if 0 <= tx < st.D and 0 <= ty < st.D:
            if st.occ[ty, tx]:
                hit = (tx, ty)
            else:
                x, y = tx, ty
    if hit is not None and move == h and st.goal[hit[1], hit[0]]:
        return WIN if _good_goal(st, hit[0], hit[1], h) else LOSE
    if st.kind == BETWEEN and st.between == (x, y):
        return WIN
    return (x, y, h)


def forward_dist(st, start=None):
    """Breadth-first search forward from one node: (dist, sorted optimal first actions); (NO_PATH, []) when nothing wins."""
    if not st.active:
        return NO_PATH, []
    start = start or (st.agent[0], st.agent[1], st.heading)
    best, firsts = None, set()
    seen = {start: 0}
    queue = deque([(start, None)])
    origin = {start: set()}              # the first actions of the shortest paths that reach a node
    while queue:
        node, _ = queue.popleft()
        d = seen[node]
        if best is not None and d + 1 > best:
            break
        for a in range(st.n_actions):
            r = transition(st, node[0], node[1], node[2], a)
            first = {a} if node == start else origin[node]
            if r == WIN:
                if best is None:
                    best = d + 1
                if d + 1 == best:
                    firsts |= first
            elif r != LOSE and r != node:
                if r not in seen:
                    seen[r] = d + 1
                    origin[r] = set(first)
                    queue.append((r, None))
                elif seen[r] == d + 1:
                    origin[r] |= first
    return (best, sorted(firsts)) if best is not None else (NO_PATH, [])


def _graph(st):
    """Every node an agent could stand on: its successors under `transition`, and its distance by a search over the reversed
    edges from the nodes that win at once."""
    D = st.D
    dist, rev, succ = {}, {}, {}
    level = deque()
    for nd in [(x, y, h) for h in st.headings for y in range(D) for x in range(D) if not st.occ[y, x]]:
        out = [transition(st, nd[0], nd[1], nd[2], a) for a in range(st.n_actions)]
        succ[nd] = out
        if WIN in out:
            dist[nd] = 1
            level.append(nd)
        for r in out:
            if r != WIN and r != LOSE and r != nd:
                rev.setdefault(r, []).append(nd)
    while level:
        nd = level.popleft()
        for pr in rev.get(nd, ()):
            if pr not in dist:
                dist[pr] = dist[nd] + 1
                level.append(pr)
    return dist, succ


def _firsts(dist, succ, node):
    d0 = dist.get(node, NO_PATH)
    if d0 == 1:
        return [a for a, r in enumerate(succ[node]) if r == WIN]
    if d0 > 1:
        return [a for a, r in enumerate(succ[node]) if r not in (WIN, LOSE) and r != node and dist.get(r) == d0 - 1]
    return []


def solve(st, want_field=False):
    """(dist, sorted optimal first actions[, field]); field: uint16 [headings, D * D], 0xFFFF = none."""
    hs = st.headings
    field = np.full((len(hs), st.D * st.D), 0xFFFF, np.uint16)
    if not st.active:
        return (NO_PATH, [], field) if want_field else (NO_PATH, [])
    dist, succ = _graph(st)
    start = (st.agent[0], st.agent[1], st.heading)
    d0, firsts = dist.get(start, NO_PATH), _firsts(dist, succ, start)
    if not want_field:
        return d0, firsts
    for (x, y, h), d in dist.items():
        field[hs.index(h), y * st.D + x] = d
    return d0, firsts, field


def plan(st):
    """(dist, the action sequence that takes the lowest optimal action id at every node); (NO_PATH, []) without a path."""
    if not st.active:
        return NO_PATH, []
    dist, succ = _graph(st)
    node = (st.agent[0], st.agent[1], st.heading)
    d0 = dist.get(node, NO_PATH)
    acts = []
    while d0 != NO_PATH and len(acts) < d0:
        a = _firsts(dist, succ, node)[0]
        acts.append(a)
        node = succ[node][a]
    return d0, acts


def cell_distance(X, Y, obstacles, start, end):
    """Moves between two cells of an X x Y board, obstacles impassable, the end cell enterable: the question the reference's
    maze2d.bfs answers (its path's length), or None."""
    occ = np.zeros((max(X, Y), max(X, Y)), bool)
    occ[:] = True
    occ[:Y, :X] = False
    for (ox, oy) in obstacles:
        occ[oy, ox] = True
    occ[start[1], start[0]] = False
    occ[end[1], end[0]] = False
    none = np.zeros_like(occ)
    st = State(occ, none, none, start, kind=BETWEEN, between=end)
    if tuple(start) == tuple(end):
        return 0
    d, _ = forward_dist(st)
    return None if d == NO_PATH else d


def yaw_to_heading(yaw):
    return int(round(yaw / (math.pi / 2))) & 3


def state_from_oracle(ow, pal, two_groups=False):
    """The State of a tests/_oracle.XWorld object (its XWorld3DNav* group is group 0 when there are two)."""
    grid = ow.grid()
    D = grid.shape[0]
    ax, ay = ow.agent_xy()
    occ = grid != 0
    occ[ay, ax] = False
    is_goal = np.zeros((D, D), bool)
    nz = grid > 0
    is_goal[nz] = pal.type_arr[grid[nz] - 1] == 0
    ego = ow.cfg.visible_radius != 0
    if two_groups:
        kind, stage = ow.group_state(0)[:2]
    else:
        kind, stage = ow.task_kind(), ow.stage()
    active = stage == 1 and ow.game_over() == 0 and kind < 5
    return State(occ, is_goal, ow.target_cells().astype(bool) & is_goal, (ax, ay), yaw_to_heading(ow.agent_yaw()) if ego else 1, ego,
                 kind, ow.between_cell(), ow.direction_target(), active)


def state_from_env(sim, e, pal_types):
    """The same from the batch's own getters (env_grid raw codes, env_state)."""
    raw = sim.env_grid(e, raw=True).astype(np.int32)
    s = sim.env_state(e)
    D = raw.shape[0]
    icon = raw & 0x7fff
    occ = icon != 0
    occ[s.xw_agent_y, s.xw_agent_x] = False
    is_goal = np.zeros((D, D), bool)
    nz = icon > 0
    is_goal[nz] = pal_types[icon[nz] - 1] == 0
    kind, stage, target = s.xw_task, s.xw_stage, s.xw_target
    between = (target % D, target // D) if kind == BETWEEN and target >= 0 else None
    direction = ((target & 0xff) % D, (target & 0xff) // D, (target >> 8) & 7) if kind == DIRECTION and target >= 0 else None
    ego = sim.cfg.visible_radius != 0
    return State(occ, is_goal, (raw >> 15).astype(bool) & is_goal, (s.xw_agent_x, s.xw_agent_y), s.xw_agent_dir if ego else 1, ego, kind,
                 between, direction, stage == 1 and s.game_over == 0 and kind < 5)
