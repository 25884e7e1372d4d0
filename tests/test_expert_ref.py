"""The shortest-path expert's contract on the CPU: the plain-Python checker (tests/_expert_ref.py) against maps worked out by
hand, against the reference's own breadth-first search (tests/golden/expert_bfs.json) and against the oracle's step rule; and
the boundary (xwb_xw_expert in include/xwb.h and in the built library)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import _expert_cases as cases
import _expert_ref as ref
from _expert_ref import AVOID, BETWEEN, DIRECTION, TARGET, State

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _map(rows, **kw):
    """'.' empty, 'A' agent, '#' block, 'G' target goal, 'g' other goal, 'M' the Between middle cell (empty), 'R' referent goal"""
    D = len(rows)
    occ, goal, tgt = (np.zeros((D, D), bool) for _ in range(3))
    agent = None
    for y, row in enumerate(rows):
        assert len(row) == D
        for x, ch in enumerate(row):
            if ch == "A":
                agent = (x, y)
            elif ch == "M":
                kw["between"] = (x, y)
            elif ch != ".":
                occ[y, x] = True
                goal[y, x] = ch in "GgR"
                tgt[y, x] = ch == "G"
                if ch == "R":
                    kw["direction"] = (x, y, kw.pop("word"))
    return State(occ, goal, tgt, agent, **kw)


def _both(st):
    d, firsts = ref.solve(st)
    assert (d, firsts) == ref.forward_dist(st)
    return d, firsts


def test_target_below_the_agent():
    assert _both(_map(["...", ".A.", ".G."])) == (1, [1])


def test_target_in_the_top_row_is_unwinnable_under_full_observation():
    st = _map([".G.", "...", "A.."])
    assert _both(st) == (ref.NO_PATH, [])
    assert ref.cell_distance(3, 3, [], (0, 2), (1, 0)) == 3          # ... although the reference's _reachable says yes


def test_the_same_map_egocentric_turn_go_bump():
    # heading +y on (0, 2): two steps backwards to (0, 0) and one turn left (+y -> +x), in any order, then the bump: 4
    assert _both(_map([".G.", "...", "A.."], ego=True, heading=1)) == (4, [1, 4])
    st = _map([".G.", ".A.", "..."], ego=True, heading=3)
    assert _both(st) == (1, [0])
    assert _both(_map([".G.", ".A.", "..."], ego=True, heading=0)) == (2, [4])     # turn left from +x faces -y


def test_between_detours_round_a_goal_ahead():
    # the middle cell lies two cells below, a goal in between: MOVE_DOWN would bump it along the heading ("wrong_goal")
    st = _map(["#A#", "#g.", "#M."], kind=BETWEEN)
    assert _both(st) == (ref.NO_PATH, [])                             # walled in: the bump is no way through
    st = _map([".A.", ".g.", ".M."], kind=BETWEEN)
    d, firsts = _both(st)
    assert d == 4 and firsts == [2, 3]                                # sideways, down, down, back: never action 1 first
    assert ref.transition(st, 1, 0, 1, 1) == ref.LOSE


def test_between_standing_on_the_middle_cell():
    occ = np.zeros((3, 3), bool)
    st = State(occ, occ, occ, (0, 0), kind=BETWEEN, between=(0, 0))
    assert _both(st) == (1, [0, 2])                                   # a move off the map leaves the agent on it


def test_direction_heading_at_the_bump_decides():
    # goal g at (1, 1), referent R at (2, 1): seen from g with heading +y (vx, vy) = (0, 1), v2 = (1, 0): sn = 1 > 0 -> RIGHT
    rows = [".A.", ".gR", "..."]
    assert _both(_map(rows, kind=DIRECTION, word=ref.RIGHT)) == (1, [1])
    assert _both(_map(rows, kind=DIRECTION, word=ref.LEFT)) == (ref.NO_PATH, [])
    # egocentric, bumping g from below (heading -y): v2 = (1, 0), sn = -1 * 1 = -1 -> LEFT
    rows = ["...", ".gR", ".A."]
    assert _both(_map(rows, kind=DIRECTION, word=ref.LEFT, ego=True, heading=3)) == (1, [0])
    d, firsts = _both(_map(rows, kind=DIRECTION, word=ref.RIGHT, ego=True, heading=3))
    assert d > 1 and 0 not in firsts                                  # must go round and bump from above


def test_non_target_goal_ahead_is_not_bumped():
    st = _map([".A.", ".g.", ".G."], kind=AVOID)
    assert _both(st) == (ref.NO_PATH, [])                             # G can only be bumped from (1, 1), which g holds
    st = _map(["A..", "g..", "..G"], kind=TARGET)
    assert _both(st) == (4, [3])                                      # right, right, down, the bump: MOVE_DOWN first would end it
    assert ref.transition(st, 0, 0, 1, 1) == ref.LOSE
    st = _map(["A..", "g..", ".G."], kind=TARGET)
    assert _both(st) == (3, [3])


def test_field_matches_per_node_forward_search():
    rng = np.random.default_rng(3)
    for trial in range(40):
        D = int(rng.integers(3, 7))
        ego = bool(trial & 1)
        cells = rng.permutation(D * D)
        occ, goal, tgt = (np.zeros((D, D), bool) for _ in range(3))
        n_obj = int(rng.integers(2, D * D // 2))
        for i, c in enumerate(cells[1:1 + n_obj]):
            occ[c // D, c % D] = True
            goal[c // D, c % D] = i % 2 == 0
            tgt[c // D, c % D] = i % 4 == 0
        kind = (TARGET, BETWEEN, DIRECTION)[trial % 3]
        kw = {}
        free = [c for c in cells if not occ[c // D, c % D]]
        if kind == BETWEEN:
            kw["between"] = (int(free[-1] % D), int(free[-1] // D))
        if kind == DIRECTION:
            g = cells[1]
            kw["direction"] = (int(g % D), int(g // D), int(rng.integers(1, 5)))
        st = State(occ, goal, tgt, (int(cells[0] % D), int(cells[0] // D)), heading=int(rng.integers(0, 4)), ego=ego, kind=kind, **kw)
        d, firsts, field = ref.solve(st, want_field=True)
        assert (d, firsts) == ref.forward_dist(st)
        for hi, h in enumerate(st.headings):
            for c in range(D * D):
                x, y = c % D, c // D
                want = 0xFFFF if occ[y, x] else ref.forward_dist(st, (x, y, h))[0] & 0xFFFF
                assert field[hi, c] == want, (trial, h, x, y)
        assert field[st.headings.index(st.heading), st.agent[1] * D + st.agent[0]] == d & 0xFFFF


def test_cell_distance_equals_the_reference_bfs():
    with open(os.path.join(ROOT, "tests", "golden", "expert_bfs.json")) as f:
        gold = json.load(f)
    assert len(gold["boards"]) >= 200
    for b in gold["boards"]:
        got = ref.cell_distance(b["X"], b["Y"], [tuple(o) for o in b["obstacles"]], tuple(b["start"]), tuple(b["end"]))
        assert got == (None if b["length"] is None else b["length"] + 1), b        # bfs returns the cells between the two ends
    assert any(b["length"] is None for b in gold["boards"]) and any(b["length"] for b in gold["boards"])


@pytest.mark.parametrize("name", sorted(n for n in cases.CASES if n != "curriculum"))
def test_checker_and_oracle_close_the_loop(oracle, name):
    """Every env with a finite dist: the oracle, driven by the checker's lowest optimal action, records correct_goal at exactly
    step dist, -0.01 before and -0.01 + 1.0 then (one group: the reward bits).  At least half of the envs have a path."""
    n = 512
    pal = cases.palette(oracle, name)
    cfg = cases.make_oracle_cfg(name)
    two = name in cases.TWO_GROUPS
    finite = 0
    step_r, win_r = np.float32(np.float64(np.float32(0.0)) + -0.01), np.float32(np.float64(np.float32(0.0)) + (-0.01 + 1.0))
    ow = oracle.XWorld(pal, render=False, **cfg)
    for e in range(n):
        ow.reset_game(cases.GID0 + e, 0)
        st = ref.state_from_oracle(ow, pal, two_groups=two)
        d, acts = ref.plan(st)
        if d == ref.NO_PATH:
            continue
        finite += 1
        for k, a in enumerate(acts, 1):
            r = ow.take_actions(a)
            event = ow.group_state(0)[3] if two else ow.event()
            assert event == (1 if k == d else 0), (name, e, k, d)
            if not two:
                assert np.float32(r).view(np.uint32) == (win_r if k == d else step_r).view(np.uint32), (name, e, k)
                assert ow.game_over() == (4 if k == d else 0), (name, e, k)
    print("%s: %d of %d episodes start without a path (%.1f %%)" % (name, n - finite, n, 100.0 * (n - finite) / n))
    assert 2 * finite >= n, (name, finite)


def test_curriculum_is_climbed_on_the_cpu(oracle):
    """32 envs under the expert: every env reaches level >= 2 within the GPU test's iteration count."""
    name, n, iters = "curriculum", 32, cases.CURRICULUM_ITERS
    pal = cases.palette(oracle, name)
    cfg = cases.make_oracle_cfg(name)
    levels = []
    for e in range(n):
        ow = oracle.XWorld(pal, render=False, **cfg)
        episode, memo = 0, {}
        ow.reset_game(cases.GID0 + e, episode)
        for t in range(iters):
            if ow.game_over() != 0:
                episode += 1
                memo = {}
                ow.reset_game(cases.GID0 + e, episode)
            key = ow.agent_xy()                          # nothing but the agent moves within an episode: one search per cell
            if key not in memo:
                memo[key] = ref.solve(ref.state_from_oracle(ow, pal))[1]
            firsts = memo[key]
            ow.take_actions(firsts[0] if firsts else 0)
        levels.append(ow.curriculum_state()[0])
    assert min(levels) >= 2, levels


def test_boundary_declared_and_exported():
    with open(os.path.join(ROOT, "include", "xwb.h")) as f:
        header = f.read()
    assert re.search(r"int xwb_xw_expert\(xwb_sim \*sim, int32_t \*actions_dev, int32_t \*dist_dev, uint16_t \*field_dev,\s*"
                     r"int32_t no_path_action,\s*void \*stream\);", header)
    assert "int xwb_xw_expert_field_dims(const xwb_sim *sim, size_t *headings, size_t *cells);" in header
    assert "#define XWB_EXPERT_NO_PATH (-1)" in header
    from xworld_amd import build
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert {"xwb_xw_expert", "xwb_xw_expert_field_dims"} <= names
