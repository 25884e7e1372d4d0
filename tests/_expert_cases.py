"""The configurations the expert's tests run, as (options of the batch, the oracle's cfg, palette subtrees): shared by
tests/test_expert_ref.py (checker against oracle, CPU) and tests/test_gpu_expert.py (kernel against checker)."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "xworld_amd", "confs")
NAV, WALLS, NAV2D = (os.path.join(CONF, f) for f in ("nav_target.json", "walls_target.json", "navigation2d.json"))
T3 = ["XWorld3DNavTarget", "XWorld3DNavTargetNear", "XWorld3DNavTargetBetween", "XWorld3DNavTargetDirection", "XWorld3DNavTargetAvoid"]
T2 = ["XWorldNavTarget", "XWorldNavNear", "XWorldNavColorTarget", "XWorldNavBetween"]
SEED, GID0 = 77, 13


def _case(conf, popts, ocfg, tasks, walls=False, **both):
    o = {"xwd_conf_path": conf, "task_mode": "lang_acquisition", "tasks": list(tasks)}
    o.update(popts)
    c = dict(ocfg)
    c.update(seed=SEED, tasks=list(tasks))
    for k, v in both.items():
        o[k] = v
        c[k] = v
    return o, c, walls


_N7 = ({"max_dim": 7, "num_blocks": 16}, dict(map_kind=0, max_dim=7, dim=7, num_goals=4, num_blocks=16))
_N8 = ({}, dict(map_kind=0, max_dim=8, dim=8, num_goals=4, num_blocks=16))
_TWO = {"max_dim": 7, "num_blocks": 6, "tasks2": T2}
_O2 = dict(map_kind=0, max_dim=7, dim=7, num_goals=4, num_blocks=6, tasks2=T2)

CASES = {
    "nav7_one": _case(NAV, *_N7, T3[2:3]),        # (Target alone: 71 % of the episodes have no path -- see docs/measurements.md)
    "nav8_five": _case(NAV, *_N8, T3),
    "walls7": _case(WALLS, {}, dict(map_kind=1, max_dim=7, dim=7, num_goals=12, num_blocks=12), T3, walls=True),
    "nav8_dim5": _case(NAV, {"dim": 5, "num_goals": 2, "num_blocks": 6}, dict(map_kind=0, max_dim=8, dim=5, num_goals=2, num_blocks=6), T3[1:4]),
    "ego3": _case(NAV, *_N7, T3, visible_radius=3),
    "ego5": _case(NAV, *_N8, T3, visible_radius=5),
    # boards of four words (max_dim > 8): 11 (odd pitch), 12 egocentric (padded pitch), 16 (padded; "is a goal" by icon type)
    "nav11": _case(NAV, {"max_dim": 11, "num_blocks": 30}, dict(map_kind=0, max_dim=11, dim=11, num_goals=4, num_blocks=30), T3),
    "ego12": _case(NAV, {"max_dim": 12, "num_blocks": 36}, dict(map_kind=0, max_dim=12, dim=12, num_goals=4, num_blocks=36), T3, visible_radius=3),
    "ego15": _case(NAV, {"max_dim": 15, "num_blocks": 50}, dict(map_kind=0, max_dim=15, dim=15, num_goals=4, num_blocks=50), T3, visible_radius=5),
    "nav16": _case(NAV, {"max_dim": 16, "num_blocks": 40}, dict(map_kind=0, max_dim=16, dim=16, num_goals=4, num_blocks=40), T3),
    "two_groups": _case(NAV2D, _TWO, dict(_O2), T3),
    "two_exclusive": _case(NAV2D, dict(_TWO, task_mode="one_channel", task_groups_exclusive=True, task_group_weights=[50, 1]),
                           dict(_O2, task_mode=1, task_groups_exclusive=1, group_weights=[50, 1]), T3, max_steps=45),
    "curriculum": _case(NAV2D, {}, dict(_N8[1]), T3, curriculum=0.1),
}
TWO_GROUPS = ("two_groups", "two_exclusive")


def make_oracle_cfg(name):
    return dict(CASES[name][1])


def palette(oracle, name):
    return oracle.Palette(oracle.WALLS_SUBTREES if CASES[name][2] else oracle.NAV_SUBTREES)


def make_sim(name, n, policy_seed=5, **extra):
    from xworld_amd.batched import BatchedSimulator
    o = dict(CASES[name][0])
    o.update(extra)
    return BatchedSimulator("xworld", o, num_envs=n, seed=SEED, policy_seed=policy_seed, env_gid0=GID0)


CURRICULUM_ITERS = 20000          # expert-driven iterations after which every one of 32 envs has reached level >= 2 (CPU run)
