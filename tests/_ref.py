"""ctypes bindings for oracle/_ref/libxwref.so: the reference's OWN SimpleGame / SimpleRace sources, compiled unmodified
against the stand-in headers of oracle/ref_standins/ (`make -C oracle ref REFERENCE=<tree>`; __graft_entry__.build() runs it
where the reference tree is present).

TEST INFRASTRUCTURE ONLY.  The library exists only where the reference tree was at hand when it was built; tests that need
it call require(): a missing library is a failure where the tree is present and a skip, with its reason, where it is not.
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "oracle", "_ref", "libxwref.so")
REFERENCE = os.environ.get("XWB_REFERENCE", "/root/reference")

GAME, RACE = 0, 1
_lib = None


def have_tree():
    return os.path.isfile(os.path.join(REFERENCE, "games", "simple_race", "simple_race_simulator.cpp"))


def have_lib():
    return os.path.isfile(LIB_PATH)


def require():
    """The loaded library; pytest.fail where it should exist, pytest.skip where it cannot."""
    import pytest
    if not have_lib():
        if have_tree():
            pytest.fail("oracle/_ref/libxwref.so is missing although the reference tree is at %s: run "
                        "__graft_entry__.build() (make -C oracle ref)" % REFERENCE)
        pytest.skip("no oracle/_ref/libxwref.so and no reference tree (%s) to build it from: the live comparison with the "
                    "reference's own code cannot run here; the recorded fixtures still do" % REFERENCE)
    return lib()


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)

    sig("xwref_set_common_flags", None, C.c_int, C.c_int, C.c_int)
    sig("xwref_set_game_flags", None, C.c_int)
    sig("xwref_set_race_flags", None, C.c_char_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_char_p, C.c_double)
    sig("xwref_threads", C.c_int)
    sig("xwref_burn_threads", None, C.c_int)
    sig("xwref_create", vp, C.c_int)
    sig("xwref_destroy", None, vp)
    sig("xwref_reset_game", None, vp)
    sig("xwref_take_actions", C.c_float, vp, C.c_int, C.c_int)
    sig("xwref_game_over", C.c_int, vp)
    sig("xwref_get_num_actions", C.c_int, vp)
    sig("xwref_get_lives", C.c_int, vp)
    sig("xwref_get_num_steps", C.c_longlong, vp)
    sig("xwref_get_screen", C.c_int, vp, vp)
    sig("xwref_get_state_screen", C.c_int, vp, vp)
    sig("xwref_get_car", None, vp, C.POINTER(C.c_float))
    sig("xwref_rollout", C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp)
    _lib = L
    return L


RACE_DEFAULTS = dict(track_type="straight", track_width=20.0, track_length=100.0, track_radius=30.0, race_full_manouver=False,
                     random=False, difficulty="easy", reward_scale=1.0, context=1, max_steps=0, simulator_seed=0)


def set_flags(game, flags):
    """The gflags of one env: they are process-wide, like the reference's, so set them right before the env is made."""
    L = lib()
    if game == RACE:
        f = dict(RACE_DEFAULTS, **flags)
        L.xwref_set_race_flags(f["track_type"].encode(), f["track_width"], f["track_length"], f["track_radius"],
                               int(f["race_full_manouver"]), int(f["random"]), f["difficulty"].encode(), f["reward_scale"])
    else:
        f = dict(dict(context=1, max_steps=0, simulator_seed=0), **flags)
        L.xwref_set_game_flags(int(f["array_size"]))
    L.xwref_set_common_flags(int(f["context"]), int(f["max_steps"]), int(f["simulator_seed"]))
    return f


class Record:
    """One env's run of the example loop (ref_api.cpp xwref_rollout): T steps; obs / cars / resets hold T + 1 records taken
    before each step (after the reset of a finished game), obs_after / cars_after T records taken right after each step."""
    __slots__ = ("actions", "rewards", "codes", "num_steps", "obs", "obs_after", "cars", "cars_after", "resets", "ctor_car",
                 "n_actions", "nth_thread")

    def reward_bits(self):
        return self.rewards.view(np.uint32)


def rollout(game, flags, actions):
    """Run `actions` through a reference env on a fresh thread.  With simulator_seed != 0 that thread is the reference's
    nth_thread-th (returned in the record)."""
    L = lib()
    f = set_flags(game, flags)
    T = len(actions)
    r = Record()
    r.actions = np.ascontiguousarray(actions, np.int32)
    r.rewards = np.zeros(T, np.float32)
    r.codes = np.zeros(T, np.uint8)
    r.num_steps = np.zeros(T, np.int32)
    if game == RACE:
        r.obs = np.zeros((T + 1, 4 * f["context"]), np.float32)
        r.cars = np.zeros((T + 1, 3), np.float32)
        r.cars_after = np.zeros((T, 3), np.float32)
        r.ctor_car = np.zeros(3, np.float32)
    else:
        r.obs = np.zeros((T + 1, f["array_size"] * f["context"]), np.uint8)
        r.cars = r.cars_after = r.ctor_car = None
    r.obs_after = np.zeros((T,) + r.obs.shape[1:], r.obs.dtype)
    r.resets = np.zeros(T + 1, np.uint8)
    r.nth_thread = L.xwref_threads() + 1 if f["simulator_seed"] else 0
    p = lambda a: None if a is None else a.ctypes.data
    r.n_actions = L.xwref_rollout(game, T, p(r.actions), p(r.rewards), p(r.codes), p(r.num_steps), p(r.obs), p(r.obs_after),
                                  r.obs.strides[0], p(r.cars), p(r.cars_after), p(r.resets), p(r.ctor_car))
    return r
