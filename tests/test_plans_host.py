"""xwb_xw_evaluate_plans on the host side: the symbol is declared, exported, listed and typed; the float32 return recurrence the
header states; and the oracle's side of tests/test_gpu_plans.py -- the cases' seeded plan sets driven through the oracle alone,
where the seeds are chosen: every case must reach each way a plan can end (tests/_plans_cases.py required)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _plans_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "xwb_xw_evaluate_plans"


def _header():
    with open(os.path.join(ROOT, "include", "xwb.h")) as f:
        return f.read()


def test_symbol_is_declared_exported_and_typed():
    from xworld_amd import lib
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, text)
    assert m, "include/xwb.h does not declare " + NAME
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["xwb_sim *sim", "const int32_t *envs_dev", "int32_t n", "const int8_t *plans_dev", "int32_t n_plans",
                      "int32_t horizon", "int32_t act_rep", "float gamma", "float *return_dev", "int32_t *steps_dev",
                      "uint8_t *code_dev", "int32_t *last_dev", "void *stream"], params
    assert NAME in lib.EXPORTED_SYMBOLS
    sig = dict((s[0], s[1:]) for s in lib._SIGS)[NAME]
    vp = C.c_void_p
    assert sig == (C.c_int, [vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, C.c_int32, C.c_float, vp, vp, vp, vp, vp])
    # the version script exports the name: node XWB_1 takes every xwb_* symbol, and the name is not in the testing node
    with open(os.path.join(ROOT, "xworld_amd", "csrc", "libxwb.map")) as f:
        script = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    nodes = dict(re.findall(r"(\w+)\s*\{(.*?)\}\s*;", script, flags=re.S))
    assert re.search(r"global:[^;]*\bxwb_\*", nodes["XWB_1"]) and NAME not in nodes["XWB_TESTING"]
    from xworld_amd import build
    assert "kernels_xworld_plans.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "kernels_xworld_plans.hip")) and os.path.exists(os.path.join(build.CSRC, "xw_step_rule.h"))


def test_abi_version_matches_the_binding():
    from xworld_amd import lib
    m = re.search(r"#define\s+XWB_ABI_VERSION\s+(\d+)", _header())
    assert m and int(m.group(1)) == lib.XWB_ABI_VERSION


def test_the_method_exists():
    import inspect
    from xworld_amd.batched import BatchedSimulator
    sig = inspect.signature(BatchedSimulator.evaluate_plans)
    assert list(sig.parameters) == ["self", "plans", "gamma", "act_rep", "envs", "last", "out", "stream"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["gamma"], d["act_rep"], d["envs"], d["last"], d["out"], d["stream"]) == (1.0, 1, None, False, None, None)


def test_return_recurrence_by_hand():
    f = np.float32
    # three time penalties and the right goal: r = (float)(-0.01), (float)(-0.01 + 1.0)
    pen, win = f(-0.01), f(-0.01 + 1.0)
    # gamma 1: plain float32 sums, left to right
    want = f(f(f(f(0) + pen) + pen) + pen)
    want = f(want + win)
    assert pc.returns_f32([pen, pen, pen, win], 1.0).tobytes() == want.tobytes()
    # gamma 0.5: the powers of two are exact, so ret = pen + pen/2 + pen/4 + win/8 with one rounding per sum
    want = f(f(f(pen + f(pen * f(0.5))) + f(pen * f(0.25))) + f(win * f(0.125)))
    assert pc.returns_f32([pen, pen, pen, win], 0.5).tobytes() == want.tobytes()
    # a gamma whose powers round: g is the ROUNDED product chain (0.9f * 0.9f rounded, times 0.9f, ...), not 0.9 ** t
    g1 = f(0.9)
    g2 = f(g1 * g1)
    want = f(f(f(0) + f(f(1) * f(1))) + f(g1 * f(1)))
    want = f(want + f(g2 * f(1)))
    assert pc.returns_f32([1, 1, 1], 0.9).tobytes() == want.tobytes()
    assert pc.returns_f32([], 0.5) == 0 and pc.returns_f32([f(-1.01)], 0.5) == f(-1.01)
    # the sum is not the float64 sum rounded once: ten penalties differ in the last bits
    ten = pc.returns_f32([pen] * 10, 1.0)
    assert ten.tobytes() != f(10 * -0.01).tobytes()


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_seeds_reach_every_ending(oracle, name):
    """the coverage condition of the GPU comparison, established with the oracle alone"""
    rec, steps, codes, last, rewards = pc.expected(name)
    got, need = pc.coverage(name), pc.required(name)
    assert need <= got, (name, "missing", need - got)
    # the shape of the answer: a plan stops with the step that set its code; an alive one ran H steps
    c = pc.CASES[name]
    cells = c["cfg"]["max_dim"] ** 2
    for e in range(pc.N):
        for k in range(pc.K):
            assert 1 <= steps[e, k] <= pc.H and (codes[e, k] != 0 or steps[e, k] == pc.H)
            assert 0 <= (last[e, k] & 0xffff) < cells and (last[e, k] >> 16) in ((0, 1, 2, 3) if pc.num_actions(name) == 6 else (0,))
    assert all(len(s) <= c["prefix"] for s in rec.since)
