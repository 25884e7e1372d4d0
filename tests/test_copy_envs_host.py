"""xwb_copy_envs without a device: the verb is declared, bound and exported, and BatchedSimulator.copy_envs checks its lists
before it touches the library."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_copy_envs_is_declared_and_exported():
    """include/xwb.h declares the verb and its flag, xworld_amd.lib binds it, the built library exports it under XWB_1"""
    from xworld_amd import build, lib
    with open(os.path.join(ROOT, "include", "xwb.h")) as f:
        header = f.read()
    assert "enum { XWB_COPY_KEEP_RNG = 1 };" in header
    assert re.search(r"int xwb_copy_envs\(xwb_sim \*dst, const int32_t \*dst_envs_dev, xwb_sim \*src, const int32_t \*src_envs_dev, "
                     r"int32_t n, int32_t flags,\s+void \*stream\);", header)
    assert re.search(r"#define XWB_ABI_VERSION\s+%d\b" % lib.XWB_ABI_VERSION, header)
    assert "xwb_copy_envs" in lib.EXPORTED_SYMBOLS and lib.XWB_COPY_KEEP_RNG == 1
    sig = [s for s in lib._SIGS if s[0] == "xwb_copy_envs"][0]
    assert len(sig[2]) == 7
    out = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    node = {line.split()[-1].split("@")[0]: line.split()[-1].split("@")[-1] for line in out.splitlines() if line.strip()}
    assert node.get("xwb_copy_envs") == "XWB_1", node.get("xwb_copy_envs")


def _bare(n=8):
    """a BatchedSimulator without a library handle: whatever reaches the library fails on it"""
    from xworld_amd.batched import BatchedSimulator
    sim = object.__new__(BatchedSimulator)
    sim.h = None
    sim.L = None
    sim.num_envs, sim.device = n, 0
    return sim


def test_python_checks_the_lists_before_it_touches_the_library():
    import numpy as np
    import torch
    sim = _bare()
    with pytest.raises(ValueError, match="3 destination envs for 2 source envs"):
        sim.copy_envs([0, 1, 2], [3, 4])
    with pytest.raises(ValueError, match="3 destination envs for 0 source envs"):
        sim.copy_envs(np.arange(3), torch.zeros(0, dtype=torch.int64))
    for bad in ([0.5, 1.0], np.zeros((2, 2), np.int32), [True, False]):
        with pytest.raises(ValueError, match="dst_envs"):
            sim.copy_envs(bad, [0, 1])
        with pytest.raises(ValueError, match="src_envs"):
            sim.copy_envs([0, 1], bad)
    with pytest.raises(ValueError, match="source"):
        sim.copy_envs([0], [1], source="another batch")
