"""CPU check of the host-testable piece that takes the exposed load waits out of k_render_pool's pass loop (DESIGN.md
§5.12, "Round 16"): ptc::sweep_mask_piped (pt_cull.h), the leaf sweep with several boxes' bounds in flight, against
ptc::sweep_mask on random rays and tables and on the sweep model's Cornell rays (tests/pool/sweep_piped_check.cpp,
which compiles the kernel's own header for the host).  tests/test_gpu_pool_waits.py holds the device side.
"""
import os
import re
import subprocess

import pytest

from test_leaf_sweep import CSRC, CXX, REPO, write_scene_bin

POOL = os.path.join(REPO, "tests", "pool")
TESTED_DEPTHS = (1, 2, 3, 4, 8)     # one_depth<D> in sweep_piped_check.cpp


def counts(line):
    words = line.split()
    return {k: int(v) for k, v in zip(words[::2], words[1::2])}


@pytest.fixture(scope="module")
def sweep_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("pool_waits")
    exe = str(d / "sweep_piped_check")
    subprocess.check_call(CXX + ["-o", exe, os.path.join(POOL, "sweep_piped_check.cpp"),
                                 os.path.join(CSRC, "pt_scene_pack.cpp"), os.path.join(CSRC, "pt_wide.cpp"),
                                 os.path.join(CSRC, "pt_scene.cpp")])

    def run(sb, stride):
        path = str(d / "scene.bin")
        write_scene_bin(sb, path)
        r = subprocess.run([exe, path, str(stride)], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
        return counts(r.stdout.strip().splitlines()[-1])
    return run


def test_piped_sweep_equals_the_plain_loop(sweep_check, cornell_scene):
    got = sweep_check(cornell_scene, 24)
    assert got["mismatches"] == 0, got
    assert got["octants"] == 0xff and got["infinite"] > 0, got
    assert got["random"] >= 40 * 24 * 33 and got["cornell"] > 10000, got


def test_the_kernel_depth_is_a_tested_one():
    """The depth the pool kernel is built with by default is one the host comparison instantiates."""
    text = open(os.path.join(CSRC, "pt_render_pool.h")).read()
    m = re.search(r"#ifndef PT_POOL_SWEEP_DEPTH\s*\n#define PT_POOL_SWEEP_DEPTH (\d+)", text)
    assert m, "PT_POOL_SWEEP_DEPTH has no default"
    assert int(m.group(1)) == 0 or int(m.group(1)) in TESTED_DEPTHS
