"""The launch planner on the shortened queues of adaptive sampling: a launch of
pt_render_adaptive is planned from Image::n_tiles = the number of tiles still active, anything
from 1 to the whole grid, with State::adaptive set.  For LDS, wide-workgroup and global-memory
scenes every such plan must name a built kernel, keep its queue ids within the id limit, carry
an item division that is exact for every item of the shortened queue, and be a plain synchronous
split launch on a generic line; with the whole grid and the flag at its default the planner
still prints tests/golden/launch_plans.txt.  Runs tests/plan/adaptive_dump.cpp on the CPU."""
import os
import subprocess

import numpy as np
import pytest

from test_launch_plan import BIG, CORNELL, CSRC, IN, REPO, case, dump, golden, parse, scene  # noqa: F401  (dump, golden: fixtures)

MID = scene(299, 150)            # a 96 KiB LDS copy: staged by a wide workgroup
FACTS = dict(lds=CORNELL, wide_workgroup=MID, global_memory=BIG)
FRAMES = (2, 8, 24, 64)          # the batches of tests/test_gpu_adaptive.py and of the measurement


@pytest.fixture(scope="module")
def adaptive_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "adaptive_dump")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(REPO, "tests", "plan", "adaptive_dump.cpp"), os.path.join(CSRC, "pt_launch_plan.cpp")])

    def run(cases):
        text = "".join(" ".join(str(c[k]) for k in IN) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        out = []
        for ln in lines:
            d = parse(ln)
            d["o_overlap2"], d["o_common"] = map(int, ln.split()[-2:])
            out.append(d)
        return out
    return run


def tile_counts(full):
    """1 .. the full grid: every count up to 70, then a spread, and the grid itself."""
    rng = np.random.RandomState(full)
    return sorted((set(range(1, min(full, 70) + 1)) | {int(x) for x in rng.randint(1, full + 1, 60)} |
                   {full // 2, full - 1, full}) - {0})


@pytest.mark.parametrize("name", sorted(FACTS))
@pytest.mark.parametrize("width, rows", [(64, 48), (61, 37), (1920, 1080)])
def test_shortened_queues(dump, adaptive_dump, name, width, rows):
    full = case(FACTS[name], width, rows, 8)["n_tiles"]
    plans = adaptive_dump([case(FACTS[name], width, rows, n, moments=1, n_tiles=a)
                           for n in FRAMES for a in tile_counts(full)])
    if name == "wide_workgroup":
        assert {p["o_nt"] for p in plans} == {1024}
    assert {p["o_lds"] for p in plans} == {int(name != "global_memory")}
    assert {p["o_wide"] for p in plans} == {int(name == "global_memory")}
    groups = set()
    for p in plans:
        ctx = str(p)
        assert (p["o_split"], p["o_overlap"], p["o_overlap2"], p["o_common"]) == (1, 0, 0, 0), ctx
        assert p["o_key"] in dump.kernels, ctx
        ng = (p["n_frames"] + p["o_group"] - 1) // p["o_group"]
        items = p["n_tiles"] * ng
        groups.add(p["o_group"])
        assert items * 64 < p["o_id_limit"] < 1 << 32, ctx
        assert p["o_launch_frames"] == p["n_frames"], ctx        # one launch per batch at these sizes
        assert 1 <= p["o_blocks"] <= max(1, -(-items * 64 // p["o_nt"])), ctx
        m = p["o_grp_magic"]
        if m:
            item = np.arange(items, dtype=np.uint64)
            assert np.array_equal((item * np.uint64(m)) >> np.uint64(32), item // np.uint64(ng)), ctx
        else:
            assert ng == 1, ctx                                  # (items * ng < 2^32 at these sizes: a magic exists)
    if (width, name) == (1920, "lds"):
        assert len(groups) > 1, groups                           # sparse lists take shorter items than the full grid


def test_full_grid_is_the_recorded_plan(dump, golden):
    """Every recorded case has the whole grid as its queue and no adaptive flag: the planner as
    it stands reproduces each line, so every other launch is planned as before."""
    lines, _ = dump([ln.split("|")[0] for ln in golden])
    assert lines == golden
