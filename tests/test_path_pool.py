"""CPU checks of the per-wave path pool (csrc/pt_pool.h): tests/pool/pool_sim.cpp drives the list
functions the kernel calls with the candidate distribution of C2's segments, through refill and drain, and fails when
a path is ever in no place or in two, when a segment is lost or duplicated, or when a pass runs fewer than
min(64, ceil(P / 2)) lanes while the queue has work (the pigeonhole bound).  It also prints the modelled wave-VALU per
segment from per-pass costs (the prediction recorded in profiles/ab/r13_path_pool/).  The GPU side is
tests/test_gpu_path_pool.py.
"""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl-path-tracing_amd", "csrc")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pool") / "pool_sim")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", exe,
                           os.path.join(REPO, "tests", "pool", "pool_sim.cpp")])

    def run(P, items, *costs):
        r = subprocess.run([exe, str(P), str(items)] + [str(c) for c in costs], capture_output=True, text=True)
        out = json.loads(r.stdout.strip().splitlines()[-1])
        out["rc"] = r.returncode
        return out
    return run


@pytest.mark.parametrize("P", [64, 68, 80, 96, 112, 116, 128])
def test_invariants(sim, P):
    res = sim(P, 5000)
    print(res)
    assert res["rc"] == 0 and res["violations"] == 0 and res["lost"] == 0 and res["short_passes"] == 0, res
    assert res["floor_lanes"] == min(64, (P + 1) // 2)


@pytest.mark.parametrize("items", [0, 1, 63, 65, 129])
def test_refill_and_drain_of_short_queues(sim, items):
    """Fewer items than paths, one more than a pass, one more than the pool: every segment is served once and every
    path retires."""
    res = sim(112, items)
    assert res["rc"] == 0 and res["lost"] == 0 and res["violations"] == 0, res


def test_lane_use_grows_with_the_pool(sim):
    """One path per lane is today's kernel (about 0.7 lane use); with 128 paths every pass is full until the drain."""
    use = {P: sim(P, 20000)["lane_use"] for P in (64, 96, 128)}
    assert use[64] < use[96] < use[128] and use[128] > 0.98 and use[64] < 0.8, use


def test_model_uses_the_costs(sim):
    a, b = sim(96, 5000, 720, 450, 30), sim(96, 5000, 1440, 900, 60)
    assert abs(b["wave_valu_per_segment"] - 2 * a["wave_valu_per_segment"]) < 0.02, (a, b)
