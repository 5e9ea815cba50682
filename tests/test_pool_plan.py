"""CPU checks of the planner's path-pool decision (csrc/pt_launch_plan.cpp, LaunchPlan::pool).

k_render_pool is the specialised swept line with its own staging, so a launch flagged `pool` while `common` or
`sweep` is false would render a wrong image, and a workgroup whose pools do not fit the CU's LDS would not launch.
tests/plan/pool_dump.cpp runs the planner on the host.
"""
import os
import subprocess

import pytest

from test_launch_plan import CORNELL, CSRC, IN, LDS_CU, REPO, case, scene

EXTRA = ("root_child", "n_leaves", "sweep_ok", "sweep_off", "pool_off", "adaptive")
OUT = "pool common sweep pool_paths pool_nt pool_blocks pool_lds_bytes overlap per_cu same".split()


def pool_case(facts=CORNELL, width=1920, rows=1080, n_frames=1024, root_child=1, n_leaves=None, sweep_ok=1, sweep_off=0,
              pool_off=0, adaptive=0, **kw):
    c = case(facts, width, rows, n_frames, **kw)
    c.update(root_child=root_child, n_leaves=facts["n_slots"] // 2 if n_leaves is None else n_leaves,
             sweep_ok=sweep_ok, sweep_off=sweep_off, pool_off=pool_off, adaptive=adaptive)
    return c


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pool_plan") / "pool_dump")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(REPO, "tests", "plan", "pool_dump.cpp"), os.path.join(CSRC, "pt_launch_plan.cpp")])

    def run(cases):
        text = "".join(" ".join(str(c[k]) for k in IN + list(EXTRA)) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        rows = [dict(zip(OUT, (int(x) for x in ln.split()))) for ln in r.stdout.splitlines()]
        assert len(rows) == len(cases)
        return rows
    return run


POOLED = [pool_case(n_frames=n) for n in (1024, 256, 64, 17)] + \
         [pool_case(rows=135), pool_case(width=64, rows=48, n_frames=24), pool_case(width=72, rows=40, n_frames=4, graph=1),
          pool_case(n_frames=4, overlap_slots=1), pool_case(group_force=4), pool_case(facts=scene(47, 24)),
          pool_case(facts=scene(1, 1), root_child=0)]


def test_default_long_launches_pool(dump):
    for c, r in zip(POOLED, dump(POOLED)):
        assert r["pool"] == 1 and r["common"] == 1 and r["sweep"] == 1 and r["overlap"] == 0, (c, r)


def test_pool_fits_the_cu(dump):
    """The workgroups the grid places on a CU hold their pools and trimmed scene in its 160 KiB, and a workgroup is
    whole waves of at most 128 paths each."""
    for c, r in zip(POOLED, dump(POOLED)):
        assert 64 <= r["pool_paths"] <= 128 and r["pool_nt"] % 64 == 0 and 64 <= r["pool_nt"] <= 1024, r
        waves = r["pool_nt"] // 64
        scene_bytes = (4 * c["n_slots"] + 3 * c["n_mats"] + 2 * c["n_spheres"] + 2 * c["n_leaves"]) * 16
        need = scene_bytes + waves * (r["pool_paths"] * 80 + (r["pool_paths"] + 15) // 16 * 16)
        assert r["pool_lds_bytes"] >= need, (c, r)
        assert r["pool_blocks"] >= 1 and r["per_cu"] * r["pool_lds_bytes"] <= LDS_CU, (c, r)
        # the occupancy the constants were measured at: 4 waves per SIMD on a full grid
        if c["width"] == 1920 and c["rows_local"] == 1080:      # (a small image has fewer workgroups than the chip holds)
            assert r["per_cu"] * waves == 16, (c, r)


OFF = dict(
    key24=dict(pool_off=1),
    key23=dict(sweep_off=1),
    no_table=dict(sweep_ok=0),
    key21_facts=dict(leaf_thresh=33),
    rpp2=dict(rpp=2),
    moller_trumbore=dict(flags=32),
    no_sky=dict(flags=2),
    counting=dict(counting=1),
    adaptive=dict(adaptive=1),
    overlap=dict(n_frames=4),
    overlap_16=dict(n_frames=16),
    key15=dict(cons_off=1),
    minw6=dict(minw=6),
    two_spheres=dict(facts=scene(35, 18, n_spheres=2)),
    global_memory=dict(variant=3),
    register_mode=dict(n_frames=64, group_force=64),
    too_many_frames=dict(n_frames=70000, scratch_budget=1 << 50),
    wide_image=dict(width=70000, rows=8),
    # 24 leaves and 40 materials: a 6.3 KB trimmed scene leaves one 512-thread workgroup per CU, 2 waves per SIMD
    scene_costs_a_workgroup=dict(facts=scene(47, 24, n_mats=40)),
)


@pytest.mark.parametrize("name", sorted(OFF))
def test_one_condition_switches_the_pool_off(dump, name):
    base, off = dump([pool_case(), pool_case(**OFF[name])])
    assert base["pool"] == 1
    assert off["pool"] == 0, (name, off)


def test_pool_implies_common_and_sweep_and_leaves_the_generic_fields(dump):
    """Over a grid of cases: `pool` only with `common && sweep` and never with an overlap slot, and every generic plan
    field is equal with key 24 at 0 and at 1."""
    cases = [pool_case(width=w, rows=h, n_frames=n, rpp=rpp, flags=fl, sweep_ok=ok, overlap_slots=sl)
             for w, h in ((1920, 1080), (64, 48), (9, 2), (1920, 135)) for n in (1, 4, 16, 17, 70, 1024)
             for rpp in (1, 2) for fl in (0, 32) for ok in (0, 1) for sl in (1, 3)]
    rows = dump(cases)
    assert any(r["pool"] for r in rows)
    for c, r in zip(cases, rows):
        assert r["same"] == 1, c
        if r["pool"]:
            assert r["common"] and r["sweep"] and not r["overlap"], (c, r)
