"""CPU checks of the planner's `common` flag (csrc/pt_launch_plan.cpp common_launch).

A launch whose plan says `common` may run the COMMON instantiation of k_render_sm, which holds the
default configuration's launch-uniform facts as constants.  A launch that is flagged while one of
those facts is false would render a wrong image (or fault), so each fact clears the flag on its
own here; tests/plan/common_dump.cpp runs the planner on the host.  The flag travels beside the
kernel key: the key of a flagged launch is the one tests/plan/plan_dump.cpp prints for the same case.
"""
import os
import subprocess

import pytest

from test_launch_plan import CORNELL, CSRC, IN, REPO, case, scene

C2_KEY = "0,1,7,0,1,1,256,0"
EXTRA = ("root_child", "tile_shift", "common_off")


def common_case(facts=CORNELL, width=1920, rows=1080, n_frames=1024, root_child=1, tile_shift=0, common_off=0, **kw):
    c = case(facts, width, rows, n_frames, tile_shift=tile_shift, **kw)
    c.update(root_child=root_child, tile_shift=tile_shift, common_off=common_off)
    return c


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("common_plan")
    exes = {}
    for name in ("common_dump", "plan_dump"):
        exes[name] = str(d / name)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exes[name],
                               os.path.join(REPO, "tests", "plan", name + ".cpp"),
                               os.path.join(CSRC, "pt_launch_plan.cpp")])

    def run(cases):
        """-> [(common, key, the key plan_dump prints for the case)]"""
        text = "".join(" ".join(str(c[k]) for k in IN + list(EXTRA)) + "\n" for c in cases)
        r = subprocess.run([exes["common_dump"]], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        mine = [ln.split() for ln in r.stdout.splitlines()]
        text = "".join(" ".join(str(c[k]) for k in IN) + "\n" for c in cases)
        r = subprocess.run([exes["plan_dump"]], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        theirs = [ln.split("|")[1].split()[23] for ln in r.stdout.splitlines()]
        assert len(mine) == len(theirs) == len(cases)
        return [(int(m[0]), m[1], t) for m, t in zip(mine, theirs)]
    run.kernels = subprocess.run([exes["common_dump"], "--kernels"], capture_output=True, text=True,
                                 check=True).stdout.split()
    return run


def test_common_list_is_the_c2_line(dump):
    assert dump.kernels == [C2_KEY]


def test_c2_launches_are_common(dump):
    """The C2 facts at 1024, 64 and 17 frames -- and small images, a row-split share, a captured
    graph, short launches and the moments (still frame-split) -- are flagged, with the parent's key."""
    cases = [common_case(n_frames=n) for n in (1024, 64, 17)]
    cases += [common_case(n_frames=n, moments=1) for n in (1024, 16)]
    cases += [common_case(width=64, rows=48, n_frames=n) for n in (1, 5, 24)]
    cases += [common_case(width=72, rows=40, n_frames=4, graph=1), common_case(rows=135, n_frames=1024),
              common_case(root_child=0), common_case(group_force=4), common_case(pull_batch=48),
              common_case(compact_max=0)]
    for c, (common, key, plain_key) in zip(cases, dump(cases)):
        assert common == 1 and key == C2_KEY == plain_key, c


ONE_FACT = dict(
    key21=dict(common_off=1),
    leaf_thresh=dict(leaf_thresh=33), leaf_thresh_same_value=dict(leaf_thresh=52),
    shade_thresh=dict(shade_thresh=17), trav_floor=dict(trav_floor=2),
    tile_16x4=dict(tile_shift=1), tile_32x2=dict(tile_shift=2), tile_64x1=dict(tile_shift=3),
    key15=dict(cons_off=1),
    minw6=dict(minw=6), minw8=dict(minw=8), minw5=dict(minw=5),
    counting=dict(counting=1),
    rpp2=dict(rpp=2),
    flag1=dict(flags=1), flag2=dict(flags=2), flag4=dict(flags=4), flag8=dict(flags=8), flag16=dict(flags=16),
    flag32=dict(flags=32),
    no_sphere=dict(facts=scene(35, 18, n_spheres=0)), two_spheres=dict(facts=scene(35, 18, n_spheres=2)),
    outside_guard=dict(facts=scene(35, 18, fast=0)),
    not_nested=dict(facts=scene(35, 18, nested=0)),
    over_pad_nodes=dict(facts=scene(69, 35)),
    root_is_a_leaf=dict(root_child=-1),
    global_memory=dict(variant=3),
    register_mode=dict(n_frames=64, group_force=64),
)


@pytest.mark.parametrize("name", sorted(ONE_FACT))
def test_one_fact_clears_common(dump, name):
    """Each fact the COMMON kernel holds as a constant, made false alone, clears the flag; the key
    stays whatever the planner makes without the flag."""
    (base, _, _), (common, key, plain_key) = dump([common_case(), common_case(**ONE_FACT[name])])
    assert base == 1
    assert common == 0 and key == plain_key, (name, key, plain_key)


def test_moments_in_register_mode_stay_common(dump):
    """With the moments on every launch is frame-split, whole-pixel items included: still the C2 line."""
    (common, key, plain_key), = dump([common_case(n_frames=64, group_force=64, moments=1)])
    assert common == 1 and key == C2_KEY == plain_key
