"""CPU checks of the render's launch planner (csrc/pt_launch_plan.{h,cpp}).

Every rule the planner holds (LDS staging, workgroup width, frames per item, queue batch,
grid, dynamic LDS, the k_render_sm instantiation) leaves the image bit-exact, so the GPU
parity tests cannot see a wrong one: it shows as lost speed or as a fault.  Here
tests/plan/plan_dump.cpp runs the planner itself on the host:

  * tests/golden/launch_plans.txt -- plans recorded from the launch code as it stood before
    the planner existed -- must be reproduced exactly;
  * the kernels the recorded profiles show (profiles/r06_*kernel_stats.csv) are the ones chosen;
  * for every row of that table and a seeded random sweep, the plan is sound against what
    k_render_sm does with it (the staging extents below restate the kernel's), and its
    kernel key is a line of pt_render_kernels.h.
"""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl-path-tracing_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "launch_plans.txt")

LDS_CU = 160 * 1024
PAD_NODES, PULL_BATCH = 67, 32          # ptl::kPadNodes, kPullBatch
IN = ("n_nodes n_spheres n_mats n_slots n_top walk_np scene_fast walk_nested wide_ok n_wide leaf_cert_ok lds_bytes "
      "lds_bytes_sk leaf_thresh shade_thresh minw trav_floor compact_max pull_batch group_force cons_off wide_off "
      "wide_threads overlap_bpc cert_off overlap_slots scratch_budget variant width rows_local n_tiles rpp flags n_cu "
      "persist_blocks counting moments aces_fuse n_frames graph").split()
OUT = ("lds wide cons_walk leaf_cert split overlap shade_lds nt mw group pull_batch grp_magic leaf_thresh shade_thresh "
       "trav_floor n_top wide_top blocks dyn_lds_bytes accum_long accum_moments aces_out accum_blocks key launch_frames "
       "scratch_bytes id_limit").split()
KEY = "count lds minw multi split padn nt wide".split()
TUNING = dict(leaf_thresh=0, shade_thresh=0, minw=0, trav_floor=0, compact_max=63, pull_batch=0, group_force=0,
              cons_off=0, wide_off=0, wide_threads=0, overlap_bpc=0, cert_off=0, overlap_slots=3,
              scratch_budget=32 << 30, variant=0)


def scene(n_nodes, n_leaves, n_mats=11, n_spheres=1, nested=1, wide=1, fast=1, cert=1):
    """The facts pt_upload_scene derives for a tree of these sizes."""
    N = max(PAD_NODES, n_nodes)
    lds = (16 * N + 8 * n_leaves + 3 * n_mats + 2 * n_spheres) * 16
    return dict(n_nodes=n_nodes, n_spheres=n_spheres, n_mats=n_mats, n_slots=2 * n_leaves, n_top=min(n_nodes, 768),
                walk_np=N, scene_fast=fast, walk_nested=nested, wide_ok=wide, n_wide=(2 * n_nodes) // 3 if wide else 0,
                leaf_cert_ok=cert, lds_bytes=lds, lds_bytes_sk=lds + 2 * N * 16)


CORNELL = scene(35, 18)                              # C2
BIG = scene(139999, 70000, n_mats=7, n_spheres=0)    # a C3 / C4-size tree with its wide tree


def case(facts, width, rows, n_frames, tile_shift=0, **kw):
    c = dict(facts, **TUNING)
    tw, th = 8 << tile_shift, 8 >> tile_shift
    c.update(width=width, rows_local=rows, n_tiles=((width + tw - 1) // tw) * ((rows + th - 1) // th), rpp=1, flags=0,
             n_cu=256, persist_blocks=2048, counting=0, moments=0, aces_fuse=0, n_frames=n_frames, graph=0)
    assert not set(kw) - set(c), kw
    c.update(kw)
    return c


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_dump")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(REPO, "tests", "plan", "plan_dump.cpp"), os.path.join(CSRC, "pt_launch_plan.cpp")])

    def run(cases):
        """Plans of `cases` (dicts, or input strings): the output lines and their parsed form."""
        text = "".join((c if isinstance(c, str) else " ".join(str(c[k]) for k in IN)) + "\n" for c in cases)
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        return lines, [parse(ln) for ln in lines]
    run.kernels = subprocess.run([exe, "--kernels"], capture_output=True, text=True, check=True).stdout.split()
    return run


def parse(line):
    a, b = line.split("|")
    d = dict(zip(IN, map(int, a.split())))
    for k, v in zip(OUT, b.split()):
        d["o_" + k] = v if k == "key" else int(v)
    d["k"] = dict(zip(KEY, map(int, d["o_key"].split(","))))
    return d


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return [ln.rstrip("\n") for ln in f if ln.strip() and not ln.startswith("#")]


def test_golden_table(dump, golden):
    assert 200 <= len(golden) and os.path.getsize(GOLDEN) < 100 * 1024
    lines, _ = dump([ln.split("|")[0] for ln in golden])
    bad = [(w, g) for w, g in zip(golden, lines) if w != g]
    assert not bad, "%d of %d plans differ; first:\nwant %s\ngot  %s" % (len(bad), len(golden), bad[0][0], bad[0][1])


def test_kernel_list_is_49_distinct_lines(dump):
    assert len(dump.kernels) == 49 and len(set(dump.kernels)) == 49


def test_recorded_kernels(dump):
    """profiles/r06_kernel_stats.csv and r06_interactive_kernel_stats.csv name the kernels the
    benchmark shapes ran: C2 (the padded Cornell copy), C3 / C4 (wide global walk), and the
    counting runs of both."""
    assert CORNELL["walk_np"] == PAD_NODES
    cases = [case(CORNELL, 1920, 1080, 1024), case(CORNELL, 1920, 1080, 1), case(BIG, 1920, 1080, 256),
             case(CORNELL, 1920, 1080, 64, counting=1), case(BIG, 1920, 1080, 64, counting=1)]
    _, plans = dump(cases)
    assert [p["o_key"] for p in plans] == ["0,1,7,0,1,1,256,0", "0,1,7,0,1,1,256,0", "0,0,6,0,1,0,256,1",
                                           "1,1,5,0,1,0,256,0", "1,0,5,0,1,0,256,0"]


def random_cases(n, seed=20250):
    rng = np.random.RandomState(seed)
    pick = lambda *v: v[rng.randint(len(v))]
    maybe = lambda p, v, d=0: v if rng.rand() < p else d
    out = []
    for i in range(n):
        # leaves: half the cases in the range where the LDS copy is 10..170 KiB, the rest up to 2^22
        leaves = int(rng.randint(1, 270)) if rng.rand() < 0.6 else int(2 ** rng.uniform(0, 22))
        nested = int(rng.rand() < 0.8)
        f = scene(2 * leaves - 1, leaves, n_mats=int(2 ** rng.uniform(0, 9)), n_spheres=maybe(0.7, int(rng.randint(0, 40))),
                  nested=nested, wide=nested and int(rng.rand() < 0.9), fast=int(rng.rand() < 0.9), cert=int(rng.rand() < 0.8))
        big = rng.rand() < 0.03     # images near the 2^31-pixel limit: queue ids and scratch split the render
        width = int(rng.randint(16384, 65537)) if big else int(2 ** rng.uniform(0, 12.5))
        rows = int(rng.randint(8192, (1 << 31) // width)) if big else maybe(0.97, int(2 ** rng.uniform(0, 11.5)))
        n_frames = int(2 ** rng.uniform(0, 13))
        kw = dict(rpp=pick(1, 1, 1, 2, 3), flags=pick(0, 0, 16, 32, 63), counting=maybe(0.15, 1), moments=maybe(0.15, 1),
                  aces_fuse=maybe(0.3, 1), graph=maybe(0.2, 1), minw=maybe(0.3, pick(5, 6, 7, 8)), variant=maybe(0.15, 3),
                  group_force=maybe(0.25, pick(1, 2, 5, n_frames, n_frames + 3)), pull_batch=maybe(0.15, pick(1, 48, 1024)),
                  cons_off=maybe(0.15, 1), wide_off=maybe(0.15, 1), wide_threads=maybe(0.3, pick(256, 512, 768, 1024)),
                  overlap_bpc=maybe(0.15, pick(1, 4, 8)), cert_off=maybe(0.1, 1), overlap_slots=pick(3, 3, 1, 2, 4),
                  scratch_budget=pick(32 << 30, 32 << 30, 1 << 20, 48 << 30, 1 << 30), leaf_thresh=maybe(0.1, 33),
                  shade_thresh=maybe(0.1, 17), trav_floor=maybe(0.1, 2), compact_max=maybe(0.1, 0, 63))
        out.append(case(f, width, rows, n_frames, tile_shift=pick(0, 0, 1, 2, 3), **kw))
    return out


@pytest.fixture(scope="module")
def plans(dump, golden):
    """The plans of the golden table's cases and of the random sweep."""
    _, a = dump([ln.split("|")[0] for ln in golden])
    _, b = dump(random_cases(4000))
    return a + b


def staged_float4(p):
    """The float4 extent k_render_sm<key> stages in dynamic LDS for these facts and this plan
    (the three staging loops at the top of the kernel)."""
    k = p["k"]
    shading = 3 * p["n_mats"] + 2 * p["n_spheres"]
    if k["lds"]:        # 8 octant images (the culling walk: + the sink image), triangles, shading records
        N = PAD_NODES if k["padn"] else p["walk_np"]
        return (18 * N if (not k["count"] and p["o_cons_walk"]) else 16 * N) + 4 * p["n_slots"] + shading
    if k["wide"]:       # top records of the wide tree, 3 float4 each
        return 3 * p["o_wide_top"] + (shading if p["o_shade_lds"] else 0)
    return 2 * p["o_n_top"] + (shading if p["o_shade_lds"] else 0)     # top nodes


def test_plans_are_sound(plans):
    rng = np.random.RandomState(7)
    for p in plans:
        k, ctx = p["k"], str(p)
        assert staged_float4(p) * 16 <= p["o_dyn_lds_bytes"] <= LDS_CU, ctx
        assert LDS_CU // max(p["o_dyn_lds_bytes"], 1) >= 1, ctx
        if k["padn"]:
            assert p["walk_np"] == PAD_NODES, ctx       # the compile-time plane offset is the scene's
        assert (k["lds"], k["wide"], k["count"], k["split"]) == (p["o_lds"], p["o_wide"], p["counting"], p["o_split"]), ctx
        assert k["multi"] == (p["rpp"] > 1), ctx
        if k["wide"]:
            assert p["o_wide_top"] <= p["n_wide"] and p["wide_ok"] and p["scene_fast"], ctx
        else:
            assert p["o_n_top"] <= p["n_top"], ctx
        assert p["o_nt"] == k["nt"] and k["nt"] in (256, 512, 768, 1024), ctx
        assert p["o_blocks"] >= 1, ctx
        assert 1 <= p["o_group"] <= p["n_frames"], ctx
        assert p["o_pull_batch"] >= (p["pull_batch"] or PULL_BATCH), ctx
        assert p["o_split"] or p["o_group"] == p["n_frames"], ctx       # register mode owns whole pixels
        assert (p["o_scratch_bytes"] > 0) == bool(p["o_split"]), ctx
        ng = (p["n_frames"] + p["o_group"] - 1) // p["o_group"]
        items, m = p["n_tiles"] * ng, p["o_grp_magic"]
        if m:
            for item in [0, items - 1] + [int(x) for x in rng.randint(0, max(items, 1), 100)]:
                if 0 <= item < items:
                    assert (item * m) >> 32 == item // ng, ctx
        else:
            assert ng == 1 or items * ng >= 1 << 32, ctx
        assert 1 <= p["o_launch_frames"] <= p["n_frames"], ctx


def test_launches_of_a_render_keep_queue_ids_and_scratch_in_bounds(dump, plans):
    """enqueue_frames issues a render as launches of launch_frames() frames and a remainder:
    each keeps its queue ids below id_limit, and its scratch within the budget (one frame per
    launch always runs)."""
    again = []
    for p in plans:
        step = p["o_launch_frames"]
        for n in {step, p["n_frames"] % step} - {0}:
            again.append(dict({k: p[k] for k in IN}, n_frames=n))
    _, launches = dump(again)
    for q in launches:
        ng = (q["n_frames"] + q["o_group"] - 1) // q["o_group"]
        if q["o_split"]:
            assert q["n_tiles"] * ng * 64 < q["o_id_limit"] or q["n_frames"] == 1, str(q)
            assert q["o_scratch_bytes"] <= q["scratch_budget"] or q["n_frames"] == 1, str(q)
        assert q["o_id_limit"] + 2048 * 4 * 2 * max(256, q["pull_batch"]) < 1 << 32, str(q)


def test_every_key_is_in_the_kernel_list(dump, plans):
    made = {p["o_key"] for p in plans}
    assert made <= set(dump.kernels), sorted(made - set(dump.kernels))
    unused = [k for k in dump.kernels if k not in made]
    print("k_render_sm lines no plan selects (%d of 49): %s" % (len(unused), unused))


def test_gpu_parity_line_cases_select_their_lines(dump, tmp_path):
    """tests/test_gpu_parity.py::test_kernel_list_line covers the lines of the kernel list no other
    GPU test launches; the planner says each of its configurations selects the line it names."""
    import test_gpu_parity as G
    facts, cases = {}, []
    for line, name, variant, rpp, waves, group, wide_off, wide_threads, counting in G.KERNEL_LINE_CASES:
        if name not in facts:
            nodes = np.asarray(G.line_scene(name, tmp_path / name)["nodes"], np.float32).reshape(-1, 12)
            facts[name] = scene(len(nodes), int((nodes[:, 8] > -1).sum()))     # 11 materials, 1 sphere: the room's
        cases.append(case(facts[name], G.LINE_W, G.LINE_H, G.LINE_FRAMES, variant=variant, rpp=rpp, minw=waves,
                          group_force=group, wide_off=wide_off, wide_threads=wide_threads, counting=int(counting)))
    _, plans = dump(cases)
    assert [p["o_key"] for p in plans] == [c[0] for c in G.KERNEL_LINE_CASES]
    assert len({c[0] for c in G.KERNEL_LINE_CASES}) == len(G.KERNEL_LINE_CASES)
