"""CPU checks of the scene packer (csrc/pt_scene_pack.{h,cpp}).

pt_upload_scene copies to the device what ptp::pack_scene built on the host: the validated scene's node records in
the top numbering, the leaf triangle quads, the eight octant walk images and the sink image, the wide tree's
arrays, materials, spheres, and the facts the launch planner reads.  A wrong offset there shows on the GPU only as
a wrong image or a fault.  Here tests/pack/pack_dump.cpp runs the packer itself on the host:

  * tests/golden/scene_packs.txt -- one row per input of build_inputs below: the return code and error text of a
    rejected scene, or every buffer's size and a digest of its bytes and every SceneFacts field -- must be
    reproduced exactly.  The rows were recorded from pt_upload_scene as it stood before the packer existed: a
    throwaway program (not kept) held that function's body, cut by line range from pt_render.hip of the commit
    before this file, over host stand-ins for float4, hipMalloc and hipMemcpy that captured the copied bytes, and
    printed them through pack_dump's own print_row.  It was built twice, with g++ -O3 -march=x86-64-v3 and with
    ROCm's clang++ -O3 (the compiler of the shipped function), both with the Makefile's FPFLAGS; the two gave
    identical rows for every input.
  * structural checks on the same dumps say what is wrong when a digest differs: the top numbering, every link of
    every octant image, the sinks, the leaf slots, the continuation words, the buffer sizes and the LDS bytes.

The issue that asked for this test lists a fractional link among the rejected inputs.  The old code accepted one
(the shader's int(float) truncates, so the validator casts), and so does the packer: `link_fractional` is an
accepted row whose tree is not nested, because pt_bvh_culling_ok wants integral links.

Which layout branch each input takes (checked by hand against the recorded facts): Cornell is padded to kPadNodes
per image plane, the ship is not; the bunny has more nodes than kTopNodes; `poking_child` is not nested (no sink
image, no wide buffers); `inverted_box` is nested but has no wide tree; `orphan_leaf` has a leaf without a wide
index; `one_triangle` has a single-triangle leaf as its root; `shrunk_leaves` fails the leaf containment.
"""
import os
import subprocess

import numpy as np
import pytest

import fuzz_scenes
import pt_host as H
import test_launch_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "opengl-path-tracing_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "scene_packs.txt")

PAD_NODES, TOP_NODES, WIDE_STRIDE = 67, 768, 3      # ptl::kPadNodes, ptp::kTopNodes, kWideStride
BUFS = "nodes tris mats spheres walk walk_sink wide_rec wide_lbox wide_nodes wide_tris".split()   # ptp::SceneBuf
FACTS = ("n_nodes n_spheres n_mats n_slots n_top walk_np scene_fast walk_nested wide_ok n_wide leaf_cert_ok lds_bytes "
         "lds_bytes_sk rb0 rb1 rb2 rb3 rb4 rb5 root_child cm0 cm1 cm2 ws0 ws1 ws2 win_bad cw0 cw1 cw2").split()
PT_E_ARG, PT_E_SCENE = -1, -4


def _scene(sb, **over):
    d = {k: np.array(sb[k], np.float32) for k in ("tris", "nodes", "mats", "spheres")}
    d["tris"], d["nodes"] = d["tris"].reshape(-1, 16), d["nodes"].reshape(-1, 12)
    d["mats"], d["spheres"] = d["mats"].reshape(-1, 16), d["spheres"].reshape(-1, 8)
    d.update(over)
    return d


def _edit(sc, key, idx, value):
    a = sc[key].copy()
    a[idx] = value
    return dict(sc, **{key: a})


def _leaves(sc):
    return [i for i in range(len(sc["nodes"])) if sc["nodes"][i, 8] > -1.0]


def _tri(v0, v1, v2):
    t = np.zeros(16, np.float32)
    t[0:3], t[4:7], t[8:11] = v0, v1, v2
    return t


def coplanar_scene():
    """Two hand-threaded leaves under one root.  Leaf 1: the two halves of a quad in z = 0 whose stored normals
    are (+0, +0, 1) and (-0, +0, 1) -- equal planes, different bytes (the signed-zero case of ptp::same_plane).
    Leaf 2: two triangles in different planes."""
    tris = np.stack([_tri((0, 0, 0), (1, 0, 0), (1, 1, 0)), _tri((-1, 0, 0), (-1, -1, 0), (0, 0, 0)),
                     _tri((0, 0, 1), (1, 0, 1), (1, 1, 1)), _tri((0, 0, 1), (1, 0, 2), (0, 1, 1))])
    nodes = np.zeros((3, 12), np.float32)
    nodes[0] = [-1, -1, 0, 0, 1, 1, 2, 0, -1, -1, 1, -1]
    nodes[1] = [-1, -1, 0, 0, 1, 1, 0, 0, 0, 1, 2, 2]
    nodes[2] = [0, 0, 1, 0, 1, 1, 2, 0, 2, 3, -1, -1]
    mats = np.zeros((1, 16), np.float32)
    mats[0, 0:3] = 0.5
    return dict(tris=tris, nodes=nodes, mats=mats, spheres=np.zeros((0, 8), np.float32))


def build_inputs(tmp, cornell_scene, ship_scene):
    """name -> (counts, mode, scene arrays or None), in the order of the golden table."""
    import pt_scenes
    c = _scene(cornell_scene)
    n = len(c["nodes"])
    leaves = _leaves(c)
    inner = [i for i in range(n) if i not in leaves]
    out = {}

    def ok(name, sc):
        out[name] = ((len(sc["tris"]), len(sc["nodes"]), len(sc["mats"]), len(sc["spheres"])), 0, sc)

    assert n == 35
    ok("cornell", c)
    ok("ship", _scene(ship_scene))
    bunny = _scene(H.setupBuffers(*pt_scenes.write_scene("bunny", str(tmp), target_tris=2000)))
    assert len(bunny["nodes"]) > TOP_NODES
    ok("bunny_2000", bunny)
    child = int(c["nodes"][0, 10])
    ok("poking_child", _edit(c, "nodes", (child, 0), c["nodes"][0, 0] - 1.0))
    orphan = c["nodes"][leaves[0]].copy()
    orphan[10] = orphan[11] = -1.0
    ok("orphan_leaf", dict(c, nodes=np.concatenate([c["nodes"], orphan[None]])))
    shrunk = c["nodes"].copy()
    for i in leaves[:8]:
        ax = int(np.argmax(shrunk[i, 4:7] - shrunk[i, 0:3]))
        shrunk[i, 4 + ax] = np.float32(0.5 * (shrunk[i, ax] + shrunk[i, 4 + ax]))
    ok("shrunk_leaves", dict(c, nodes=shrunk))
    ok("tiny_coordinate", _edit(c, "nodes", (leaves[3], 1), 1e-20))       # below 2^-40: scene_fast 0
    ok("huge_coordinate", _edit(c, "nodes", (0, 4), 3e20))                # above 2^60
    inv = c["nodes"].copy()
    i = leaves[2]
    inv[i, 0], inv[i, 4] = c["nodes"][i, 4], c["nodes"][i, 0]              # min.x > max.x on a leaf with extent
    assert inv[i, 0] > inv[i, 4]
    ok("inverted_box", dict(c, nodes=inv))
    one = _scene(H.scene_from_arrays(np.stack([_tri((0, 0, 0), (1, 0, 1), (0, 1, 0.5))]), c["mats"][:1], builtins=False))
    assert len(one["nodes"]) == 1
    ok("one_triangle", one)
    sph = np.zeros((2, 8), np.float32)
    sph[:, 0:4] = [[0, 0, 1, 0.5], [2, 1, 0, 1.5]]
    sph[1, 4] = 1
    ok("spheres_only", dict(tris=np.zeros((0, 16), np.float32), nodes=np.zeros((0, 12), np.float32),
                            mats=c["mats"][:2], spheres=sph))
    ok("empty", dict(tris=np.zeros((0, 16), np.float32), nodes=np.zeros((0, 12), np.float32),
                     mats=np.zeros((0, 16), np.float32), spheres=np.zeros((0, 8), np.float32)))
    ok("coplanar_pairs", coplanar_scene())
    for seed in range(len(fuzz_scenes.SIZES)):                            # one per size; seed 5 (300) moved far off
        ok("fuzz_%d" % seed, _scene(fuzz_scenes.random_case(seed, far=(seed == 5))[0]))
    # a fractional link truncates like the shader's int(float): accepted, but the tree check wants integers
    frac = c["nodes"].copy()
    frac[leaves[1], 10:12] += 0.5
    ok("link_fractional", dict(c, nodes=frac))

    # --- one rejected input per error string of the validator
    out["negative_count"] = ((-1, 0, 1, 0), 2, None)
    out["null_with_count"] = ((1, 1, 1, 0), 1, None)
    out["too_many_records"] = ((4, (1 << 24) + 1, 1, 0), 2, None)
    ok("no_materials", dict(c, mats=np.zeros((0, 16), np.float32)))
    ok("link_nan", _edit(c, "nodes", (inner[1], 11), np.nan))
    ok("link_huge", _edit(c, "nodes", (inner[1], 10), 3e38))
    ok("link_out_of_range", _edit(c, "nodes", (leaves[0], 10), float(n)))
    ok("link_below_range", _edit(c, "nodes", (inner[2], 10), -2.0))
    ok("leaf_index_out_of_range", _edit(c, "nodes", (leaves[4], 9), float(len(c["tris"]))))
    ok("leaf_index_nan", _edit(c, "nodes", (leaves[4], 9), np.nan))
    lk = c["nodes"].copy()
    lk[leaves[0], 10] = lk[leaves[0], 11] + 1 if lk[leaves[0], 11] + 1 < n else 0
    ok("leaf_hit_ne_miss", dict(c, nodes=lk))
    ok("internal_without_hit", _edit(c, "nodes", (inner[3], 10), -1.0))
    cyc = c["nodes"].copy()
    cyc[leaves[-1], 10:12] = 0.0
    ok("cycle", dict(c, nodes=cyc))
    ok("triangle_material", _edit(c, "tris", (5, 12), float(len(c["mats"]))))
    assert len(c["spheres"]) > 0
    ok("sphere_material", _edit(c, "spheres", (0, 4), -1.0))
    return out


def write_input(path, counts, mode, sc):
    with open(path, "wb") as f:
        np.array(list(counts) + [mode], np.int32).tofile(f)
        if mode == 0:
            for k in ("tris", "nodes", "mats", "spheres"):
                np.ascontiguousarray(sc[k], np.float32).tofile(f)


def parse_buffers(path):
    with open(path, "rb") as f:
        raw = f.read()
    bufs, want, o = {}, {}, 0
    for name in BUFS:
        n, w = np.frombuffer(raw, np.int64, 2, o)
        o += 16
        bufs[name] = np.frombuffer(raw, np.float32, 4 * int(n), o).reshape(-1, 4)
        want[name] = int(w)
        o += 16 * int(n)
    nn = int(np.frombuffer(raw, np.int32, 1, o)[0])
    pos = np.frombuffer(raw, np.int32, nn, o + 4)
    assert o + 4 + 4 * nn == len(raw)
    return bufs, want, pos


@pytest.fixture(scope="module")
def packs(tmp_path_factory, cornell_scene, ship_scene):
    """Every input packed once: name -> (row, facts or None, buffers or None, size function, top numbering)."""
    d = tmp_path_factory.mktemp("pack")
    exe = str(d / "pack_dump")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-march=x86-64-v3", "-Wall",
                           "-Werror", "-o", exe, os.path.join(REPO, "tests", "pack", "pack_dump.cpp"),
                           os.path.join(CSRC, "pt_scene_pack.cpp"), os.path.join(CSRC, "pt_wide.cpp"),
                           os.path.join(CSRC, "pt_scene.cpp")])
    out = {}
    for name, (counts, mode, sc) in build_inputs(d, cornell_scene, ship_scene).items():
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        write_input(src, counts, mode, sc)
        r = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stderr)
        row = r.stdout.strip()
        if row.startswith("rc=0 "):
            facts = dict(zip(FACTS, row.split("facts=")[1].split()))
            facts = {k: int(v, 16) if k[:2] in ("rb", "cm", "ws", "cw") else int(v) for k, v in facts.items()}
            out[name] = (row, facts) + parse_buffers(dst) + (sc,)
        else:
            out[name] = (row, None, None, None, None, sc)
    return out


def accepted(packs):
    return [(name, p) for name, p in packs.items() if p[1] is not None]


def test_golden_table(packs):
    with open(GOLDEN) as f:
        golden = [ln.rstrip("\n") for ln in f if ln.strip() and not ln.startswith("#")]
    assert os.path.getsize(GOLDEN) < 64 * 1024
    got = ["%s %s" % (name, p[0]) for name, p in packs.items()]
    assert len(golden) == len(got) >= 35
    bad = [(w, g) for w, g in zip(golden, got) if w != g]
    assert not bad, "%d of %d rows differ; first:\nwant %s\ngot  %s" % (len(bad), len(golden), bad[0][0], bad[0][1])


def test_rejections(packs):
    """Every error string of the validator, with its code."""
    want = {"negative_count": (PT_E_ARG, "negative count"),
            "null_with_count": (PT_E_ARG, "null array with nonzero count"),
            "too_many_records": (PT_E_SCENE, "scene exceeds 2^24 records"),
            "no_materials": (PT_E_SCENE, "no materials"),
            "link_nan": (PT_E_SCENE, "BVH link out of range at node"),
            "link_huge": (PT_E_SCENE, "BVH link out of range at node"),
            "link_out_of_range": (PT_E_SCENE, "BVH link out of range at node"),
            "link_below_range": (PT_E_SCENE, "BVH link out of range at node"),
            "leaf_index_out_of_range": (PT_E_SCENE, "leaf triangle index out of range at node"),
            "leaf_index_nan": (PT_E_SCENE, "leaf triangle index out of range at node"),
            "leaf_hit_ne_miss": (PT_E_SCENE, "leaf with hit link != miss link is unsupported"),
            "internal_without_hit": (PT_E_SCENE, "internal node without a hit link at node"),
            "cycle": (PT_E_SCENE, "BVH links form a cycle"),
            "triangle_material": (PT_E_SCENE, "triangle material index out of range"),
            "sphere_material": (PT_E_SCENE, "sphere material index out of range")}
    assert {n for n, p in packs.items() if p[1] is None} == set(want)
    for name, (rc, text) in want.items():
        assert packs[name][0].startswith("rc=%d err=%s" % (rc, text)), (name, packs[name][0])


def test_sizes_and_lds_bytes(packs):
    for name, (_, f, bufs, want, pos, sc) in accepted(packs):
        assert {k: len(v) for k, v in bufs.items()} == want, name
        N, n_leaves = max(PAD_NODES, f["n_nodes"]), f["n_slots"] // 2
        assert f["walk_np"] == N and f["n_top"] == min(f["n_nodes"], TOP_NODES), name
        # the facts tests/test_launch_plan.py assumes of a tree of these sizes (its planner inputs) are the packer's
        assumed = test_launch_plan.scene(f["n_nodes"], n_leaves, n_mats=f["n_mats"], n_spheres=f["n_spheres"])
        for k in ("n_slots", "n_top", "walk_np", "lds_bytes", "lds_bytes_sk"):
            assert f[k] == assumed[k], (name, k)
        assert f["lds_bytes"] == (16 * N + 8 * n_leaves + 3 * f["n_mats"] + 2 * f["n_spheres"]) * 16, name
        assert f["lds_bytes_sk"] == f["lds_bytes"] + 2 * N * 16, name
        assert len(bufs["walk"]) == 16 * N and len(bufs["walk_sink"]) == (18 * N if f["walk_nested"] else 0), name
        ni = f["n_wide"] if f["wide_ok"] else 0
        assert (len(bufs["wide_rec"]), len(bufs["wide_lbox"]), len(bufs["wide_tris"])) == (WIDE_STRIDE * ni, 2 * ni, 8 * ni)
        assert len(bufs["wide_nodes"]) == (len(bufs["nodes"]) if ni else 0), name
        assert not f["wide_ok"] or f["walk_nested"], name


def test_expected_branches(packs):
    """The facts that say which layout branch an input took (the module docstring's list)."""
    f = {name: p[1] for name, p in accepted(packs)}
    assert f["cornell"]["walk_np"] == PAD_NODES > f["cornell"]["n_nodes"] and f["ship"]["walk_np"] == f["ship"]["n_nodes"]
    assert f["bunny_2000"]["n_top"] == TOP_NODES < f["bunny_2000"]["n_nodes"]
    for name in ("cornell", "ship", "bunny_2000", "orphan_leaf", "one_triangle", "coplanar_pairs"):
        assert f[name]["walk_nested"] and f[name]["wide_ok"] and f[name]["leaf_cert_ok"], name
    assert not f["cornell"]["win_bad"] and f["cornell"]["ws0"] != 0
    assert not f["poking_child"]["walk_nested"] and not f["poking_child"]["wide_ok"] and f["poking_child"]["win_bad"]
    assert not f["link_fractional"]["walk_nested"]
    assert f["inverted_box"]["walk_nested"] and not f["inverted_box"]["wide_ok"]
    s = f["shrunk_leaves"]
    assert s["walk_nested"] and s["wide_ok"] and not s["leaf_cert_ok"] and s["win_bad"] and s["ws0"] == 0
    for name in ("tiny_coordinate", "huge_coordinate", "inverted_box"):
        assert f[name]["scene_fast"] == 0 and f["cornell"]["scene_fast"] == 1, name
    assert f["one_triangle"]["root_child"] == -1 and f["one_triangle"]["n_slots"] == 2
    assert f["cornell"]["root_child"] == 1
    for name in ("spheres_only", "empty"):
        assert f[name]["n_nodes"] == 0 and f[name]["root_child"] == -1 and not f[name]["walk_nested"], name
    assert any(f["fuzz_%d" % s]["n_nodes"] > TOP_NODES for s in range(9))


def test_top_numbering(packs):
    """A permutation with the root at 0; the first n_top device nodes are the breadth-first ones, and the node
    records are the reference's boxes under it."""
    for name, (_, f, bufs, _, pos, sc) in accepted(packs):
        n = f["n_nodes"]
        assert len(pos) == n, name
        if n == 0:
            continue
        assert pos[0] == 0 and sorted(pos) == list(range(n)), name
        nd = bufs["nodes"].reshape(-1, 8)
        ref = sc["nodes"]
        want = np.stack([ref[:, 0], ref[:, 4], ref[:, 1], ref[:, 5], ref[:, 2], ref[:, 6]], axis=1)
        assert np.array_equal(nd[pos, :6].view(np.uint32), want.view(np.uint32)), name
        if n > TOP_NODES:       # past the top set the original order is kept
            rest = [p for p in pos if p >= TOP_NODES]
            assert rest == sorted(rest), name


def _links(hi):
    return hi[:, 2].copy().view(np.int32), hi[:, 3].copy().view(np.int32)


def test_walk_images(packs):
    """Every link of every octant image lands on a node of that image or is the leaf / end code; the sink image's
    links land in it or on a sink; every sink links to itself; boxes are the device nodes' with the octant's axes
    swapped."""
    for name, (_, f, bufs, _, pos, sc) in accepted(packs):
        n, N, n_leaves = f["n_nodes"], f["walk_np"], f["n_slots"] // 2
        dn = bufs["nodes"].reshape(-1, 2, 4)
        a_dev, b_dev = _links(dn[:n, 1]) if n else (np.zeros(0, np.int32),) * 2
        for img, sinks in ((bufs["walk"], False), (bufs["walk_sink"], True)):
            if len(img) == 0:
                assert sinks and not f["walk_nested"], name
                continue
            sink0 = 16 * 2 * N * 8
            for k in range(8):
                base = 16 * 2 * N * k
                lo, hi = img[2 * N * k:2 * N * k + n], img[2 * N * k + N:2 * N * k + N + n]
                assert not img[2 * N * k + n:2 * N * k + N].any() and not img[2 * N * k + N + n:2 * N * (k + 1)].any(), name
                a, b = _links(hi)
                leaf = a_dev < 0
                # internal nodes: the hit link is the child's byte offset in this image
                assert np.array_equal(a[~leaf], base + 16 * a_dev[~leaf]) and (a_dev[~leaf] < n).all(), (name, k)
                code = ~a_dev[leaf]
                if sinks:
                    assert np.array_equal(a[leaf], sink0 + 16 * (1 + (code >> 2))), (name, k)
                    assert np.array_equal(b, np.where(b_dev >= 0, base + 16 * b_dev, sink0)), (name, k)
                else:
                    assert np.array_equal(a[leaf], -2 - code), (name, k)
                    assert np.array_equal(b, np.where(b_dev >= 0, base + 16 * b_dev, -1)), (name, k)
                assert ((code >> 2) < n_leaves).all() and (b_dev < n).all() and (b_dev >= -1).all(), name
                want_lo, want_hi = dn[:n, 0].copy(), dn[:n, 1, :2].copy()
                if k & 1:
                    want_lo[:, [0, 1]] = want_lo[:, [1, 0]]
                if k & 2:
                    want_lo[:, [2, 3]] = want_lo[:, [3, 2]]
                if k & 4:
                    want_hi = want_hi[:, ::-1]
                assert np.array_equal(lo.view(np.uint32), want_lo.view(np.uint32)), (name, k)
                assert np.array_equal(hi[:, :2].view(np.uint32), want_hi.view(np.uint32)), (name, k)
            if sinks:
                sk = img[16 * N + N:16 * N + N + n_leaves + 1]
                a, b = _links(sk)
                self = sink0 + 16 * np.arange(n_leaves + 1)
                assert np.array_equal(a, self) and np.array_equal(b, self) and not sk[:, :2].any(), name
                assert not img[16 * N:16 * N + N].any() and not img[16 * N + N + n_leaves + 1:].any(), name


def test_leaf_slots_and_continuations(packs):
    """Every leaf slot is written exactly once; a leaf's first triangle carries its miss link in image 0 (the LDS
    walk's continuation) and its second the leaf's own offset; the triangle quads are the reference's vertices."""
    for name, (_, f, bufs, _, pos, sc) in accepted(packs):
        n, N, n_leaves = f["n_nodes"], f["walk_np"], f["n_slots"] // 2
        ref, tris = sc["nodes"], sc["tris"]
        leaves = [i for i in range(n) if ref[i, 8] > -1.0]
        assert len(leaves) == n_leaves, name
        dn = bufs["nodes"].reshape(-1, 2, 4)
        dt = bufs["tris"].reshape(-1, 2, 4, 4)
        slots = []
        for i in leaves:
            j = int(pos[i])
            code = ~int(dn[j, 1, 2:3].copy().view(np.int32)[0])
            s = code >> 2
            slots.append(s)
            t0, t1 = int(ref[i, 8]), int(ref[i, 9])
            assert (code & 1) == (t0 == t1), name
            for h, t in ((0, t0), (1, t1)):
                assert np.array_equal(dt[s, h, 1:, :3].view(np.uint32), tris[t].reshape(4, 4)[:3, :3].view(np.uint32)), name
                assert int(dt[s, h, 2, 3:].copy().view(np.int32)[0]) == int(tris[t, 12]), name
            cop = bool(np.array_equal(dt[s, 0, 0], dt[s, 1, 0]))          # equal as floats: -0 == +0, NaN differs
            assert ((code >> 1) & 1) == cop, name
            hi0 = bufs["walk"][N + j]
            assert dt[s, 0, 1, 3:].tobytes() == hi0[3:].tobytes(), name            # the continuation word
            assert int(dt[s, 1, 3, 3:].copy().view(np.int32)[0]) == 16 * j, name
            if f["walk_nested"]:
                assert int(dt[s, 1, 1, 3:].copy().view(np.int32)[0]) == int(cop), name
        assert sorted(slots) == list(range(n_leaves)), name


def test_coplanar_flags(packs):
    """The signed-zero pair is flagged though its two plane quads differ in their bytes; the pair in two planes is
    not; the single-triangle leaf is flagged as its own copy."""
    _, f, bufs, _, pos, sc = packs["coplanar_pairs"]
    dn = bufs["nodes"].reshape(-1, 2, 4)
    dt = bufs["tris"].reshape(-1, 2, 4, 4)
    codes = [~int(dn[int(pos[i]), 1, 2:3].copy().view(np.int32)[0]) for i in (1, 2)]
    assert [c >> 2 for c in codes] == [0, 1] and [(c >> 1) & 1 for c in codes] == [1, 0]
    assert dt[0, 0, 0].tobytes() != dt[0, 1, 0].tobytes() and np.array_equal(dt[0, 0, 0], dt[0, 1, 0])
    _, f, bufs, _, pos, sc = packs["one_triangle"]
    assert ~int(bufs["nodes"].reshape(-1, 2, 4)[0, 1, 2:3].copy().view(np.int32)[0]) == 0b011


def test_wide_numbering(packs):
    """The wide-numbered node copy differs from the device nodes only in leaf codes, which carry distinct wide
    indices below n_wide with the same flags; the leaf's triangles sit at that index."""
    for name, (_, f, bufs, _, pos, sc) in accepted(packs):
        if not f["wide_ok"]:
            continue
        dn, dw = bufs["nodes"].reshape(-1, 8).view(np.uint32), bufs["wide_nodes"].reshape(-1, 8).view(np.uint32)
        keep = [c for c in range(8) if c != 6]
        assert np.array_equal(dn[:, keep], dw[:, keep]), name
        a, aw = dn[:, 6].view(np.int32), dw[:, 6].view(np.int32)
        leaf = a < 0
        assert np.array_equal(a[~leaf], aw[~leaf]) and (aw[leaf] < 0).all(), name
        moved = leaf & (np.arange(len(a)) < f["n_nodes"])
        if name == "orphan_leaf":                  # the appended leaf has no wide index: its code is left alone
            moved[int(pos[-1])] = False
        code, codew = ~a[moved], ~aw[moved]
        assert np.array_equal(code & 3, codew & 3), name
        g = codew >> 2
        assert len(set(g.tolist())) == len(g) and (g < f["n_wide"]).all(), name
        dt, dtw = bufs["tris"].reshape(-1, 8, 4), bufs["wide_tris"].reshape(-1, 8, 4)
        for q in (0, 2, 3, 4, 6):                  # the quads without a walk-image word
            assert np.array_equal(dt[code >> 2][:, q].view(np.uint32), dtw[g][:, q].view(np.uint32)), name
