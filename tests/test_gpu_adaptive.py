"""Adaptive sampling on the GPU (pt_api.h: pt_render_adaptive, pt_read_tile_frames; ptrace
--adaptive) against the numpy restatement of its batch loop
(tests/adaptive_model.py) on the oracle's per-frame colours.  Every case checks four things, bit
for bit: the per-tile frame map is the model's, the image is the oracle's render of f frames in
every tile that received f, the moments are fold(colours[:f]) there, and every pt_adaptive_stats
field is the model's.  Cornell box, 8 bounces, unless a case says otherwise."""
import json
import subprocess

import numpy as np
import pytest

import adaptive_model as M
import oracle_lib as O
import pt_host as H
from test_gpu_cli import EXE, read_pfm
from test_gpu_noise import fold, frame_colours, same_bits
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu

f32 = np.float32
W, HH, B = 64, 48, 8
STAT_KEYS = ("pixels", "sum_q", "above", "max_q", "frames", "tiles", "tiles_active", "pixel_frames")


@pytest.fixture(scope="module")
def colours64(cornell_scene):
    """Frames 1..64 at 64 x 48, rendered once for the module and never modified."""
    cs = frame_colours(cornell_scene, W, HH, 1, 64)
    for c in cs:
        c.setflags(write=False)
    return cs


@pytest.fixture(scope="module")
def images64(cornell_scene):
    """f -> the oracle's 64 x 48 render of frames 1..f, each rendered once."""
    cache = {}

    def image_of(f):
        if f not in cache:
            cache[f] = O.render(cornell_scene, W, HH, max_bounce=B, n_frames=f)
            cache[f].setflags(write=False)
        return cache[f]
    return image_of


def tracer(sc, w=W, h=HH, max_bounce=B, **kw):
    pt = H.PathTracer(w, h, max_bounce=max_bounce, **kw)
    pt.upload(sc)
    return pt


def check(pt, got, want, image_of, what, base_image=None, base_moments=None):
    """got = render_adaptive's (frames_done, stats); want = adaptive_model.run's result."""
    done, stats = got
    frames = pt.tile_frames()
    print(what, "frames per tile:", dict(zip(*np.unique(frames, return_counts=True))), stats)
    assert np.array_equal(frames, want["frames"]), what + ": frame map"
    assert done == want["frames_done"], what
    assert {k: stats[k] for k in STAT_KEYS} == want["stats"], what
    assert_bitwise(pt.read_rgba32f(), M.compose(want["pixel_frames"], image_of, base_image), what + ": image")
    mom, n = pt.read_moments()
    assert n == want["stats"]["frames"], what
    want_mom = want["moments"] if base_moments is None else np.where(want["pixel_frames"][..., None] > 0, want["moments"], base_moments)
    same_bits(mom, want_mom, what + ": moments")


def test_base(cornell_scene, colours64, images64):
    want = M.run(colours64, W, HH, 0, 8, 64, 0.25)
    assert len(np.unique(want["frames"])) >= 4 and want["stats"]["tiles_active"] >= 1   # (tests/test_adaptive_model.py)
    pt = tracer(cornell_scene)                   # render_adaptive turns the moments on
    check(pt, pt.render_adaptive(0.25, batch=8, max_frames=64), want, images64, "base")
    # the same call again restarts: the same result, not a continuation
    check(pt, pt.render_adaptive(0.25, batch=8, max_frames=64), want, images64, "base, again")
    pt.close()


def test_partial_tiles(cornell_scene):
    """61 x 37: partial tiles on both edges, a pixel count that is no multiple of 64."""
    w, h = 61, 37
    cs = frame_colours(cornell_scene, w, h, 1, 40)
    for shift in (0, 2):
        want = M.run(cs, w, h, shift, 8, 40, 0.25)
        pt = tracer(cornell_scene, w, h)
        pt.set_key(20, shift + 1)
        check(pt, pt.render_adaptive(0.25, batch=8, max_frames=40), want,
              lambda f: O.render(cornell_scene, w, h, max_bounce=B, n_frames=f), "61 x 37, shape %d" % (shift + 1))
        pt.close()


@pytest.mark.parametrize("key", [1, 2, 3, 4])
def test_tile_shapes(cornell_scene, colours64, images64, key):
    """Tuning key 20: 8 x 8, 16 x 4, 32 x 2 and 64 x 1 tiles (the last: every tile row differs)."""
    want = M.run(colours64, W, HH, key - 1, 8, 64, 0.25)
    assert want["frames"].shape == (HH // (8 >> (key - 1)), W // (8 << (key - 1)))
    pt = tracer(cornell_scene)
    pt.set_key(20, key)
    check(pt, pt.render_adaptive(0.25, batch=8, max_frames=64), want, images64, "key 20 = %d" % key)
    pt.close()


@pytest.mark.parametrize("batch, max_frames", [(8, 60), (24, 64), (5, 23)])
def test_batches(cornell_scene, colours64, images64, batch, max_frames):
    """A short last batch (60 = 7 x 8 + 4); batches of 24 (three load groups of 8 frames) with a
    last one of 16; batches of 5 (no full load group) with a last one of 3."""
    want = M.run(colours64, W, HH, 0, batch, max_frames, 0.25)
    pt = tracer(cornell_scene)
    check(pt, pt.render_adaptive(0.25, batch=batch, max_frames=max_frames), want, images64, "batch %d to %d" % (batch, max_frames))
    pt.close()


def test_long_list(cornell_scene):
    """1024 x 512: 8,192 tiles, the shortest list whose pass gives a wave more than one tile
    (adapt_tiles_per_wave: two in turn), over many blocks that each reserve a stretch of the
    next list.  Batches of 2 up to 6 frames."""
    w, h = 1024, 512
    cs = frame_colours(cornell_scene, w, h, 1, 6)
    want = M.run(cs, w, h, 0, 2, 6, 0.5)
    assert want["stats"]["tiles"] == 8192 and len(np.unique(want["frames"])) == 3
    assert 0 < want["stats"]["tiles_active"] < 8192
    pt = tracer(cornell_scene, w, h)
    check(pt, pt.render_adaptive(0.5, batch=2, max_frames=6), want,
          lambda f: O.render(cornell_scene, w, h, max_bounce=B, n_frames=f), "8,192 tiles")
    pt.close()


def test_everything_retires_at_once(cornell_scene, colours64, images64):
    want = M.run(colours64, W, HH, 0, 8, 64, 64.0)
    assert want["frames_done"] == 8 and want["stats"]["tiles_active"] == 0
    pt, other = tracer(cornell_scene), tracer(cornell_scene)
    check(pt, pt.render_adaptive(64.0, batch=8, max_frames=64), want, images64, "target 64")
    done, s = other.render_until(64.0, batch=8, max_frames=64)
    assert done == 8
    same_bits(pt.read_rgba32f(), other.read_rgba32f(), "the image of pt_render_until")
    pt.close()
    other.close()


def test_nothing_retires(cornell_scene, colours64, images64):
    want = M.run(colours64, W, HH, 0, 8, 28, 1e-6)
    assert want["frames_done"] == 28 and want["stats"]["tiles_active"] == want["stats"]["tiles"] == 48
    pt, other = tracer(cornell_scene), tracer(cornell_scene)
    check(pt, pt.render_adaptive(1e-6, batch=8, max_frames=28), want, images64, "target 1e-6")
    other.set_moments(True)
    other.render(1, 28, 0)
    same_bits(pt.read_rgba32f(), other.read_rgba32f(), "the image of pt_render(1, 28, 0)")
    same_bits(pt.read_moments()[0], other.read_moments()[0], "the moments of pt_render(1, 28, 0)")
    pt.close()
    other.close()


def test_footprint(cornell_scene, colours64, images64):
    """PT_FLAG_REF_DISPATCH leaves 60 x 40 of 64 x 48: the tiles of row 5 are empty (frame count
    0), column 7's tiles hold 4 of their 8 columns; nothing outside the footprint is touched."""
    mask = np.zeros((HH, W), np.uint8)
    mask[:40, :60] = 1
    want = M.run(colours64, W, HH, 0, 8, 64, 0.25, mask=mask)
    assert (want["frames"][5] == 0).all() and (want["frames"][:5] > 0).all() and want["stats"]["pixels"] == 2400
    pt = tracer(cornell_scene, flags=H.PT_FLAG_REF_DISPATCH)
    pt.set_moments(True)
    marker = np.full((HH, W, 4), 7.5, f32)
    pt.write_rgba32f(marker)                     # what lies outside the footprint must stay
    check(pt, pt.render_adaptive(0.25, batch=8, max_frames=64), want, images64, "footprint", base_image=marker)
    pt.close()


@pytest.mark.parametrize("rank", [0, 1])
def test_row_split(cornell_scene, colours64, images64, rank):
    """A context of a two-way row split decides on its own local rows (24 of them: 3 tile rows)."""
    cs = [np.ascontiguousarray(c[rank::2]) for c in colours64]
    want = M.run(cs, W, HH // 2, 0, 8, 64, 0.25)
    pt = tracer(cornell_scene, rank=rank, world=2)
    check(pt, pt.render_adaptive(0.25, batch=8, max_frames=64), want, lambda f: images64(f)[rank::2], "rank %d of 2" % rank)
    pt.close()


def test_continue_after_plain_render(cornell_scene, colours64, images64):
    """accumulate_first = 1 after a plain 8-frame render with the moments on: n0 = 8, the call's
    frames are 9..64, and a tile that received f of them holds the render of frames 1..8+f."""
    want = M.run(colours64, W, HH, 0, 8, 56, 0.25, n0=8)
    assert want["stats"]["frames"] == 64 and len(np.unique(want["frames"])) >= 3
    pt = tracer(cornell_scene)
    pt.set_moments(True)
    pt.render(1, 8, 0)
    got = pt.render_adaptive(0.25, batch=8, max_frames=56, frame_first=9, accumulate_first=1)
    check(pt, got, want, lambda f: images64(8 + f), "n0 = 8")
    pt.close()


def test_rays_per_pixel(cornell_scene):
    cs = [O.render(cornell_scene, W, HH, max_bounce=B, frame_first=f, n_frames=1, acc_first=0, rpp=3) for f in range(1, 33)]
    want = M.run(cs, W, HH, 0, 8, 32, 0.15)
    assert len(np.unique(want["frames"])) >= 3
    pt = tracer(cornell_scene, rays_per_pixel=3)
    check(pt, pt.render_adaptive(0.15, batch=8, max_frames=32), want,
          lambda f: O.render(cornell_scene, W, HH, max_bounce=B, n_frames=f, rpp=3), "3 rays per pixel")
    pt.close()


def test_global_memory_kernel(cornell_scene, colours64, images64):
    """pt_set_kernel(3): the scene stays in global memory."""
    want = M.run(colours64, W, HH, 0, 8, 40, 0.25)
    pt = tracer(cornell_scene)
    pt.set_kernel(3)
    check(pt, pt.render_adaptive(0.25, batch=8, max_frames=40), want, images64, "kernel variant 3")
    pt.close()


def test_wide_walk_scene():
    """fuzz_scenes seed 16: 2,500 triangles, too large for LDS, on the wide global-memory walk, at
    its own image size (31 x 14), camera and frame numbers; shaded, 3 bounces."""
    import fuzz_scenes
    sc, kw = fuzz_scenes.random_case(16)
    assert len(sc["tris"]) == 2500
    w, h, flags, first, mb = kw["W"], kw["H"], kw["flags"], kw["frame_first"], 3
    cs = [O.render(sc, w, h, max_bounce=mb, frame_first=f, n_frames=1, acc_first=0, flags=flags) for f in range(first, first + 24)]
    want = M.run(cs, w, h, 0, 4, 24, 0.2)
    assert len(np.unique(want["frames"])) >= 3 and want["stats"]["tiles_active"] >= 1
    pt = tracer(sc, w, h, max_bounce=mb, flags=flags)
    got = pt.render_adaptive(0.2, batch=4, max_frames=24, frame_first=first)
    check(pt, got, want, lambda f: O.render(sc, w, h, max_bounce=mb, frame_first=first, n_frames=f, flags=flags), "wide walk")
    pt.close()


def test_non_interference(cornell_scene, colours64, images64):
    pt = tracer(cornell_scene)
    pt.render(1, 64, 0)                          # learns a tile order
    before = pt.tile_order()
    pt.render_adaptive(0.25, batch=8, max_frames=64)
    after = pt.tile_order()
    assert after["sorts"] == before["sorts"] and np.array_equal(after["perm"], before["perm"])
    with pytest.raises(H.PTError) as e:
        pt.noise(0.25)
    assert e.value.code == -6                    # PT_E_STATE: per-tile counts
    with pytest.raises(H.PTError) as e:
        pt.render_adaptive(0.25, batch=8, max_frames=16, frame_first=65, accumulate_first=1)
    assert e.value.code == -6
    with pytest.raises(H.PTError) as e:
        pt.render_until(0.25, batch=8, max_frames=16, frame_first=65, accumulate_first=1)
    assert e.value.code == -6
    assert pt.read_moments()[1] == 64            # the largest count
    # a plain restarting render: the oracle's image, a uniform count, pt_noise answers again
    pt.render(1, 20, 0)
    assert_bitwise(pt.read_rgba32f(), images64(20), "pt_render(1, 20, 0) after an adaptive run")
    mom, n = pt.read_moments()
    assert n == 20
    same_bits(mom, fold(colours64[:20]), "moments after the restart")
    assert pt.noise(0.25)["frames"] == 20
    order = pt.tile_order()
    flat = order["perm"][:, 0] * order["tiles_x"] + order["perm"][:, 1]
    assert sorted(flat.tolist()) == list(range(order["n_tiles"]))
    assert order["sorts"] == before["sorts"] + 1         # the 20-frame render's sort alone
    # a change of tile shape drops the map: all zero until the next adaptive call
    pt.set_key(20, 2)
    assert pt.tile_frames().shape == (12, 4) and not pt.tile_frames().any()
    pt.close()


def test_launch_counts_of_plain_renders(cornell_scene):
    """A context that never calls the new entry points launches what it did before they existed:
    the first render and the cold 64-frame render's probe on the generic line, everything after
    the first sort on the specialised line (pt_debug_launches)."""
    pt = tracer(cornell_scene)
    pt.render(1, 1, 0)
    assert pt.launches() == (1, 0)
    pt.render(1, 64, 0)
    assert pt.launches() == (2, 1)
    pt.render(1, 20, 0)
    for f in range(21, 24):
        pt.dispatch(f, 1)
    assert pt.launches() == (2, 5)
    pt.close()


def test_errors(cornell_scene):
    pt = H.PathTracer(W, HH, max_bounce=B)
    with pytest.raises(H.PTError) as e:
        pt.render_adaptive(0.25, batch=8, max_frames=64)
    assert e.value.code == -6                    # PT_E_STATE: no scene yet
    pt.upload(cornell_scene)
    for bad in (dict(batch=1), dict(batch=8, max_frames=7), dict(target=0.0), dict(target=-1.0), dict(target=float("nan"))):
        kw = dict(dict(target=0.25, batch=8, max_frames=64), **bad)
        with pytest.raises(H.PTError) as e:
            pt.render_adaptive(**kw)
        assert e.value.code == -1                # PT_E_ARG
    assert pt.tile_frames().shape == (6, 8) and not pt.tile_frames().any()
    n, tx = H.C.c_int(), H.C.c_int()
    small = np.zeros(47, np.uint32)
    assert H.lib().pt_read_tile_frames(pt.h, small.ctypes.data, 47, H.C.byref(n), H.C.byref(tx)) == -1
    assert H.lib().pt_read_tile_frames(pt.h, None, 0, H.C.byref(n), H.C.byref(tx)) == 0
    assert (n.value, tx.value) == (48, 8)
    pt.close()


def test_cli(tmp_path, cornell_paths, cornell_scene, colours64, images64):
    want = M.run(colours64, W, HH, 0, 8, 64, 0.25)
    pfm, pgm = str(tmp_path / "out.pfm"), str(tmp_path / "spp.pgm")
    common = [EXE, *cornell_paths, "--width", str(W), "--height", str(HH), "--bounces", str(B), "--noise-target", "0.25",
              "--batch", "8", "--max-spp", "64", "--json", "--pfm", pfm, "--ppm", str(tmp_path / "out.ppm")]
    out = subprocess.run(common + ["--adaptive", "--spp-map", pgm], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    summary = json.loads(out.stdout.strip().splitlines()[-1])
    s = want["stats"]
    assert summary["frames_done"] == summary["frames"] == want["frames_done"]
    assert (summary["tiles"], summary["tiles_active"], summary["pixel_frames"]) == (s["tiles"], s["tiles_active"], s["pixel_frames"])
    assert abs(summary["noise_mean"] - s["sum_q"] / s["pixels"] / 65536.0) < 1e-7
    assert abs(summary["noise_max"] - s["max_q"] / 65536.0) < 1e-7
    assert abs(summary["noise_above_frac"] - s["above"] / s["pixels"]) < 1e-7
    img = M.compose(want["pixel_frames"], images64)
    same_bits(np.ascontiguousarray(read_pfm(pfm)), np.ascontiguousarray(img[..., :3]), "PFM")
    with open(pgm, "rb") as f:
        assert f.readline().strip() == b"P5"
        tx, ty = (int(v) for v in f.readline().split())
        assert int(f.readline()) == 255              # no count above 255: 8-bit samples
        data = np.frombuffer(f.read(), np.uint8).reshape(ty, tx)
    assert np.array_equal(data[::-1], want["frames"])        # PGM rows run top to bottom
    # counts above 255 make a 16-bit map: one 8 x 8 tile that never retires, 2 batches of 132 frames
    cs8 = frame_colours(cornell_scene, 8, 8, 1, 264)
    want8 = M.run(cs8, 8, 8, 0, 132, 264, 1e-6)
    assert want8["frames"].tolist() == [[264]]
    out = subprocess.run([EXE, *cornell_paths, "--width", "8", "--height", "8", "--bounces", str(B), "--noise-target", "1e-6",
                          "--batch", "132", "--max-spp", "264", "--adaptive", "--spp-map", pgm, "--pfm", pfm,
                          "--ppm", str(tmp_path / "out.ppm")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    with open(pgm, "rb") as f:
        assert f.read() == b"P5\n1 1\n65535\n" + bytes([264 >> 8, 264 & 255])
    ck = tmp_path / "none.ptck"
    for extra in (["--adaptive", "--gpus", "2"], ["--adaptive", "--resume", str(ck)], ["--adaptive", "--events", str(ck)]):
        bad = subprocess.run(common + extra, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--noise-target" in bad.stderr, extra
    plain = [a for a in common if a not in ("--noise-target", "0.25")]
    for extra, word in ((["--adaptive"], "--adaptive"), (["--spp-map", pgm], "--spp-map")):
        bad = subprocess.run(plain + extra, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and word in bad.stderr, extra
