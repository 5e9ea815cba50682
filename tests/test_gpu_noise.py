"""The per-pixel noise estimate on the GPU (pt_api.h: pt_set_moments, pt_read_moments, pt_noise,
pt_render_until, pt_group_noise; ptrace --noise-target): the luminance moments the accumulate
pass keeps, the device reduction and the stop rule, against the oracle's per-frame colours
folded in by a numpy float32 restatement of the definition -- bit for bit, no tolerance.  In
every case the image must equal the same render with the moments off and the oracle's render.
Cornell box, 8 bounces."""
import json
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pt_host as H
from test_gpu_cli import EXE, read_pfm
from test_gpu_parity import assert_bitwise
from test_noise_host import q_numpy, stats_numpy

pytestmark = pytest.mark.gpu

f32 = np.float32
W, HH, B = 64, 48, 8
STAT_KEYS = ("pixels", "sum_q", "above", "max_q", "frames")


def frame_colours(sc, w, h, first, n, flags=0):
    """The oracle's colour of frames first .. first+n-1, one (h, w, 4) image each."""
    return [O.render(sc, w, h, max_bounce=B, frame_first=f, n_frames=1, acc_first=0, flags=flags)
            for f in range(first, first + n)]


def fold(colours):
    """(S1, S2) of the colours in order: the update of pt_api.h in numpy float32."""
    s1 = np.zeros(colours[0].shape[:2], f32)
    s2 = np.zeros_like(s1)
    for c in colours:
        y = (c[..., 0] * f32(0.2126) + c[..., 1] * f32(0.7152)) + c[..., 2] * f32(0.0722)
        s1 = s1 + y
        s2 = s2 + y * y
    return np.stack([s1, s2], axis=-1)


def same_bits(got, want, what):
    assert got.shape == want.shape, what
    bad = int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32)))
    assert bad == 0, "%s: %d of %d words differ" % (what, bad, got.size)


def stats_of(d):
    return {k: d[k] for k in STAT_KEYS}


@pytest.fixture(scope="module")
def colours64(cornell_scene):
    """Frames 1..64 at 64 x 48, rendered once for the module and never modified."""
    cs = frame_colours(cornell_scene, W, HH, 1, 64)
    for c in cs:
        c.setflags(write=False)
    return cs


def tracer(sc, w=W, h=HH, moments=True, **kw):
    pt = H.PathTracer(w, h, max_bounce=B, **kw)
    pt.upload(sc)
    if moments:
        pt.set_moments(True)
    return pt


def both(sc, run, w=W, h=HH, **kw):
    """run(pt) on a tracer with the moments on and on one with them off -> (the first tracer,
    still open; its image), after checking that the two images are the same bits."""
    on, off = tracer(sc, w, h, True, **kw), tracer(sc, w, h, False, **kw)
    run(on)
    run(off)
    img, img_off = on.read_rgba32f(), off.read_rgba32f()
    with pytest.raises(H.PTError) as e:
        off.noise(0.25)
    assert e.value.code == -6                       # PT_E_STATE: moments off
    off.close()
    same_bits(img, img_off, "image with moments on / off")
    return on, img


def test_long_launch_shape(cornell_scene):
    """61 x 37, 37 frames in one launch: the long accumulate shape's groups of 8 frames and a
    remainder of 5, a pixel count that is no multiple of the block's."""
    w, h, n = 61, 37, 37
    cs = frame_colours(cornell_scene, w, h, 1, n)
    want = fold(cs)
    pt, img = both(cornell_scene, lambda t: t.render(1, n, 0), w, h)
    mom, frames = pt.read_moments()
    got = pt.noise(0.25)
    pt.close()
    assert_bitwise(img, O.render(cornell_scene, w, h, max_bounce=B, n_frames=n), "image")
    assert frames == n
    same_bits(mom, want, "moments")
    assert stats_of(got) == stats_numpy(want[..., 0], want[..., 1], n, 0.25)
    assert stats_of(got) == stats_of(H.noise_host(mom, n, 0.25))
    assert got["pixels"] == w * h and 0 < got["above"] < w * h


def test_short_overlapped_launches(cornell_scene, colours64):
    """20 one-frame dispatches in flight on the overlap slots (key 9 automatic): the moments of
    one 20-frame render."""
    def run(t):
        for f in range(1, 21):
            t.render_async(f, 1, int(f > 1))
        t.sync()
    pt, img = both(cornell_scene, run)
    mom, frames = pt.read_moments()
    pt.render(1, 20, 0)
    mom_one, frames_one = pt.read_moments()
    pt.close()
    assert_bitwise(img, O.render(cornell_scene, W, HH, max_bounce=B, n_frames=20), "image")
    assert frames == frames_one == 20
    same_bits(mom, mom_one, "20 dispatches against one render")
    same_bits(mom, fold(colours64[:20]), "moments")


def test_reset_and_continue(cornell_scene, colours64):
    def run(t):
        t.render(1, 5, 0)
        t.render(6, 7, 1)
    pt, img = both(cornell_scene, run)
    mom, frames = pt.read_moments()
    assert_bitwise(img, O.render(cornell_scene, W, HH, max_bounce=B, n_frames=12), "image")
    assert frames == 12
    same_bits(mom, fold(colours64[:12]), "frames 1..5 then 6..12")
    pt.render(1, 3, 0)                       # a reset restarts the count and the moments
    mom, frames = pt.read_moments()
    assert frames == 3
    same_bits(mom, fold(colours64[:3]), "after a reset")
    pt.dispatch(1, 0)                        # one frame: too few for an estimate
    with pytest.raises(H.PTError) as e:
        pt.noise(0.25)
    assert e.value.code == -6
    assert pt.read_moments()[1] == 1
    pt.close()


@pytest.mark.parametrize("key", ["scratch_mib", "group"])
def test_split_renders(cornell_scene, colours64, key):
    """Key 8 = 1 MiB: 40 frames (36,864 B of colours each) take two launches.  Key 5 = 64, at
    least the frame count: one item per pixel, which the moments keep in split mode."""
    def run(t):
        t.set_tuning(**{key: 1 if key == "scratch_mib" else 64})
        t.render(1, 40, 0)
    pt, img = both(cornell_scene, run)
    mom, frames = pt.read_moments()
    pt.close()
    assert_bitwise(img, O.render(cornell_scene, W, HH, max_bounce=B, n_frames=40), "image")
    assert frames == 40
    same_bits(mom, fold(colours64[:40]), "moments")


def test_graph(cornell_scene, colours64):
    def run(t):
        t.progressive_setup(4, 2)
        t.progressive_reset(1)
        t.progressive_run(3)
    pt, img = both(cornell_scene, run)
    mom, frames = pt.read_moments()
    assert_bitwise(img, O.render(cornell_scene, W, HH, max_bounce=B, n_frames=24), "image")
    assert frames == 24
    same_bits(mom, fold(colours64[:24]), "3 replays")
    assert stats_of(pt.noise(0.25)) == stats_numpy(mom[..., 0], mom[..., 1], 24, 0.25)
    pt.progressive_reset(1)
    pt.progressive_run(1)
    mom, frames = pt.read_moments()
    img = pt.read_rgba32f()
    pt.close()
    assert frames == 8
    same_bits(mom, fold(colours64[:8]), "a replay from frame 1")
    assert_bitwise(img, O.render(cornell_scene, W, HH, max_bounce=B, n_frames=8), "image after the reset")


def test_footprint_and_rows(cornell_scene, colours64):
    """PT_FLAG_REF_DISPATCH leaves 60 columns and 40 rows of 64 x 48: moments outside stay 0 and
    are not counted; two row-split contexts add up to the single context's summary.  (The
    oracle renders every pixel: the footprint is cut out of its colours here.)"""
    n, flag = 6, H.PT_FLAG_REF_DISPATCH
    mask = np.zeros((HH, W), np.uint8)
    mask[:40, :60] = 1
    want = fold(colours64[:n]) * mask[..., None].astype(f32)
    pt, img = both(cornell_scene, lambda t: t.render(1, n, 0), flags=flag)
    mom, _ = pt.read_moments()
    one = pt.noise(0.25)
    pt.close()
    want_img = O.render(cornell_scene, W, HH, max_bounce=B, n_frames=n) * mask[..., None].astype(f32)
    assert_bitwise(img, want_img, "image")
    same_bits(mom, want, "moments")
    assert one["pixels"] == 60 * 40
    assert stats_of(one) == stats_numpy(want[..., 0], want[..., 1], n, 0.25, mask)
    assert stats_of(one) == stats_of(H.noise_host(mom, n, 0.25, mask))

    trs = [H.PathTracer(W, HH, max_bounce=B, flags=flag, rank=r, world=2) for r in (0, 1)]
    g = H.Group(trs)
    g.upload(cornell_scene)
    for t in trs:
        t.set_moments(True)
        t.render_async(1, n, 0)
    whole = g.noise(0.25)
    parts = [t.read_moments()[0] for t in trs]
    trs[1].render(n + 1, 1, 1)               # unequal frame counts: no summary of the image
    with pytest.raises(H.PTError) as e:
        g.noise(0.25)
    g.close()
    for t in trs:
        t.close()
    assert e.value.code == -6
    assert stats_of(whole) == stats_of(one)
    for r in (0, 1):
        same_bits(parts[r], np.ascontiguousarray(want[r::2]), "rank %d" % r)


def stop_batch(colours, batch, max_frames, target):
    """The first multiple of `batch` at which the mean relative error meets the target."""
    for n in range(batch, max_frames + 1, batch):
        m = fold(colours[:n])
        s = stats_numpy(m[..., 0], m[..., 1], n, target)
        print("frames %d: mean relative error %.4f" % (n, s["sum_q"] / s["pixels"] / 65536.0))
        if s["sum_q"] <= int(f32(target) * f32(65536.0)) * s["pixels"]:
            return n, s
    return max_frames, s


@pytest.fixture(scope="module")
def stop64(colours64):
    """Where batches of 8 up to 64 frames stop for a target of 0.25, from the oracle's colours."""
    return stop_batch(colours64, 8, 64, 0.25)


def test_render_until(cornell_scene, colours64, stop64):
    want_n, want_s = stop64
    assert 8 < want_n < 64                       # the stop falls away from both ends
    pt = tracer(cornell_scene, moments=False)    # render_until turns the moments on
    done, s = pt.render_until(0.25, batch=8, max_frames=64)
    img = pt.read_rgba32f()
    assert done == want_n and stats_of(s) == want_s
    assert_bitwise(img, O.render(cornell_scene, W, HH, max_bounce=B, n_frames=done), "image")
    same_bits(pt.read_moments()[0], fold(colours64[:done]), "moments")
    # a target no render meets stops at max_frames; the last batch is shorter
    done, s = pt.render_until(1e-6, batch=8, max_frames=20)
    assert done == 20 and s["frames"] == 20
    assert_bitwise(pt.read_rgba32f(), O.render(cornell_scene, W, HH, max_bounce=B, n_frames=20), "image at max_frames")
    for bad in (dict(batch=1), dict(batch=8, max_frames=7), dict(target=0.0), dict(target=-1.0)):
        kw = dict(dict(target=0.25, batch=8, max_frames=64), **bad)
        with pytest.raises(H.PTError) as e:
            pt.render_until(**kw)
        assert e.value.code == -1                # PT_E_ARG
    pt.close()


def test_cli_noise_target(tmp_path, cornell_paths, cornell_scene, stop64):
    want_n, want_s = stop64
    pfm = str(tmp_path / "out.pfm")
    common = [EXE, *cornell_paths, "--width", str(W), "--height", str(HH), "--bounces", str(B), "--noise-target", "0.25",
              "--batch", "8", "--max-spp", "64", "--json", "--pfm", pfm, "--ppm", str(tmp_path / "out.ppm")]
    out = subprocess.run(common, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    summary = json.loads(out.stdout.strip().splitlines()[-1])
    assert summary["frames_done"] == summary["frames"] == want_n
    assert abs(summary["noise_mean"] - want_s["sum_q"] / want_s["pixels"] / 65536.0) < 1e-7
    assert abs(summary["noise_max"] - want_s["max_q"] / 65536.0) < 1e-7
    assert abs(summary["noise_above_frac"] - want_s["above"] / want_s["pixels"]) < 1e-7
    want = O.render(cornell_scene, W, HH, max_bounce=B, n_frames=want_n)
    same_bits(np.ascontiguousarray(read_pfm(pfm)), np.ascontiguousarray(want[..., :3]), "PFM")
    ck = tmp_path / "none.ptck"
    for extra in (["--gpus", "2"], ["--resume", str(ck)], ["--events", str(ck)]):
        bad = subprocess.run(common + extra, capture_output=True, text=True, timeout=120)
        assert bad.returncode != 0 and "--noise-target" in bad.stderr, extra
