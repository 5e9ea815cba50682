"""Reference compositions of the film tests (tests/test_film_host.py on the CPU, tests/test_gpu_film.py on the GPU;
DESIGN.md §15), in numpy binary32 and written from the definitions of include/pt_api.h: the moments folded from
per-frame colours, the guides put together from three display-mode images, the frames an exposure folds into the
guides.  `trace(camera, frame_first, n_frames, mode)` is whatever camera trace the caller holds to be right: the host
twin pt_trace_camera_host on the CPU, pt_trace_camera on contexts of display modes 2, 3 and 4 on the GPU -- code that
was there before the film."""
import numpy as np

f32 = np.float32


def luminance(c):
    return (c[..., 0] * f32(0.2126) + c[..., 1] * f32(0.7152)) + c[..., 2] * f32(0.0722)


def fold_moments(colours, prior=None):
    """(S1, S2) after the per-frame colours (each (H, W, 4)) in order, from `prior` (H, W, 2) or from zero."""
    h, w = colours[0].shape[:2]
    s1 = np.zeros((h, w), f32) if prior is None else prior[..., 0].copy()
    s2 = np.zeros((h, w), f32) if prior is None else prior[..., 1].copy()
    with np.errstate(all="ignore"):
        for c in colours:
            y = luminance(np.asarray(c, f32))
            s1 = (s1 + y).astype(f32)
            s2 = (s2 + y * y).astype(f32)
    return np.stack([s1, s2], -1)


def guides_of(trace, camera, frames):
    """N.rgb, Z, A.rgb, 0 per pixel from the images of display modes 2, 3 and 4 over frames 1..frames."""
    n, a, z = (trace(camera, 1, frames, mode) for mode in (2, 3, 4))
    g = np.zeros(n.shape[:2] + (8,), f32)
    g[..., 0:3], g[..., 3], g[..., 4:7] = n[..., :3], z[..., 0], a[..., :3]
    return g


def held_after(first, n, held, guide_frames):
    """guides_held after an exposure of frames first .. first + n - 1, by the header's rule."""
    last = first + n - 1
    if held < guide_frames and first <= held + 1 <= last:
        return min(guide_frames, last)
    return held


def words(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(words(got) != words(want))
    assert len(bad) == 0, "%s: %d of %d words differ, first at %s: got %s, want %s" % (
        what, len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
