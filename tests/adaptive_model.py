"""The batch loop of pt_render_adaptive (include/pt_api.h) restated in numpy: which
work-queue tile receives how many frames, and the call's summary, from per-frame colours alone.
Nothing here comes from the library: the colours are the oracle's, the moments are
test_gpu_noise.fold's float32 sums and q is test_noise_host.q_numpy."""
import numpy as np

from test_noise_host import q_numpy

f32 = np.float32


def luminance_sums(colours):
    """Cumulative (S1, S2) after each colour, in order: sums[k] = the moments of colours[:k]
    (test_gpu_noise.fold's update, kept per prefix)."""
    s1 = np.zeros(colours[0].shape[:2], f32)
    s2 = np.zeros_like(s1)
    sums = [np.stack([s1, s2], axis=-1)]
    for c in colours:
        y = (c[..., 0] * f32(0.2126) + c[..., 1] * f32(0.7152)) + c[..., 2] * f32(0.0722)
        s1 = s1 + y
        s2 = s2 + y * y
        sums.append(np.stack([s1, s2], axis=-1))
    return sums


def tile_grid(width, rows, shift):
    """(tile width, tile height, tiles_x, tiles_y) of tuning key 20 = shift + 1."""
    tw, th = 8 << shift, 8 >> shift
    return tw, th, -(-width // tw), -(-rows // th)


def target_q(target):
    t = min(max(f32(target), f32(0.0)), f32(64.0))
    return int(f32(t) * f32(65536.0))


def run(colours, width, rows, shift, batch, max_frames, target, mask=None, n0=0):
    """colours: the per-frame colours (rows, width, 4) of the n0 frames already in the moments
    followed by the call's frames, in order.  mask: the footprint (rows, width), nonzero = inside.
    -> dict(frames_done, frames: (tiles_y, tiles_x) frames per tile, pixel_frames: (rows, width)
    frames per pixel, stats: every pt_adaptive_stats field, moments: (rows, width, 2) expected
    moments, footprint pixels only)."""
    tw, th, tiles_x, tiles_y = tile_grid(width, rows, shift)
    mask = np.ones((rows, width), bool) if mask is None else np.asarray(mask) != 0
    sums = luminance_sums(colours[: n0 + max_frames])
    tq = target_q(target)
    frames = np.zeros((tiles_y, tiles_x), np.int64)
    tile_q = {}
    active = []
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            sl = (slice(ty * th, min((ty + 1) * th, rows)), slice(tx * tw, min((tx + 1) * tw, width)))
            if mask[sl].any():
                active.append((ty, tx, sl))
    n_tiles = len(active)
    done = 0
    while done < max_frames and active:
        done += min(batch, max_frames - done)
        n = n0 + done
        stay = []
        for ty, tx, sl in active:
            m = sums[n][sl]
            q = q_numpy(m[..., 0], m[..., 1], n).astype(np.uint64)[mask[sl]]
            frames[ty, tx] = done
            tile_q[(ty, tx)] = q
            if int(q.sum()) > tq * q.size:
                stay.append((ty, tx, sl))
        active = stay
    per_pixel = np.repeat(np.repeat(frames, th, axis=0), tw, axis=1)[:rows, :width] * mask
    allq = np.concatenate(list(tile_q.values())) if tile_q else np.zeros(0, np.uint64)
    stats = dict(pixels=int(allq.size), sum_q=int(allq.sum()), above=int(np.count_nonzero(allq > tq)),
                 max_q=int(allq.max()) if allq.size else 0, frames=n0 + done, tiles=n_tiles, tiles_active=len(active),
                 pixel_frames=int(per_pixel.sum()))
    moments = np.zeros((rows, width, 2), f32)
    for f in np.unique(per_pixel[mask]):
        pick = mask & (per_pixel == f)
        moments[pick] = sums[n0 + int(f)][pick]
    return dict(frames_done=done, frames=frames, pixel_frames=per_pixel, stats=stats, moments=moments)


def compose(per_pixel, image_of, base=None):
    """The expected image: pixel (y, x) from image_of(f) with f = per_pixel[y, x] frames; pixels
    with f = 0 keep `base` (zeros when None)."""
    out = None
    for f in np.unique(per_pixel):
        if f == 0:
            continue
        img = image_of(int(f))
        if out is None:
            out = np.zeros_like(img) if base is None else np.array(base, f32)
        out[per_pixel == f] = img[per_pixel == f]
    if out is None:
        out = np.array(base, f32)
    return out
