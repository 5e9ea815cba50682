#!/usr/bin/env python3
"""What the noise estimate costs (profiles/noise_estimate.json): 1080p Cornell,
8 bounces, with the per-pixel moments off and on in one process, interleaved --
  * the C2 shape, one 1024-frame launch per render (ms per frame),
  * the one-dispatch-per-frame loop, 1,000 frames in flight (ms per frame),
then pt_noise's host round trip and pt_render_until runs in batches of 64 frames.
Host clock around work that ends in a device synchronise; every shape warmed first.

  python tools/noise_measure.py out.json
  PT_LIB=<older libptrace.so> PT_LIB_PARTIAL=1 python tools/noise_measure.py out.json --plain
--plain: the moments-off figures only (a library from before the feature, for the A/B)."""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "opengl-path-tracing_amd")]
import numpy as np  # noqa: E402
import pt_host as H  # noqa: E402
import pt_scenes  # noqa: E402

W, HH, B = 1920, 1080, 8


def make(sb, moments):
    pt = H.PathTracer(W, HH, max_bounce=B)
    pt.upload(sb)
    if moments:
        pt.set_moments(True)
    return pt


def long_launch(pt):
    t = time.perf_counter()
    pt.render(1, 1024, 0)
    return (time.perf_counter() - t) * 1e3 / 1024


def frame_loop(pt, frames=1000):
    t = time.perf_counter()
    for f in range(1, frames + 1):
        pt.render_async(f, 1, int(f > 1))
    pt.sync()
    return (time.perf_counter() - t) * 1e3 / frames


def main():
    out_path = sys.argv[1]
    plain = "--plain" in sys.argv[2:]
    sb = H.setupBuffers(*pt_scenes.write_scene("cornell", os.path.join(REPO, "scenes")))
    out = {"lib": os.path.relpath(H.LIB_PATH, REPO), "width": W, "height": HH, "bounces": B}
    modes = [False] if plain else [False, True]
    pts = {m: make(sb, m) for m in modes}
    for m in modes:                       # warm every shape
        long_launch(pts[m])
        long_launch(pts[m])
        frame_loop(pts[m], 300)
    for name, fn in (("long_launch", long_launch), ("frame_loop", frame_loop)):
        res = {m: [] for m in modes}
        for rep in range(6):              # interleaved, the order alternating
            for m in (modes if rep % 2 == 0 else modes[::-1]):
                res[m].append(round(fn(pts[m]), 5))
        for m in modes:
            out["%s_ms_per_frame_moments_%s" % (name, "on" if m else "off")] = res[m]
    if not plain:
        on, off = pts[True], pts[False]
        out["images_equal_bits"] = bool(np.array_equal(on.read_rgba32f().view(np.uint32),
                                                       off.read_rgba32f().view(np.uint32)))
        on.render(1, 64, 0)
        on.noise(0.05)
        t = time.perf_counter()
        for _ in range(200):
            s = on.noise(0.05)
        out["pt_noise_call_us"] = round((time.perf_counter() - t) * 1e6 / 200, 2)
        out["noise_after_64_frames"] = s
        for target in (0.1, 0.05):
            t = time.perf_counter()
            done, s = on.render_until(target, batch=64, max_frames=4096)
            dt = time.perf_counter() - t
            t = time.perf_counter()
            off.render(1, done, 0)
            out["render_until_%g" % target] = dict(batch=64, frames_done=done, seconds=round(dt, 4),
                                                   plain_render_same_frames_seconds=round(time.perf_counter() - t, 4),
                                                   stats=s)
    for p in pts.values():
        p.close()
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
