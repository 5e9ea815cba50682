#!/usr/bin/env python3
"""What a film costs over the plain camera trace, and where its moments should live (DESIGN.md §15.4;
profiles/film.json): pt_film_expose at 1920 x 1080, max_bounce 8, thin lens, 8 frames per call, on Cornell and the
69k-triangle stand-in.  From HIP events on the context stream: the median, and the range, of --reps repetitions after 2
warm-ups.

  yardstick        pt_trace_camera_device on the same camera, in the same process
  regs             (a) the moments in registers beside the running mean, stored with the pixel
  global           (b) the moments read and written in global memory at each path end
                   both through pt__film_debug (an internal entry point), on a film whose guides are complete, so that
                   the exposure folds none; timed as yardstick, (a), (b) and then again as (b), (a), yardstick
                   ("other_order")
  with_guides      the shipped variant when the call also folds the guide frames 1..4 (pt_film_set_camera before each
                   repetition)
  denoise          pt_film_denoise, 5 iterations, guides complete; and guides_only: the same after pt_film_set_camera,
                   so that it gathers the 4 guide frames by a guides-only launch first
  noise            pt_film_noise (wall-clock: it waits)

The `resources` mode needs no GPU: it compiles csrc/pt_film_kernels.hip for gfx950 with the compiler's resource
remarks and records each kernel's registers, scratch, LDS and occupancy.

  python tools/film_measure.py resources out.json
  python tools/film_measure.py gpu out.json [--reps 5] [--scenes cornell,bunny]
Both modes update out.json in place.
"""
import json
import os
import re
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "opengl-path-tracing_amd")
sys.path[:0] = [PKG, os.path.join(REPO, "tools")]

from camera_measure import timed  # noqa: E402  (the same events, warm-ups and statistics)
from query_measure import Hip, load, save, scene  # noqa: E402

W, HH = 1920, 1080
MAX_BOUNCE = 8
FRAMES = 8
GUIDE_FRAMES = 4
MOMENTS = 1                               # ptfilm::Debug (csrc/pt_film_launch.h)
VARIANTS = {"regs": 1, "global": 2}


def resources():
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(PKG, "csrc", "pt_film_kernels.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            t = re.search(r"k_film_exposeILb([01])E", name)
            if t:
                name = "k_film_expose<%s>" % ("regs" if t.group(1) == "1" else "global")
            else:
                name = next((k for k in ("k_film_noise", "k_film_aces") if k in name), name)
            cur = kernels.setdefault(name, {})
            continue
        m = re.search(r"remark: \s*(VGPRs|AGPRs|SGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return dict(kernels=kernels)


def gpu(reps, names):
    import pt_host as H
    L = H.lib()
    hip = Hip(L)
    doc = dict(width=W, height=HH, pixels=W * HH, reps=reps, max_bounce=MAX_BOUNCE, frames=FRAMES, guide_frames=GUIDE_FRAMES,
               unit="ms per call (median; ms_range: the repetitions' least and greatest time)", scenes={})
    for name in names:
        sb = scene(H, name)
        pt = H.PathTracer(W, HH, max_bounce=MAX_BOUNCE)
        pt.upload(sb)
        cam = H.Camera("thinlens", W, HH, sb["cam"], aperture=0.05, focus=6.0)
        film = H.Film(pt, cam, GUIDE_FRAMES)
        film.expose(1, FRAMES, 0)                                     # the guides complete
        pt.sync()
        assert film.info() == (FRAMES, GUIDE_FRAMES)
        d_rgba = hip.alloc(W * HH * 16)
        row = dict(triangles=len(sb["tris"]), nodes=len(sb["nodes"]))

        def variant(which):
            assert L.pt__film_debug(MOMENTS, VARIANTS[which]) == 0
            return timed(hip, pt, lambda: film.expose(1, FRAMES, 0), reps)

        yard = lambda: timed(hip, pt, lambda: pt.trace_camera_device(cam, d_rgba.value, 1, FRAMES, 0), reps)
        first = dict(yardstick=yard(), regs=variant("regs"))
        first["global"] = variant("global")
        again = {"global": variant("global")}
        again["regs"] = variant("regs")
        again["yardstick"] = yard()
        row["moments"] = dict(first, other_order=again)
        print(name, "moments", json.dumps(row["moments"], sort_keys=True), flush=True)
        assert L.pt__film_debug(MOMENTS, 0) == 0

        def exposed_with_guides():
            film.set_camera(cam)
            film.expose(1, FRAMES, 0)

        row["with_guides"] = timed(hip, pt, exposed_with_guides, reps)
        row["denoise"] = timed(hip, pt, lambda: film.denoise(), reps)

        def denoised_with_gather():
            film.set_camera(cam)
            film.denoise()

        row["denoise_guides_only"] = timed(hip, pt, denoised_with_gather, reps)
        ts = []
        for rep in range(reps + 2):
            t0 = time.perf_counter()
            film.noise(0.05)
            if rep >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        row["noise_wall"] = dict(ms=round(statistics.median(ts), 3), ms_range=[round(min(ts), 3), round(max(ts), 3)])
        print(name, json.dumps({k: row[k] for k in ("with_guides", "denoise", "denoise_guides_only", "noise_wall")},
                               sort_keys=True), flush=True)
        hip.L.hipFree(d_rgba)
        film.close()
        pt.close()
        doc["scenes"][name] = row
    return doc


def main():
    if len(sys.argv) < 3 or sys.argv[1] not in ("resources", "gpu"):
        sys.exit(__doc__)
    mode, path, args = sys.argv[1], sys.argv[2], sys.argv[3:]
    opt = lambda name, default: args[args.index(name) + 1] if name in args else default
    doc = load(path)
    if mode == "resources":
        doc["resources"] = resources()
    else:
        doc["measured"] = gpu(int(opt("--reps", 5)), opt("--scenes", "cornell,bunny").split(","))
    save(path, doc)
    if mode == "resources":
        print(json.dumps(doc["resources"], indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
