#!/usr/bin/env python3
"""What a traced ray costs (profiles/trace.json): pt_trace_device on 1080p camera rays (coherent) and on
the same number of shuffled bounce-like rays (origin a camera hit's p, direction in the hemisphere of its n), 1 and 8
frames at max_bounce 8, on Cornell, the reference's ship and the 69k- and 249k-triangle stand-ins -- with refill
between segments against the plain one-ray-per-lane loop, and with the top of the tree staged in LDS against
unstaged (pt__trace_debug, an internal entry point of the library), side by side.  From HIP events on the context
stream: the median, and the range, of --reps repetitions after 2 warm-ups.

The unit is segments per second.  The segment count is the host twin's, which runs the same per-ray code: every
--sample'th ray of the batch goes through pt__trace_host_segments (an internal entry point) and the count is scaled
by the sampling rate.

The `resources` mode needs no GPU: it compiles csrc/pt_trace_kernels.hip for gfx950 with the compiler's resource
remarks and records each kernel's registers, scratch, LDS and occupancy.

  python tools/trace_measure.py resources out.json
  python tools/trace_measure.py gpu out.json [--reps 5] [--sample 97] [--scenes cornell,ship,bunny,sponza]
Both modes update out.json in place.
"""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "opengl-path-tracing_amd")
sys.path[:0] = [PKG, os.path.join(REPO, "tools")]

from query_measure import Hip, load, save, scene  # noqa: E402  (the same runtime handle, scenes and JSON form)

W, HH = 1920, 1080
MAX_BOUNCE = 8
STAGING, REFILL = 0, 1                    # ptt::Debug (csrc/pt_trace_launch.h)
COMBOS = (("refill_staged", 1, 1), ("refill_unstaged", 1, 2), ("plain_staged", 2, 1), ("plain_unstaged", 2, 2))


def resources():
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(PKG, "csrc", "pt_trace_kernels.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            t = re.search(r"k_traceILb([01])ELb([01])E", m.group(1))
            name = "k_trace<STAGED=%s, REFILL=%s>" % (t.group(1), t.group(2)) if t else m.group(1)
            cur = kernels.setdefault(name, {})
            continue
        m = re.search(r"remark: \s*(VGPRs|AGPRs|SGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return dict(kernels=kernels)


def timed(hip, pt, d_rays, d_seeds, n, d_rgba, n_frames, reps):
    a, b = C.c_void_p(), C.c_void_p()
    hip.ok(hip.L.hipEventCreate(C.byref(a)))
    hip.ok(hip.L.hipEventCreate(C.byref(b)))
    stream = C.c_void_p(pt.stream())
    ts = []
    for rep in range(reps + 2):
        hip.ok(hip.L.hipEventRecord(a, stream))
        pt.trace_device(d_rays.value, d_seeds.value, n, d_rgba.value, 1, n_frames, 0)
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        if rep >= 2:
            ts.append(ms.value)
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    return statistics.median(ts), min(ts), max(ts)


def host_segments(H, sb, rays, seeds, n_frames, sample):
    """Segments of the whole batch, from the host twin's count on every sample'th ray."""
    L = H.lib()
    r, s = np.ascontiguousarray(rays[::sample]), np.ascontiguousarray(seeds[::sample])
    t, nd, m, sp = (np.ascontiguousarray(sb[k], np.float32).reshape(-1) for k in ("tris", "nodes", "mats", "spheres"))
    out = np.zeros((len(r), 4), np.float32)
    count = C.c_longlong(0)
    vp = C.c_void_p
    L.pt__trace_host_segments.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                          vp, vp, C.c_longlong, C.c_int, C.c_int, C.c_int, vp, C.POINTER(C.c_longlong)]
    rc = L.pt__trace_host_segments(t.ctypes.data, len(sb["tris"]), nd.ctypes.data, len(sb["nodes"]), m.ctypes.data,
                                   len(sb["mats"]), sp.ctypes.data, len(sb["spheres"]), 0, MAX_BOUNCE, 1, r.ctypes.data,
                                   s.ctypes.data, len(r), 1, n_frames, 0, out.ctypes.data, C.byref(count))
    assert rc == 0, rc
    return count.value * len(rays) / len(r)


def gpu(reps, sample, names):
    import pt_host as H
    L = H.lib()
    hip = Hip(L)
    ys, xs = np.meshgrid(np.arange(HH), np.arange(W), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], 1)
    n = len(xy)
    doc = dict(width=W, height=HH, rays=n, reps=reps, max_bounce=MAX_BOUNCE, segment_sample=sample,
               unit="Msegments/s (median; ms_range: the repetitions' least and greatest time)", scenes={})
    rng = np.random.default_rng(5)
    for name in names:
        sb = scene(H, name)
        pt = H.PathTracer(W, HH, max_bounce=MAX_BOUNCE)
        pt.upload(sb)
        camera = H.pixel_rays(W, HH, sb["cam"], xy)
        h = pt.intersect(camera)
        hit = np.nonzero(h["kind"] > 0)[0]
        src = hit[rng.integers(0, hit.size, n)]                    # shuffled: neighbouring lanes start far apart
        u = rng.standard_normal((n, 3)).astype(np.float32)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        bounce = H.make_rays(h["p"][src, 0:3], h["n"][src, 0:3] + np.float32(0.98) * u)
        seeds = H.pixel_seeds(xy)
        row = dict(triangles=len(sb["tris"]), nodes=len(sb["nodes"]), camera_hit_fraction=round(hit.size / n, 4))
        d_rgba, d_seeds = hip.alloc(n * 16), hip.alloc(n * 4)
        hip.ok(L.hipMemcpy(d_seeds, seeds.ctypes.data, seeds.nbytes, 1))
        for rname, rays in (("camera", camera), ("bounce", bounce)):
            d_rays = hip.alloc(rays.nbytes)
            hip.ok(L.hipMemcpy(d_rays, rays.ctypes.data, rays.nbytes, 1))
            for n_frames in (1, 8):
                segs = host_segments(H, sb, rays, seeds, n_frames, sample)
                case = dict(segments=int(segs), segments_per_path=round(segs / n / n_frames, 3))
                for cname, refill, staging in COMBOS:
                    assert L.pt__trace_debug(REFILL, refill) == 0 and L.pt__trace_debug(STAGING, staging) == 0
                    ms, lo, hi = timed(hip, pt, d_rays, d_seeds, n, d_rgba, n_frames, reps)
                    case[cname] = dict(ms=round(ms, 3), ms_range=[round(lo, 3), round(hi, 3)],
                                       msegments_per_s=round(segs / ms / 1e3, 1))
                row["%s_%df" % (rname, n_frames)] = case
                print(name, rname, n_frames, json.dumps(case, sort_keys=True), flush=True)
            hip.L.hipFree(d_rays)
        L.pt__trace_debug(REFILL, 0)
        L.pt__trace_debug(STAGING, 0)
        hip.L.hipFree(d_rgba)
        hip.L.hipFree(d_seeds)
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
        doc["measured"] = gpu(int(opt("--reps", 5)), int(opt("--sample", 97)),
                              opt("--scenes", "cornell,ship,bunny,sponza").split(","))
    save(path, doc)
    if mode == "resources":
        print(json.dumps(doc["resources"], indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
