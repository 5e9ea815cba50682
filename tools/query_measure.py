#!/usr/bin/env python3
"""What a ray query costs (profiles/query.json): pt_intersect_device on 1080p primary rays (coherent)
and on the same number of shuffled bounce-like rays (origin a primary hit's p, direction in the hemisphere of its n),
on Cornell, the reference's ship and the 69k- and 249k-triangle stand-ins, closest-hit and any-hit, with the top of
the tree staged in LDS and unstaged (pt__query_debug, an internal entry point of the library) side by side -- from HIP
events on the context stream, the median of --reps warmed repetitions.
The `resources` mode needs no GPU: it compiles csrc/pt_query_kernels.hip for gfx950 with the compiler's resource
remarks and records each kernel's registers, scratch, LDS and occupancy.

  python tools/query_measure.py resources out.json
  python tools/query_measure.py gpu out.json [--reps 5] [--scenes cornell,ship,bunny,sponza]
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
sys.path[:0] = [PKG]

W, HH = 1920, 1080


def load(path):
    return json.load(open(path)) if os.path.exists(path) else {}


def save(path, doc):
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def resources():
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(PKG, "csrc", "pt_query_kernels.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            t = re.search(r"k_castILb([01])ELb([01])E", m.group(1))
            name = "k_cast<ANY=%s, STAGED=%s>" % (t.group(1), t.group(2)) if t else m.group(1)
            cur = kernels.setdefault(name, {})
            continue
        m = re.search(r"remark: \s*(VGPRs|AGPRs|SGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    return dict(kernels=kernels)


class Hip:
    """The HIP runtime the library links, through the library's handle."""

    def __init__(self, lib):
        vp = C.c_void_p
        self.L = lib
        for fn, args in (("hipMalloc", [C.POINTER(vp), C.c_size_t]), ("hipFree", [vp]),
                         ("hipMemcpy", [vp, vp, C.c_size_t, C.c_int]), ("hipEventCreate", [C.POINTER(vp)]),
                         ("hipEventRecord", [vp, vp]), ("hipEventSynchronize", [vp]), ("hipEventDestroy", [vp]),
                         ("hipEventElapsedTime", [C.POINTER(C.c_float), vp, vp])):
            getattr(lib, fn).restype, getattr(lib, fn).argtypes = C.c_int, args

    def ok(self, rc):
        assert rc == 0, "HIP error %d" % rc

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.ok(self.L.hipMalloc(C.byref(p), nbytes))
        return p


def timed(hip, pt, d_rays, n, d_hits, any_hit, reps):
    a, b = C.c_void_p(), C.c_void_p()
    hip.ok(hip.L.hipEventCreate(C.byref(a)))
    hip.ok(hip.L.hipEventCreate(C.byref(b)))
    stream = C.c_void_p(pt.stream())
    ts = []
    for rep in range(reps + 2):
        hip.ok(hip.L.hipEventRecord(a, stream))
        pt.intersect_device(d_rays.value, n, d_hits.value, any_hit)
        hip.ok(hip.L.hipEventRecord(b, stream))
        hip.ok(hip.L.hipEventSynchronize(b))
        ms = C.c_float()
        hip.ok(hip.L.hipEventElapsedTime(C.byref(ms), a, b))
        if rep >= 2:
            ts.append(ms.value)
    hip.L.hipEventDestroy(a)
    hip.L.hipEventDestroy(b)
    return statistics.median(ts)


def scene(H, name):
    import pt_scenes
    if name == "ship":
        z = np.load(os.path.join(REPO, "tests", "golden", "ship_scene.npz"))
        return H.scene_from_arrays(z["tris"], z["mats"])
    return H.setupBuffers(*pt_scenes.write_scene(name, os.path.join(REPO, "scenes")))


def gpu(reps, names):
    import pt_host as H
    L = H.lib()
    L.pt__query_debug.argtypes = [C.c_int]
    hip = Hip(L)
    ys, xs = np.meshgrid(np.arange(HH), np.arange(W), indexing="ij")
    xy = np.stack([xs.ravel(), ys.ravel()], 1)
    doc = dict(width=W, height=HH, rays=len(xy), reps=reps, unit="Mrays/s", scenes={})
    rng = np.random.default_rng(5)
    for name in names:
        sb = scene(H, name)
        pt = H.PathTracer(W, HH, max_bounce=8)
        pt.upload(sb)
        primary = H.pixel_rays(W, HH, sb["cam"], xy)
        h = pt.intersect(primary)
        hit = np.nonzero(h["kind"] > 0)[0]
        src = hit[rng.integers(0, hit.size, len(xy))]              # shuffled: neighbouring lanes start far apart
        u = rng.standard_normal((len(src), 3)).astype(np.float32)
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        bounce = H.make_rays(h["p"][src, 0:3], h["n"][src, 0:3] + np.float32(0.98) * u)
        row = dict(triangles=len(sb["tris"]), nodes=len(sb["nodes"]), primary_hit_fraction=round(hit.size / len(xy), 4))
        d_hits = hip.alloc(len(xy) * 48)
        for rname, rays in (("primary", primary), ("bounce", bounce)):
            d_rays = hip.alloc(rays.nbytes)
            hip.ok(L.hipMemcpy(d_rays, rays.ctypes.data, rays.nbytes, 1))
            for vname, variant in (("staged", 0), ("unstaged", 1)):
                assert L.pt__query_debug(variant) == 0
                for aname, any_hit in (("closest", False), ("any", True)):
                    ms = timed(hip, pt, d_rays, len(rays), d_hits, any_hit, reps)
                    row["%s_%s_%s" % (rname, aname, vname)] = dict(ms=round(ms, 4), mrays_per_s=round(len(rays) / ms / 1e3, 1))
            hip.L.hipFree(d_rays)
        L.pt__query_debug(0)
        hip.L.hipFree(d_hits)
        pt.close()
        doc["scenes"][name] = row
        print(name, json.dumps(row, sort_keys=True), flush=True)
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
        doc["measured"] = gpu(int(opt("--reps", 5)), opt("--scenes", "cornell,ship,bunny,sponza").split(","))
    save(path, doc)
    if mode == "resources":
        print(json.dumps(doc["resources"], indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
