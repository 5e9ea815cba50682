#!/usr/bin/env python3
"""What the denoised view costs (profiles/denoise.json), on 1080p Cornell, 8 bounces:
  * a 5-iteration pt_denoise, guided (moments of 8 frames) and unguided, per pass -- the prep and
    each iteration -- with the taps read from the LDS tile (the default up to step 16) and by
    direct loads, from HIP events on the context stream (pt__denoise_debug / pt__denoise_times,
    internal entry points of the library), the median of --reps warmed repetitions;
  * the guide render (three display modes, guide_frames 4);
  * a plain device copy that moves the bytes an iteration must move (64 B per pixel: 16 colour + 32
    guides read, 16 written), timed in the same process with the same kind of events;
  * with --parent-lib: bench.py's headline on that library and on this build, alternating.
The `resources` mode needs no GPU: it compiles csrc/pt_denoise_kernels.hip for gfx950 with the
compiler's resource remarks and records each kernel's registers, LDS and occupancy.

  python tools/denoise_measure.py resources out.json
  python tools/denoise_measure.py gpu out.json [--reps 7] [--parent-lib <older libptrace.so>] [--runs 3]
Both modes update out.json in place.
"""
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "opengl-path-tracing_amd")
sys.path[:0] = [PKG]

W, HH, B = 1920, 1080, 8
LDS_CU, TX, TY = 160 * 1024, 64, 4


def load(path):
    return json.load(open(path)) if os.path.exists(path) else {}


def save(path, doc):
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def resources():
    """Registers, scratch, static LDS and register-limited occupancy per kernel, from the compiler's remarks;
    and the dynamic LDS of the tiled iteration per step with the workgroups per CU it allows."""
    hipcc = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "bin", "hipcc")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize", "--cuda-device-only", "-c",
           "-Rpass-analysis=kernel-resource-usage", os.path.join(PKG, "csrc", "pt_denoise_kernels.hip"), "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(re.sub(r"^_ZN3ptd\d+_GLOBAL__N_1\d+|E.*$", "", m.group(1)) or m.group(1), {})
            continue
        m = re.search(r"remark: \s*(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    tile = {}
    for step in (1, 2, 4, 8, 16):
        lds = (TX + 4 * step) * (TY + 4) * 48
        blocks = min(8, LDS_CU // lds)                       # 256-thread workgroups: one wave per SIMD each
        tile[str(step)] = dict(lds_bytes=lds, workgroups_per_cu=blocks, waves_per_simd=blocks,
                               loads_per_pixel=round((TX + 4 * step) * (TY + 4) / (TX * TY), 3))
    return dict(kernels=kernels, lds_tile_by_step=tile)


def timed_denoise(H, pt, variant, reps, **params):
    """Median ms per pass of `reps` warmed denoises: [guides, prep, iteration 0, ...]."""
    L = H.lib()
    L.pt__denoise_debug.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pt__denoise_times.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    assert L.pt__denoise_debug(pt.h, variant, 1) == 0
    rows = []
    for rep in range(reps + 2):
        pt.denoise(**params)
        out = (C.c_float * 16)()
        n = L.pt__denoise_times(pt.h, out, 16)
        assert n >= 3, n
        if rep >= 2:
            rows.append(list(out[:n]))
    assert L.pt__denoise_debug(pt.h, 0, 0) == 0
    return [round(statistics.median(r[i] for r in rows), 5) for i in range(len(rows[0]))]


def copy_ms(reps):
    """A plain device copy whose traffic is an iteration's: 32 B per pixel read and 32 B written."""
    hip = C.CDLL(os.path.join(os.environ.get("ROCM", "/opt/rocm"), "lib", "libamdhip64.so"))   # the library's own runtime
    vp = C.c_void_p

    def ok(rc):
        assert rc == 0, "HIP error %d" % rc
    n = W * HH * 32
    src, dst, a, b = vp(), vp(), vp(), vp()
    ok(hip.hipMalloc(C.byref(src), C.c_size_t(n)))
    ok(hip.hipMalloc(C.byref(dst), C.c_size_t(n)))
    ok(hip.hipMemset(src, 0, C.c_size_t(n)))
    ok(hip.hipEventCreate(C.byref(a)))
    ok(hip.hipEventCreate(C.byref(b)))
    ts = []
    for rep in range(reps + 2):
        ok(hip.hipEventRecord(a, vp(0)))
        ok(hip.hipMemcpyAsync(dst, src, C.c_size_t(n), 3, vp(0)))     # hipMemcpyDeviceToDevice
        ok(hip.hipEventRecord(b, vp(0)))
        ok(hip.hipEventSynchronize(b))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), a, b))
        if rep >= 2:
            ts.append(ms.value)
    for e in (a, b):
        ok(hip.hipEventDestroy(e))
    for p in (src, dst):
        ok(hip.hipFree(p))
    return round(statistics.median(ts), 5)


def bench_once(lib):
    env = dict(os.environ)
    if lib:
        env.update(PT_LIB=lib, PT_LIB_PARTIAL="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"],
                       env=env, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:
        sys.exit("bench.py failed (%d) with %s:\n%s" % (r.returncode, lib or "this build", r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])["value"]


def gpu(reps, parent_lib, runs):
    import pt_host as H
    import pt_scenes
    sb = H.setupBuffers(*pt_scenes.write_scene("cornell", os.path.join(REPO, "scenes")))
    doc = dict(width=W, height=HH, bounces=B, frames=8, reps=reps, unit="ms")
    copy = None
    for name, moments in (("guided", True), ("unguided", False)):
        pt = H.PathTracer(W, HH, max_bounce=B)
        pt.upload(sb)
        if copy is None:    # (after the first context: the device is set)
            copy = doc["copy_64B_per_pixel_ms"] = copy_ms(reps)
        if moments:
            pt.set_moments(True)
        pt.render(1, 8, 0)
        for vname, variant in (("lds", 0), ("direct", 1)):
            t = timed_denoise(H, pt, variant, reps)
            its = t[2:]
            doc["%s_%s" % (name, vname)] = dict(prep_ms=t[1], iteration_ms=its, total_ms=round(t[1] + sum(its), 5),
                                                ratio_to_copy=[round(x / copy, 2) for x in its])
        if moments:     # the guide render: every call renders when guide_frames alternates
            g = []
            for rep in range(reps + 2):
                L = H.lib()
                L.pt__denoise_debug(pt.h, 0, 1)
                pt.denoise(guide_frames=4 if rep % 2 else 3)
                out = (C.c_float * 16)()
                L.pt__denoise_times(pt.h, out, 16)
                if rep >= 2 and rep % 2:
                    g.append(out[0])
            L.pt__denoise_debug(pt.h, 0, 0)
            doc["guide_render_ms"] = dict(guide_frames=4, ms=round(statistics.median(g), 5))
        pt.close()
    if parent_lib:
        res = {"parent": [], "head": []}
        for i in range(runs):
            for who in (("parent", "head") if i % 2 == 0 else ("head", "parent")):
                res[who].append(bench_once(parent_lib if who == "parent" else None))
        doc["bench_headline"] = dict(command="bench.py --gpus 1 --steps 10 --warmup 3", unit="Mrays/s", runs=res,
                                     parent_span=[min(res["parent"]), max(res["parent"])],
                                     head_span=[min(res["head"]), max(res["head"])])
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
        doc["measured"] = gpu(int(opt("--reps", 7)), opt("--parent-lib", None), int(opt("--runs", 3)))
    save(path, doc)
    print(json.dumps(doc[("resources" if mode == "resources" else "measured")], indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
