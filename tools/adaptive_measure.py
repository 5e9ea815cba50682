#!/usr/bin/env python3
"""What adaptive sampling costs and buys (profiles/adaptive_sampling.json), on
1080p Cornell, 8 bounces:
  * the plain path: bench.py's headline on a library from before the feature (--parent-lib) and on
    this build, alternating, each run a process of its own (the queue's tile count became a
    kernel argument of k_render_sm);
  * pt_render_adaptive against pt_render_until and against the plain pt_render of the adaptive
    run's frames_done frames (the uniform render that gives every tile the same guarantee), in
    batches of 64 for targets 0.1 and 0.05: frames, pixel-frames, wall time (host clock around
    the synchronous calls, warmed, repetitions interleaved), final mean relative error;
  * the fused accumulate-and-retire pass: every k_accum_retire dispatch of one adaptive run under
    rocprofv3 --kernel-trace --stats, with the length of its list.
Every step is a process or call with its own time limit; the first that fails ends the run.

  python tools/adaptive_measure.py out.json [--parent-lib <older libptrace.so>] [--runs 4]
"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "opengl-path-tracing_amd")]

W, HH, B, BATCH, MAX_FRAMES = 1920, 1080, 8, 64, 4096
TARGETS = (0.1, 0.05)


def bench_once(lib):
    env = dict(os.environ)
    if lib:
        env.update(PT_LIB=lib, PT_LIB_PARTIAL="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "3"],
                       env=env, capture_output=True, text=True, timeout=240)
    if r.returncode != 0:
        sys.exit("bench.py failed (%d) with %s:\n%s" % (r.returncode, lib or "this build", r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])["value"]


def plain_path(parent_lib, runs):
    res = {"parent": [], "head": []}
    for i in range(runs):
        for who in (("parent", "head") if i % 2 == 0 else ("head", "parent")):
            res[who].append(bench_once(parent_lib if who == "parent" else None))
    span = lambda v: [min(v), max(v)]
    p, h = span(res["parent"]), span(res["head"])
    width = p[1] - p[0]
    return dict(command="bench.py --gpus 1 --steps 10 --warmup 3", unit="Mrays/s", runs=res, parent_span=p, head_span=h,
                parent_span_width_frac=round(width / p[0], 5),
                head_below_parent_span_by_more_than_its_width=bool(h[0] < p[0] - width))


def pass_child():
    """The workload of the kernel trace: one adaptive run whose lists shrink from the full grid."""
    import pt_host as H
    import pt_scenes
    sb = H.setupBuffers(*pt_scenes.write_scene("cornell", os.path.join(REPO, "scenes")))
    pt = H.PathTracer(W, HH, max_bounce=B)
    pt.upload(sb)
    pt.render(1, 64, 0)
    print(json.dumps(pt.render_adaptive(0.1, batch=BATCH, max_frames=1024)))
    pt.close()


def pass_trace():
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
                            sys.executable, os.path.abspath(__file__), "--pass-child"], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.exit("rocprofv3 failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
        trace = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        rows = [k for k in csv.DictReader(open(trace[0]))] if trace else []
    rows.sort(key=lambda k: int(k["Start_Timestamp"]))
    out, render_us = [], None
    for k in rows:
        us = (int(k["End_Timestamp"]) - int(k["Start_Timestamp"])) / 1e3
        if "k_render_sm" in k["Kernel_Name"]:
            render_us = us
        if "k_accum_retire" in k["Kernel_Name"]:
            grid = int(k.get("Grid_Size") or k.get("Grid_Size_X") or 0)
            out.append(dict(grid_threads=grid, pass_us=round(us, 2), render_kernel_us=round(render_us or 0.0, 2)))
    return dict(workload="pt_render_adaptive(0.1, batch 64, max 1024) after a 64-frame render, 32,400 tiles",
                dispatches=out)


def feature():
    import pt_host as H
    import pt_scenes
    sb = H.setupBuffers(*pt_scenes.write_scene("cornell", os.path.join(REPO, "scenes")))
    pt = H.PathTracer(W, HH, max_bounce=B)
    pt.upload(sb)
    pt.set_moments(True)
    pt.render(1, 256, 0)                  # warm: the tile order, the scratch of a 64-frame batch
    pt.render_adaptive(0.2, batch=BATCH, max_frames=256)
    pt.render_until(0.2, batch=BATCH, max_frames=256)
    out = {}
    for target in TARGETS:
        runs = {"adaptive": [], "until": [], "plain": []}
        facts = {}
        for rep in range(3):
            t = time.perf_counter()
            done, s = pt.render_adaptive(target, batch=BATCH, max_frames=MAX_FRAMES)
            runs["adaptive"].append(time.perf_counter() - t)
            facts["adaptive"] = dict(frames_done=done, pixel_frames=s["pixel_frames"], mean_rel=s["mean"], tiles=s["tiles"],
                                     tiles_active=s["tiles_active"], above_frac=s["above_frac"])
            t = time.perf_counter()
            udone, us = pt.render_until(target, batch=BATCH, max_frames=MAX_FRAMES)
            runs["until"].append(time.perf_counter() - t)
            facts["until"] = dict(frames_done=udone, pixel_frames=udone * us["pixels"], mean_rel=us["mean"],
                                  above_frac=us["above_frac"])
            t = time.perf_counter()
            pt.render(1, done, 0)
            runs["plain"].append(time.perf_counter() - t)
            ps = pt.noise(target)
            facts["plain"] = dict(frames_done=done, pixel_frames=done * ps["pixels"], mean_rel=ps["mean"],
                                  above_frac=ps["above_frac"])
        for k, v in runs.items():
            best = min(v)
            facts[k].update(seconds=[round(x, 4) for x in v], ns_per_pixel_frame=round(best * 1e9 / max(facts[k]["pixel_frames"], 1), 4))
        facts["adaptive_ns_per_pixel_frame_over_plain"] = round(
            facts["adaptive"]["ns_per_pixel_frame"] / facts["plain"]["ns_per_pixel_frame"], 4)
        out["target_%g" % target] = facts
    pt.close()
    return out


def main():
    if "--pass-child" in sys.argv[1:]:
        return pass_child()
    out_path = sys.argv[1]
    arg = lambda name, d: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else d
    parent, runs = arg("--parent-lib", None), int(arg("--runs", "4"))
    out = {"width": W, "height": HH, "bounces": B, "batch": BATCH, "max_frames": MAX_FRAMES}

    def save():
        with open(out_path, "w") as f:
            json.dump(out, f, indent=1)
    if parent:
        out["plain_path"] = plain_path(os.path.abspath(parent), runs)
        save()
    out["pass"] = pass_trace()
    save()
    out["feature"] = feature()
    save()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
