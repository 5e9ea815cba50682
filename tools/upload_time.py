"""Wall time of PathTracer.upload (the Python call around pt_upload_scene) on a benchmark scene.

Six uploads on one context; the first carries the context's first allocations, the figure is the
best of the next five.  One JSON line.  profiles/ab/r10_scene_pack/upload_*.json were recorded with
it on the C4 stand-in (the default).

Usage: python tools/upload_time.py [scene] [label]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "opengl-path-tracing_amd"))

import pt_host  # noqa: E402
import pt_scenes  # noqa: E402

scene = sys.argv[1] if len(sys.argv) > 1 else "sponza"
label = sys.argv[2] if len(sys.argv) > 2 else "head"
sb = pt_host.setupBuffers(*pt_scenes.write_scene(scene, os.path.join(REPO, "scenes")))
pt = pt_host.PathTracer(64, 64, max_bounce=8, device=0)
ms = []
for _ in range(6):
    t0 = time.perf_counter()
    pt.upload(sb)
    ms.append((time.perf_counter() - t0) * 1e3)
pt.render(1, 1, 0)     # the uploaded scene renders
pt.close()
print(json.dumps({"tree": label, "scene": scene, "triangles": len(sb["tris"]), "nodes": len(sb["nodes"]),
                  "first_ms": round(ms[0], 2), "next_five_ms": [round(t, 2) for t in ms[1:]],
                  "best_of_five_ms": round(min(ms[1:]), 2)}))
