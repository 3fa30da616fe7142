"""GPU box: per-frame time of a sequence whose LIGHT moves a little on every frame (three frames in flight, the eight
swing views of bench.py, frame-only mode, no event marks): the regime in which the silhouette cache never has a key twice
and must cost nothing.  Run on two builds of the library on one box; with --still the light stays put (the cache's own
regime, for comparison).   usage: tools/time_light_sweep.py [scene] [--frames N] [--reps R] [--still]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("scene", nargs="?", default="c4_torus200k_1080p")
ap.add_argument("--frames", type=int, default=2048)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--lights", type=int, default=64)
ap.add_argument("--still", action="store_true")
args = ap.parse_args()

import numpy as np
import torch
import bench
import scenes
from py_numpy_renderer_amd._native import fill_frame_desc
from py_numpy_renderer_amd._pack import pack_frame
from py_numpy_renderer_amd.multigpu import BandRenderer

api = scenes.product_api()
scene = scenes.build(api, args.scene)
shadows = args.scene not in scenes.NO_SHADOW
br = BandRenderer(scene, 0, 1, shadows=shadows, light_timing=True, frames_in_flight=3, timing_every=0)
views = bench.swing_cameras(api, scene, bench.N_VIEWS)
home = np.array(scene.light.position, dtype=np.float64)
descs = []
for k in range(args.lights):                       # (coprime with the three lanes and the eight views)
    scene.camera, scene.debug_camera = views[k % len(views)]
    if not args.still:
        scene.light.position = home + (1e-3 * k, 0.0, -5e-4 * k)
    descs.append(fill_frame_desc(pack_frame(scene, shadows), br.band, light_timing=True, counters=False, stripe=br.stripe))
br.set_descriptors(descs)
for _ in range(256):
    br.step()
assert br.verify()
ms = []
for _ in range(args.reps):
    br.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.frames):
        br.step()
    br.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3 / args.frames)
assert br.verify()
print(json.dumps({"scene": args.scene, "light": "still" if args.still else "moves every frame", "frames": args.frames,
                  "ms_per_frame": [round(m, 5) for m in ms], "sil_cache": scene._backend().sil_cache()
                  if hasattr(scene._backend(), "sil_cache") else None}))
scene.close()
