"""GPU box: what a frame with n = 1 .. 4 lights costs (Scene.add_light), frame-only mode, the uint8 frame left in
device memory.  Per scene and n: wall-clock ms per frame with one frame at a time (enqueue, wait) and with three in
flight on three streams, and the device time of the three kernels (HIP events of frames enqueued with all marks).
The yardstick of an n-light frame is n single-light frames: the n = 1 row times n.  On a build without add_light
(the commit before the feature) only the n = 1 rows are printed, so the same tool times the yardstick on both builds.

    python tools/time_lights.py [--frames N] [--reps R] [scene ...]     (default: c4_torus200k_1080p c3_diablo_floor_1080p)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c4_torus200k_1080p", "c3_diablo_floor_1080p"])
ap.add_argument("--frames", type=int, default=400)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--n", type=int, nargs="*", default=[1, 2, 3, 4], help="numbers of lights to time")
ap.add_argument("--mode", choices=("both", "one", "three"), default="both",
                help="time only one frame at a time / only three in flight (for a kernel trace of one regime)")
args = ap.parse_args()

import torch
import scenes


def extra_lights(api):
    """The lights of tests/multilight_ref.py: a point, a directional and a spot light."""
    return [api.Light((-3, 2.5, 1.5), color=(1.0, 0.8, 0.6), ambient_strength=0.05, specular_strength=0.3),
            api.Light((0.5, 4, -3), light_type=api.Lightning.DIRECTIONAL_LIGHTNING, center=(0, 0, 0),
                      color=(0.6, 0.7, 1.0), ambient_strength=0.0, specular_strength=0.2),
            api.Light((-1, 3, 3), light_type=api.Lightning.SPOT_LIGHTNING, center=(0, 0.3, 0),
                      ambient_strength=0.02, specular_strength=0.4)]


def measure(api, name, n):
    scene = scenes.build(api, name)
    for light in extra_lights(api)[:n - 1]:
        scene.add_light(light)
    backend = scene._backend()
    h, w = scene.resolution
    streams = [torch.cuda.Stream() for _ in range(3)]
    outs = [torch.zeros(h * w * 3 + 4096, dtype=torch.uint8, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    desc = backend.render_device(scene, outs[0].data_ptr(), streams[0].cuda_stream, no_timing=True)
    for _ in range(4):                                # the work lists grow to what the frame needs
        torch.cuda.synchronize()
        if not backend.overflowed():
            break
        backend.enqueue(desc, outs[0].data_ptr(), streams[0].cuda_stream)
    quiet, marked = backend.with_timing(desc, "none"), backend.with_timing(desc, "all")

    def one_at_a_time(frames):
        for _ in range(frames):
            backend.enqueue(quiet, outs[0].data_ptr(), streams[0].cuda_stream)
            streams[0].synchronize()

    def three_in_flight(frames):
        for k in range(frames):
            s = k % 3
            streams[s].synchronize()
            backend.enqueue(quiet, outs[s].data_ptr(), streams[s].cuda_stream)
        torch.cuda.synchronize()

    row = {}
    for label, fn in (("one", one_at_a_time), ("three", three_in_flight)):
        if args.mode not in ("both", label):
            row[label] = [float("nan")] * args.reps
            continue
        fn(32)
        best = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.frames)
            best.append((time.perf_counter() - t0) * 1e3 / args.frames)
        row[label] = best
    for _ in range(24 if args.mode != "three" else 0):   # kernel times: one marked frame at a time
        backend.enqueue(marked, outs[0].data_ptr(), streams[0].cuda_stream)
        streams[0].synchronize()
    times = dict.fromkeys(backend.KERNEL_TIME_NAMES, float("nan"))
    if args.mode != "three":
        times, _ = backend.stream_kernel_times(streams[0].cuda_stream, 16)
    stats = backend.stats()
    scene.close()
    return row, times, stats


def main():
    api = scenes.product_api()
    multi = hasattr(api.Scene, "add_light")
    print(f"# frames {args.frames} x reps {args.reps}; ms per frame (min / median of reps); kernels in us (one frame at a time)")
    for name in args.scenes:
        base = None
        for n in args.n if multi else (1,):
            row, t, st = measure(api, name, n)
            one, three = sorted(row["one"]), sorted(row["three"])
            if base is None:                          # (the first row: n = 1 unless --n says otherwise)
                base = (one[0] / n, three[0] / n)
            print(f"{name:22s} n={n}  one at a time {one[0]:7.4f} / {one[len(one) // 2]:7.4f}   three in flight {three[0]:7.4f} / "
                  f"{three[len(three) // 2]:7.4f}   k_setup {t['setup'] * 1e3:6.1f} k_bin_work {t['bin_work'] * 1e3:6.1f} "
                  f"k_tile {t['tile'] * 1e3:6.1f} frame {t['frame'] * 1e3:6.1f}   n_quads {st['n_quads']}   "
                  f"vs {n} x single: {one[0] / (n * base[0]):5.3f} / {three[0] / (n * base[1]):5.3f}", flush=True)


if __name__ == "__main__":
    main()
