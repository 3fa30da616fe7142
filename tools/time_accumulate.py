"""GPU box: what a weighted sum of sub-frames costs (Scene.accumulate).  Per scene at its full size, --sub sub-frames with a
light that moves on every one; ms per accumulated frame, minimum / median of --reps runs:

  (a)  by hand    --sub x (backend.render(keep_float=True) + read_frame_f32()), the sum in NumPy (float32, the weights of
                  the definition) and the finalise in NumPy.  The only way on a build without Scene.accumulate -- run this
                  tool with --tree on a built checkout of the commit before the feature for the parent's figure.
  (a') uint8      --sub x Scene.render() and the mean of the uint8 frames: wrong (after the gamma, after the
                  quantisation) but common; given for scale only.
  (b)  accumulate Scene.accumulate(): --sub x add(1.0), one result().
  (c)  kernels    device us of k_accum_add and k_accum_resolve inside that sequence (HIP events; the add: mean over the
                  sub-frames of one accumulation but the first, which reads no sum), with the bytes they move -- 3 x and 1 x
                  the float frame, plus the output -- as GB/s.  tools/micro/accum_bench.hip times the same kernels alone.

    python tools/time_accumulate.py --out profiles/accumulate_time.txt [--tree DIR] [--label WORD] [scene ...]
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c4_torus200k_1080p", "c3_diablo_floor_1080p"])
ap.add_argument("--sub", type=int, default=16, help="sub-frames per accumulated frame")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--tree", default=None, help="a built checkout to measure instead of this one (the commit before the feature)")
ap.add_argument("--label", default="", help="a word for the header line (which build this is)")
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()

ROOT = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import scenes

HBM_GBS = 8000.0        # the HBM figure DESIGN.md uses for the MI355X


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def light_at(scene, k):
    scene.light.position = np.array((2.0 + 0.02 * (k % 5), 3.0 + 0.02 * (k % 3), 4.0 - 0.02 * (k % 7)))


def runs(fn):
    """ms per call of fn(rep), --reps times after one warm-up call: (minimum, median)."""
    fn(0)
    per = []
    for rep in range(1, args.reps + 1):
        t0 = time.perf_counter()
        fn(rep)
        per.append((time.perf_counter() - t0) * 1e3)
    per.sort()
    return per[0], per[len(per) // 2]


def measure(api, name):
    has = hasattr(api.Scene, "accumulate")
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    backend = scene._backend()
    n = args.sub
    tag = f"{name:22s}"
    for k in range(4):                                   # the work lists grow to what the scene needs
        light_at(scene, k)
        scene.render()
    w = np.float32(1.0)

    def by_hand(rep):
        acc = None
        for k in range(n):
            light_at(scene, rep * n + k)
            backend.render(scene, keep_float=True, counters=False, keep_buffers=False, timing=False)
            part = w * backend.read_frame_f32()
            acc = part if acc is None else acc + part
        r = np.minimum(acc * np.float32(1.0 / n), np.float32(1.0))
        return (r[::-1] ** 0.8 * 255).astype(np.uint8)

    def by_bytes(rep):
        total = None
        for k in range(n):
            light_at(scene, rep * n + k)
            frame = scene.render().astype(np.uint16)
            total = frame if total is None else total + frame
        return (total // n).astype(np.uint8)

    a = runs(by_hand)
    emit(f"{tag} (a)  {n} x (keep_float frame + read_frame_f32), NumPy sum and finalise   {a[0]:9.3f} / {a[1]:9.3f} ms")
    a1 = runs(by_bytes)
    emit(f"{tag} (a') {n} x Scene.render(), mean of the uint8 frames                      {a1[0]:9.3f} / {a1[1]:9.3f} ms")
    if not has:
        scene.close()
        return

    add_us = []

    def by_accumulate(rep, timed=False):
        with scene.accumulate() as acc:
            for k in range(n):
                light_at(scene, rep * n + k)
                acc.add(1.0)
                if timed and k > 0:
                    add_us.append(backend.accum_times()["accum_add"] * 1e3)
            return acc.result()

    b = runs(by_accumulate)
    emit(f"{tag} (b)  Scene.accumulate(): {n} x add(1.0), one result()                   {b[0]:9.3f} / {b[1]:9.3f} ms     "
         f"(a) / (b) = {a[0] / b[0]:.1f}   per sub-frame {b[0] / n:.3f} ms")
    apart = np.abs(by_accumulate(1).astype(np.int16) - by_hand(1).astype(np.int16))
    by_accumulate(2, timed=True)
    resolve_us = backend.accum_times()["accum_resolve"] * 1e3
    _, _, hs, ws = backend.accum_debug()
    frame_bytes, out_bytes = hs * ws * 3 * 4, (hs // scene.supersample) * (ws // scene.supersample) * 3
    add_us.sort()
    med = add_us[len(add_us) // 2]
    emit(f"{tag} (c)  k_accum_add in the sequence (a frame's kernels between two adds): {add_us[0]:.1f} / {med:.1f} us (minimum / median of "
         f"{len(add_us)}), {3 * frame_bytes / 1e6:.1f} MB -> {3 * frame_bytes / med / 1e3:.0f} GB/s at the median (HBM: {HBM_GBS:.0f})")
    emit(f"{tag} (c)  k_accum_resolve: {resolve_us:.1f} us, {(frame_bytes + out_bytes) / 1e6:.1f} MB -> "
         f"{(frame_bytes + out_bytes) / resolve_us / 1e3:.0f} GB/s")
    emit(f"{tag}      (b)'s bytes against (a)'s (NumPy's power against the device's step table): at most {int(apart.max())} apart, "
         f"{int((apart > 0).sum())} of {apart.size} differ")
    scene.close()


def main():
    api = scenes.product_api()
    emit(f"# {args.label + ': ' if args.label else ''}{args.sub} sub-frames x reps {args.reps}; ms per accumulated frame, minimum / median of the "
         f"runs; Scene.accumulate {'present' if hasattr(api.Scene, 'accumulate') else 'absent (the build before the feature)'}")
    for name in args.scenes:
        measure(api, name)


if __name__ == "__main__":
    main()
