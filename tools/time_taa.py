"""GPU box: what the temporal anti-aliasing costs (Scene.temporal_aa) and what the other ways to the same image cost.

  (k)  kernels    device us of the k_velocity in front of k_taa and of k_taa inside real frames (HIP events round the
                  launches, mr_debug_taa_times): minimum / median / maximum of --launches frames, for a still camera and
                  for a pan (the camera turned about its place by --pan degrees a frame, back and forth between two
                  places, so every frame of the case has the same motion and the sky moves with the scene).
                  MR_TAA_TILE=64x4 | 16x16 in the environment times the other workgroup shapes.
  (f)  feature    Scene.render() of a scene without and of its twin with the pass, the same views alternated frame by
                  frame in one loop; ms per frame, minimum / median of --reps, and the difference: the two kernels, the
                  full resolve, the taps every tile now writes, the matrices and the jitter the host builds.
  (s)  the other ways to an anti-aliased still image: --frames temporal-AA frames, one supersample = 4 frame, and
                  render_mean(--sub, a sub-sample offset per sub-frame); ms, minimum / median / maximum of --mean-reps.

    python tools/time_taa.py --out profiles/taa_time.txt [--label WORD] [--only k] [scene ...]
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c3_diablo_floor_1080p"])
ap.add_argument("--launches", type=int, default=24)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--frames", type=int, default=32)
ap.add_argument("--sub", type=int, default=16)
ap.add_argument("--mean-reps", type=int, default=7)
ap.add_argument("--pan", type=float, default=0.42, help="degrees the camera turns from frame to frame in the pan")
ap.add_argument("--only", default="kfs", help="which of the three parts to run")
ap.add_argument("--label", default="", help="a word for the header line (which build this is)")
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import scenes


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def spread(values):
    values = sorted(values)
    return values[0], values[len(values) // 2], values[-1]


def turned(api, cam, angle):
    """*cam* turned by *angle* radians about its up axis, in its place."""
    eye, center, up = (np.asarray(v, dtype=np.float64).ravel()[:3] for v in (cam.position, cam.center, cam.up))
    forward = center - eye
    right = np.cross(forward, up)
    right *= np.linalg.norm(forward) / np.linalg.norm(right)
    return api.Camera(tuple(eye), tuple(eye + np.cos(angle) * forward + np.sin(angle) * right), fovy=cam.fovy, near=cam.near, far=cam.far,
                      backface_culling=cam.backface_culling)


def measure(api, name):
    from py_numpy_renderer_amd import TemporalAA, _pack
    scene, plain = scenes.build(api, name), scenes.build(api, name)
    for s in (scene, plain):
        s.draw_debug_frustum = False
    scene.temporal_aa = TemporalAA(blend=0.1, jitter=8)
    backend = scene._backend()
    tag = f"{name:22s}"
    shape = os.environ.get("MR_TAA_TILE", "32x8")
    base = scene.camera
    cases = [("a still camera", (base, base)), (f"a pan of {args.pan} degrees a frame", (base, turned(api, base, np.radians(args.pan))))]
    for label, views in cases:
        for k in range(4):                                   # the work lists, both float frames and the history grow to what the views need
            scene.camera = plain.camera = views[k % 2]
            scene.render(), plain.render()
        u = backend.read_velocity()
        what = f"{label} (|U| up to {np.hypot(u[..., 0], u[..., 1]).max():.2f} samples, mean {np.hypot(u[..., 0], u[..., 1]).mean():.2f})"
        if "k" in args.only:
            us = {"velocity": [], "taa": []}
            for k in range(args.launches):
                scene.camera = views[k % 2]
                scene.render()
                for key, ms in backend.taa_times().items():
                    us[key].append(ms * 1e3)
            _, hs, ws = backend.taa_debug()[:3]
            v, t = spread(us["velocity"]), spread(us["taa"])
            emit(f"{tag} (k)  k_velocity {v[0]:.1f} / {v[1]:.1f} / {v[2]:.1f} us, k_taa ({shape}) {t[0]:.1f} / {t[1]:.1f} / {t[2]:.1f} us "
                 f"(minimum / median / maximum of {args.launches} frames), {hs} x {ws} samples, {hs * ws * 56 / 1e6:.1f} MB at 56 bytes a sample: {what}")
        if "f" in args.only:
            per = {False: [], True: []}
            for rep in range(args.reps):
                scene.camera = plain.camera = views[rep % 2]
                for on in ((False, True) if rep % 2 == 0 else (True, False)):
                    target = scene if on else plain
                    t0 = time.perf_counter()
                    target.render()
                    per[on].append((time.perf_counter() - t0) * 1e3)
            off, with_taa = spread(per[False]), spread(per[True])
            emit(f"{tag} (f)  Scene.render() without / with the pass, {label}, alternated: {off[0]:.3f} / {off[1]:.3f} ms and "
                 f"{with_taa[0]:.3f} / {with_taa[1]:.3f} ms (minimum / median of {args.reps}): +{with_taa[0] - off[0]:.3f} ms at the minimum, "
                 f"+{with_taa[1] - off[1]:.3f} ms at the median")
    if "s" in args.only:
        scene.camera = plain.camera = base
        ms = {"taa": [], "ss4": [], "mean": []}
        for _ in range(args.mean_reps + 1):
            scene.reset_motion()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                scene.render()
            ms["taa"].append((time.perf_counter() - t0) * 1e3)
            plain.supersample = 4
            plain.render()                                   # (its buffers grow outside the clock)
            t0 = time.perf_counter()
            plain.render()
            ms["ss4"].append((time.perf_counter() - t0) * 1e3)
            plain.supersample = 1
            offsets = [_pack.taa_jitter(k, args.sub) for k in range(args.sub)]
            t0 = time.perf_counter()
            plain.render_mean(args.sub, lambda k: plain.__dict__.__setitem__("_sample_jitter", offsets[k]))
            ms["mean"].append((time.perf_counter() - t0) * 1e3)
            plain.__dict__.pop("_sample_jitter", None)
        a, b, c = spread(ms["taa"][1:]), spread(ms["ss4"][1:]), spread(ms["mean"][1:])
        emit(f"{tag} (s)  a still image: {args.frames} temporal-AA frames {a[0]:.2f} / {a[1]:.2f} / {a[2]:.2f} ms ({a[1] / args.frames:.3f} ms a frame, "
             f"every one of them shown), one supersample = 4 frame {b[0]:.2f} / {b[1]:.2f} / {b[2]:.2f} ms, render_mean({args.sub}, a sub-sample "
             f"offset per sub-frame) {c[0]:.2f} / {c[1]:.2f} / {c[2]:.2f} ms (minimum / median / maximum of {args.mean_reps})")
    scene.close(), plain.close()


def main():
    api = scenes.product_api()
    emit(f"# {args.label + ': ' if args.label else ''}k_velocity and k_taa over {args.launches} frames, Scene.render() over {args.reps} alternated pairs")
    for name in args.scenes:
        measure(api, name)


if __name__ == "__main__":
    main()
