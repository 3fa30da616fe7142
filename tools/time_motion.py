"""GPU box: what the one-pass motion blur costs (Scene.motion_blur) and how far it is from the many-frame one.

  (k)  kernels    device us of k_velocity and k_mblur inside real frames (HIP events round the launches,
                  mr_debug_motion_times): minimum / median / maximum of --launches frames, for a frame at rest and for
                  camera pans (the camera turned about its place, so the sky moves with the scene) whose largest
                  half-length h is about 4, about 8 and at the clamp of 16.  The camera goes back and forth between two
                  places, so every frame of a case has the same motion.  MR_MBLUR_TILE=32x32x256 | 16x16 in the
                  environment times the other workgroup shapes.
  (f)  feature    Scene.render() of a scene without and of its twin with the blur, the same views alternated frame by
                  frame in one loop; ms per frame, minimum / median of --reps, and the difference: the two kernels, the
                  full resolve, the taps every tile now writes and the matrices the host builds.
  (a)  the alternative it replaces: render_mean(--sub, turn) over --sub cameras between the two places of the pan of 8
                  (built outside the clock); ms, minimum / median / maximum of --mean-reps.

    python tools/time_motion.py --out profiles/motion_time.txt [--label WORD] [--only k] [scene ...]
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c3_diablo_floor_1080p"])
ap.add_argument("--launches", type=int, default=24)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--sub", type=int, default=16)
ap.add_argument("--mean-reps", type=int, default=7)
ap.add_argument("--only", default="kfa", help="which of the three parts to run")
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


def half_lengths(scene, api, z, winner, face_off, cam_a, cam_b):
    """h of every sample of a frame seen through cam_b that follows one seen through cam_a (the host mirror's U)."""
    import motion_ref
    from py_numpy_renderer_amd import _native, _pack
    held = scene.camera
    scene.camera = cam_a
    previous = _pack.MotionState(scene)
    scene.camera = cam_b
    depth_map, matrices, background, class_of, _ = _pack.motion_matrices(scene, previous)
    scene.camera = held
    desc = _native.fill_motion_desc(depth_map, scene.motion_blur.shutter, matrices, background, class_of)
    return motion_ref.segment(_native.host_velocity(z, winner, face_off, desc), scene.motion_blur.shutter)[0]


def pans(api, scene, z, winner, face_off):
    """(label, camera A, camera B) of the four cases of (k): the angle whose largest h is the label's, by bisection on the
    host mirror (the frame's own z-buffer; the nearest samples and the frame's edge move most)."""
    base = scene.camera
    cases = [("at rest", base, turned(api, base, 0.0), 0.0)]
    for label, target in (("largest h about 4", 4.0), ("largest h about 8", 8.0), ("h at the clamp of 16 (largest unclamped about 20)", 20.0)):
        lo, hi = 0.0, 0.5
        for _ in range(12):
            mid = 0.5 * (lo + hi)
            u_h = half_lengths(scene, api, z, winner, face_off, base, turned(api, base, mid))
            # (h is clamped at 16: the unclamped half-length of the label comes from the share that reached the clamp)
            top = float(u_h.max()) if target <= 16 else (20.0 if (u_h >= 16).mean() > 0.95 else float(u_h.max()) * 0.5)
            lo, hi = (mid, hi) if top < target else (lo, mid)
        cases.append((label, base, turned(api, base, hi), hi))
    return cases


def measure(api, name):
    from py_numpy_renderer_amd import MotionBlur
    scene, plain = scenes.build(api, name), scenes.build(api, name)
    for s in (scene, plain):
        s.draw_debug_frustum = False
    backend = scene._backend()
    backend.render(scene, keep_float=True, counters=False, keep_buffers=True)
    z, winner = backend.read_z().copy(), backend.read_winner().copy()
    face_off = np.cumsum([0] + [len(m._faces) for m in scene.models])[:-1].astype(np.int32)
    scene.motion_blur = MotionBlur(shutter=1.0)
    tag = f"{name:22s}"
    shape = os.environ.get("MR_MBLUR_TILE", "32x32")
    cases = pans(api, scene, z, winner, face_off)
    for label, cam_a, cam_b, angle in cases:
        h = half_lengths(scene, api, z, winner, face_off, cam_a, cam_b)
        what = f"{label} (turned by {np.degrees(angle):.3f} degrees a frame; h from {h.min():.2f} to {h.max():.2f}, mean {h.mean():.2f})"
        views = (cam_a, cam_b)
        for k in range(4):                                   # the work lists and both float frames grow to what the views need
            scene.camera = plain.camera = views[k % 2]
            scene.render(), plain.render()
        if "k" in args.only:
            us = {"velocity": [], "mblur": []}
            for k in range(args.launches):
                scene.camera = views[k % 2]
                scene.render()
                for key, ms in backend.motion_times().items():
                    us[key].append(ms * 1e3)
            _, hs, ws = backend.motion_debug()
            v, b = spread(us["velocity"]), spread(us["mblur"])
            emit(f"{tag} (k)  k_velocity {v[0]:.1f} / {v[1]:.1f} / {v[2]:.1f} us, k_mblur ({shape}) {b[0]:.1f} / {b[1]:.1f} / {b[2]:.1f} us "
                 f"(minimum / median / maximum of {args.launches} frames), {hs} x {ws} samples: {what}")
        if "f" in args.only:
            per = {False: [], True: []}
            for rep in range(args.reps):
                scene.camera = plain.camera = views[rep % 2]
                for on in ((False, True) if rep % 2 == 0 else (True, False)):
                    target = scene if on else plain
                    t0 = time.perf_counter()
                    target.render()
                    per[on].append((time.perf_counter() - t0) * 1e3)
            off, with_blur = spread(per[False]), spread(per[True])
            emit(f"{tag} (f)  Scene.render() without / with the blur, {label}, alternated: {off[0]:.3f} / {off[1]:.3f} ms and "
                 f"{with_blur[0]:.3f} / {with_blur[1]:.3f} ms (minimum / median of {args.reps}): +{with_blur[0] - off[0]:.3f} ms at the minimum, "
                 f"+{with_blur[1] - off[1]:.3f} ms at the median")
    if "a" in args.only:
        _, cam_a, _, angle = cases[2]
        ms = []
        for _ in range(args.mean_reps + 1):
            cams = [turned(api, cam_a, angle * (k + 0.5) / args.sub) for k in range(args.sub)]      # (a camera caches its matrices for life)
            t0 = time.perf_counter()
            plain.render_mean(args.sub, lambda k: setattr(plain, "camera", cams[k]))
            ms.append((time.perf_counter() - t0) * 1e3)
        lo, mid, hi = spread(ms[1:])
        emit(f"{tag} (a)  render_mean({args.sub}, the camera turned in {args.sub} steps through the pan of 8), the cameras built outside the "
             f"clock: {lo:.2f} / {mid:.2f} / {hi:.2f} ms (minimum / median / maximum of {args.mean_reps})")
    scene.close(), plain.close()


def main():
    api = scenes.product_api()
    emit(f"# {args.label + ': ' if args.label else ''}k_velocity and k_mblur over {args.launches} frames, Scene.render() over {args.reps} alternated pairs")
    for name in args.scenes:
        measure(api, name)


if __name__ == "__main__":
    main()
