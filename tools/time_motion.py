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
  (d)  deforming  (asked for with --only d) the scene's first model skinned with the `bend` rig of tests/skin_ref.py, its
                  bones going back and forth between two frames of the rig under a still camera: device us of
                  k_face_homography and k_velocity_faces (mr_debug_motion_faces_times); Scene.render() of a scene without
                  the blur whose bones change every frame, vertex tracking off and on, alternated -- the pose pass with
                  its device-to-device copy; and Scene.render() with MotionBlur(deformation=False) and (deformation=True).

    python tools/time_motion.py --out profiles/motion_time.txt [--label WORD] [--only k] [scene ...]
    python tools/time_motion.py --out profiles/motion_faces_time.txt --only d
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


def measure_deforming(api, name):
    import skin_ref
    from py_numpy_renderer_amd import MotionBlur, Skin
    tag = f"{name:22s}"
    made = {}
    for key, blur in (("plain_off", None), ("plain_on", None), ("matrix", MotionBlur(shutter=1.0)), ("faces", MotionBlur(shutter=1.0, deformation=True))):
        s = made[key] = scenes.build(api, name)
        s.draw_debug_frustum = False
        joints, weights, _ = skin_ref.rig(api, s.models[0], "bend")
        s.models[0].skin = Skin(joints, weights)
        s.motion_blur = blur
    bones = [skin_ref.rig(api, made["faces"].models[0], "bend", frame=k)[2] for k in (0, 1)]
    n_faces, n_verts = len(made["faces"].models[0]._faces), sum(len(m.vertices) for m in made["faces"].models)

    def step(scene, k):
        scene.models[0].bones = bones[k % 2]
        scene.render()

    for k in range(4):
        for s in made.values():
            step(s, k)
    tracked = made["plain_on"]._backend()
    assert tracked.lib.mr_scene_track_vertices(tracked.handle, 1) == 0
    backend = made["faces"]._backend()
    us = {"face_homography": [], "velocity_faces": []}
    for k in range(args.launches):
        step(made["faces"], k)
        for key, ms in backend.motion_faces_times().items():
            us[key].append(ms * 1e3)
    ran, skipped, records, snapshots = backend.motion_faces_debug()
    _, hs, ws = backend.motion_debug()
    a, b = spread(us["face_homography"]), spread(us["velocity_faces"])
    covered = float((backend.read_winner() < n_faces).mean() - (backend.read_winner() < 0).mean())
    emit(f"{tag} (d)  k_face_homography {a[0]:.1f} / {a[1]:.1f} / {a[2]:.1f} us ({records} face records, 72 bytes each), k_velocity_faces "
         f"{b[0]:.1f} / {b[1]:.1f} / {b[2]:.1f} us ({hs} x {ws} samples, {covered:.1%} of them the skinned model's) (minimum / median / maximum of "
         f"{args.launches} frames; the pass ran in {ran} frames and was skipped in {skipped})")
    for label, off, on in (("no blur, the bones change every frame: vertex tracking off / on (the pose pass and its copy of "
                            f"{n_verts} vertices, {n_verts * 32} bytes)", "plain_off", "plain_on"),
                           ("the bones change every frame: MotionBlur(deformation=False) / (deformation=True)", "matrix", "faces")):
        per = {off: [], on: []}
        for rep in range(args.reps):
            for key in ((off, on) if rep % 2 == 0 else (on, off)):
                t0 = time.perf_counter()
                step(made[key], rep)
                per[key].append((time.perf_counter() - t0) * 1e3)
        x, y = spread(per[off]), spread(per[on])
        emit(f"{tag} (d)  Scene.render(), {label}, alternated: {x[0]:.3f} / {x[1]:.3f} ms and {y[0]:.3f} / {y[1]:.3f} ms (minimum / median of "
             f"{args.reps}): {y[0] - x[0]:+.3f} ms at the minimum, {y[1] - x[1]:+.3f} ms at the median")
    assert made["plain_on"]._backend().motion_faces_debug()[3] > 0 and made["plain_off"]._backend().motion_faces_debug()[3] == 0
    for s in made.values():
        s.close()


def main():
    api = scenes.product_api()
    if "d" in args.only:
        emit(f"# {args.label + ': ' if args.label else ''}the per-face velocity of a skinned model over {args.launches} frames, Scene.render() over "
             f"{args.reps} alternated pairs")
        for name in args.scenes:
            measure_deforming(api, name)
        if not set(args.only) & set("kfa"):
            return
    emit(f"# {args.label + ': ' if args.label else ''}k_velocity and k_mblur over {args.launches} frames, Scene.render() over {args.reps} alternated pairs")
    for name in args.scenes:
        measure(api, name)


if __name__ == "__main__":
    main()
