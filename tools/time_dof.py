"""GPU box: what the one-pass depth of field costs (Scene.depth_of_field) and how far it is from the many-frame lens.

  (k)  kernel     device us of k_dof inside real frames (HIP events round the launch, mr_debug_dof_times): minimum / median /
                  maximum of --launches frames, for lenses whose largest circle of confusion is about 4 and about 8 samples,
                  one that clamps every sample at 16, and one that leaves the whole frame in focus (the pass doing
                  nothing).  MR_DOF_TILE=32x32x256 | 16x16 in the environment times the other workgroup shapes.
  (f)  feature    Scene.render() without and with the lens, alternated frame by frame in one loop; ms per frame, minimum /
                  median of --reps, and the difference: the kernel, the full resolve, and the taps every tile now writes.
  (a)  the alternative it replaces: render_mean(--sub, step) with the camera's eye jittered over the lens' disc and its
                  center held; ms, minimum / median of --mean-reps.
  (q)  quality    on --quality-scene: the float frame of the one pass against the mean of --quality-sub such sub-frames;
                  mean and largest absolute difference, over the frame, where the circle is >= 1.5 samples, where it is
                  < 0.5, and over the background; the sharp frame and an anti-aliasing-only mean beside it for scale.

    python tools/time_dof.py --out profiles/dof_time.txt [--label WORD] [--only k] [scene ...]
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c3_diablo_floor_1080p"])
ap.add_argument("--launches", type=int, default=25)
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--sub", type=int, default=16)
ap.add_argument("--mean-reps", type=int, default=7)
ap.add_argument("--quality-scene", default="diablo_floor_small")
ap.add_argument("--quality-sub", type=int, default=64)
ap.add_argument("--quality-lens", type=float, default=0.05)
ap.add_argument("--only", default="kfaq", help="which of the four parts to run")
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


def circles(scene, z, dof):
    """|s| of every sample of the z-buffer *z* under *dof*."""
    import dof_ref
    from py_numpy_renderer_amd import _pack
    scene.depth_of_field = dof
    try:
        return np.abs(dof_ref.circle(z, *_pack.dof_constants(scene)))
    finally:
        scene.depth_of_field = None


def lenses(scene, z):
    """(label, DepthOfField) for the four cases of (k): the circle is linear in lens_radius."""
    from py_numpy_renderer_amd import DepthOfField
    unit = float(circles(scene, z, DepthOfField(lens_radius=1.0)).max())
    near = float(circles(scene, z, DepthOfField(focus=0.2, lens_radius=1.0)).min())
    return [("in focus everywhere", DepthOfField(lens_radius=0.4 / unit)),
            ("largest c about 4", DepthOfField(lens_radius=4.0 / unit)),
            ("largest c about 8", DepthOfField(lens_radius=8.0 / unit)),
            ("clamped at 16 everywhere", DepthOfField(focus=0.2, lens_radius=16.5 / near))]


def jittered(api, scene, dof, n):
    """*n* cameras whose eyes lie on the lens' disc (a Vogel spiral) round the scene camera's, the center held."""
    cam = scene.camera
    eye, center = np.asarray(cam.position, dtype=np.float64), np.asarray(cam.center, dtype=np.float64)
    forward = (center - eye) / np.linalg.norm(center - eye)
    right = np.cross(forward, np.asarray(cam.up, dtype=np.float64))
    right /= np.linalg.norm(right)
    up = np.cross(right, forward)
    cams = []
    for k in range(n):
        r, phi = dof.lens_radius * np.sqrt((k + 0.5) / n), k * np.pi * (3.0 - np.sqrt(5.0))
        pos = eye + r * np.cos(phi) * right + r * np.sin(phi) * up
        cams.append(api.Camera(tuple(pos), tuple(center), fovy=cam.fovy, near=cam.near, far=cam.far, backface_culling=cam.backface_culling))
    return cams


def measure(api, name):
    from py_numpy_renderer_amd import DepthOfField
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    backend = scene._backend()
    backend.render(scene, keep_float=True, counters=False, keep_buffers=True)
    z = backend.read_z().copy()
    tag = f"{name:22s}"
    cases = lenses(scene, z)
    shape = os.environ.get("MR_DOF_TILE", "32x32")
    for label, dof in cases:
        c = np.minimum(circles(scene, z, dof), 16)
        for on in (None, dof, None, dof):                    # the work lists and both float frames grow to what the scene needs
            scene.depth_of_field = on
            scene.render()
        what = f"{label} (focus {dof.focus!r}, lens_radius {dof.lens_radius:.4g}; c from {c.min():.2f} to {c.max():.2f}, mean {c.mean():.2f})"
        if "k" in args.only:
            scene.depth_of_field = dof
            us = []
            for _ in range(args.launches):
                scene.render()
                us.append(backend.dof_time() * 1e3)
            lo, mid, hi = spread(us)
            _, hs, ws = backend.dof_debug()
            emit(f"{tag} (k)  k_dof ({shape}) {what}: {lo:.1f} / {mid:.1f} / {hi:.1f} us (minimum / median / maximum of {len(us)} frames), {hs} x {ws} samples")
        if "f" in args.only:
            per = {False: [], True: []}
            for rep in range(args.reps):
                for on in ((False, True) if rep % 2 == 0 else (True, False)):
                    scene.depth_of_field = dof if on else None
                    t0 = time.perf_counter()
                    scene.render()
                    per[on].append((time.perf_counter() - t0) * 1e3)
            off, with_dof = spread(per[False]), spread(per[True])
            emit(f"{tag} (f)  Scene.render() without / with the lens, {label}, alternated: {off[0]:.3f} / {off[1]:.3f} ms and "
                 f"{with_dof[0]:.3f} / {with_dof[1]:.3f} ms (minimum / median of {args.reps}): +{with_dof[0] - off[0]:.3f} ms at the minimum, "
                 f"+{with_dof[1] - off[1]:.3f} ms at the median")
    if "a" in args.only:
        scene.depth_of_field = None
        held = scene.camera
        dof = cases[2][1]
        ms = []
        for _ in range(args.mean_reps + 1):
            cams = jittered(api, scene, dof, args.sub)       # (a camera caches its matrices for life: new ones per picture, built outside the clock)
            t0 = time.perf_counter()
            scene.render_mean(args.sub, lambda k: setattr(scene, "camera", cams[k]))
            ms.append((time.perf_counter() - t0) * 1e3)
        scene.camera = held
        lo, mid, hi = spread(ms[1:])
        emit(f"{tag} (a)  render_mean({args.sub}, eye jittered over a lens of radius {dof.lens_radius:.4g}, center held), the cameras built "
             f"outside the clock: {lo:.2f} / {mid:.2f} / {hi:.2f} ms (minimum / median / maximum of {args.mean_reps})")
    scene.close()


def quality(api):
    from py_numpy_renderer_amd import DepthOfField
    name, n = args.quality_scene, args.quality_sub
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    backend = scene._backend()
    dof = DepthOfField(lens_radius=args.quality_lens)
    backend.render(scene, keep_float=True, counters=False, keep_buffers=True)
    z, sharp = backend.read_z().copy(), backend.read_frame_f32().copy()
    c = np.minimum(circles(scene, z, dof), 16)
    scene.depth_of_field = dof
    scene.render()
    one_pass = backend.read_frame_f32().copy()
    scene.depth_of_field = None
    held, cams = scene.camera, jittered(api, scene, dof, n)
    with scene.accumulate() as acc:
        for k in range(n):
            scene.camera = cams[k]
            acc.add(1.0)
        many = acc.float_frame() / np.float32(n)
    scene.camera = held
    # the same mean with a lens a sixteenth as wide: what the jitter does to edges and textures in focus (anti-aliasing),
    # which no single frame shares
    thin = jittered(api, scene, DepthOfField(lens_radius=dof.lens_radius / 16), n)
    with scene.accumulate() as acc:
        for k in range(n):
            scene.camera = thin[k]
            acc.add(1.0)
        aa_only = acc.float_frame() / np.float32(n)
    scene.camera = held
    covered = np.isfinite(z)
    parts = (("covered, c >= 1.5", covered & (c >= 1.5)), ("covered, c < 0.5", covered & (c < 0.5)), ("background", ~covered))
    emit(f"{name:22s} (q)  lens_radius {dof.lens_radius}, c from {c.min():.2f} to {c.max():.2f}; absolute difference of the float frames (largest "
         f"channel) against the mean of {n} sub-frames with the eye jittered over the lens, as mean / largest, over the frame and over "
         + ", ".join(f"{label} ({mask.mean():.1%} of it)" for label, mask in parts))
    for label, frame in (("the one pass", one_pass), ("the sharp frame", sharp), ("the mean over a lens 1/16 as wide", aa_only)):
        d = np.abs(frame.astype(np.float64) - many.astype(np.float64)).max(axis=-1)
        emit(f"{name:22s} (q)  {label:34s}: {d.mean():.4f} / {d.max():.4f}; " + "; ".join(f"{d[mask].mean():.4f} / {d[mask].max():.4f}" for _, mask in parts))
    scene.close()


def main():
    api = scenes.product_api()
    emit(f"# {args.label + ': ' if args.label else ''}k_dof over {args.launches} frames, Scene.render() over {args.reps} alternated pairs")
    if set(args.only) & set("kfa"):
        for name in args.scenes:
            measure(api, name)
    if "q" in args.only:
        quality(api)


if __name__ == "__main__":
    main()
