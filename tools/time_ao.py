"""GPU box: what ambient obscurance costs (Scene.ambient_occlusion).  Per scene at its full size and per supersample
factor in --ss:

  (k)  kernel     device us of k_ao inside real frames (HIP events round the launch, mr_debug_ao_times), minimum / median
                  of --launches frames, with its algorithmic bytes -- 8 B of z read, 12 B of colour read and 12 B written
                  per sample -- as GB/s.  MR_AO_TILE=32x32 | 64x16 in the environment times the other workgroup shapes.
  (f)  feature    Scene.render() without and with obscurance, alternated frame by frame in one loop; ms per frame,
                  minimum / median of --reps, and the difference: the kernel, the full resolve, and the taps every tile
                  now writes.
  (h)  by hand    the alternative without the feature: a frame with its taps kept, z and the float frame copied to the
                  host, the definition applied there (mr_host_ao, or --by-hand ref for tests/ao_ref.py in NumPy) and
                  finalised in NumPy.  Only for the supersample factors in --by-hand-ss.

    python tools/time_ao.py --out profiles/ao_time.txt [--label WORD] [scene ...]
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c3_diablo_floor_1080p", "c4_torus200k_1080p"])
ap.add_argument("--ss", type=int, nargs="*", default=[1, 2])
ap.add_argument("--launches", type=int, default=15)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--by-hand", choices=["mirror", "ref", "none"], default="mirror")
ap.add_argument("--by-hand-ss", type=int, nargs="*", default=[1])
ap.add_argument("--label", default="", help="a word for the header line (which build this is)")
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import scenes

HBM_GBS = 8000.0        # the HBM figure DESIGN.md uses for the MI355X


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def low_mid(values):
    values = sorted(values)
    return values[0], values[len(values) // 2]


def measure(api, name, s):
    from py_numpy_renderer_amd import AmbientOcclusion, _native, _pack
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    scene.supersample = s
    backend = scene._backend()
    ao = AmbientOcclusion()
    tag = f"{name:22s} s={s}"
    for on in (None, ao, None, ao):                      # the work lists grow to what the scene needs
        scene.ambient_occlusion = on
        scene.render()

    scene.ambient_occlusion = ao
    us = []
    for _ in range(args.launches):
        scene.render()
        us.append(backend.ao_time() * 1e3)
    _, hs, ws = backend.ao_debug()
    moved = hs * ws * 32
    lo, mid = low_mid(us)
    emit(f"{tag} (k)  k_ao ({os.environ.get('MR_AO_TILE', '64x64')} samples a workgroup) inside a frame: {lo:.1f} / {mid:.1f} us (minimum / median of "
         f"{len(us)}), {hs} x {ws} samples, {moved / 1e6:.1f} MB -> {moved / mid / 1e3:.0f} GB/s at the median (HBM: {HBM_GBS:.0f})")

    per = {False: [], True: []}
    for rep in range(args.reps):
        for on in ((False, True) if rep % 2 == 0 else (True, False)):
            scene.ambient_occlusion = ao if on else None
            t0 = time.perf_counter()
            scene.render()
            per[on].append((time.perf_counter() - t0) * 1e3)
    off, with_ao = low_mid(per[False]), low_mid(per[True])
    emit(f"{tag} (f)  Scene.render() without / with obscurance, alternated: {off[0]:.3f} / {off[1]:.3f} ms and {with_ao[0]:.3f} / {with_ao[1]:.3f} ms "
         f"(minimum / median of {args.reps}): +{with_ao[0] - off[0]:.3f} ms at the minimum, +{with_ao[1] - off[1]:.3f} ms at the median")

    if args.by_hand != "none" and s in args.by_hand_ss:
        import ao_ref
        scene.ambient_occlusion = ao
        m, k, perspective = _pack.ao_constants(scene)
        desc = _native.fill_ao_desc(ao, m, k, perspective)
        scene.ambient_occlusion = None
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            backend.render(scene, keep_float=True, counters=False, keep_buffers=True, timing=False)
            z, f = backend.read_z(), backend.read_frame_f32()
            if args.by_hand == "mirror":
                f = _native.host_ao(z, f, desc)
            else:
                f = ao_ref.apply(z, f, m, k, perspective, **ao_ref.params())
            if s > 1:
                f = f.reshape(hs // s, s, ws // s, s, 3).mean(axis=(1, 3), dtype=np.float32)
            out = (np.minimum(f, np.float32(1.0))[::-1] ** 0.8 * 255).astype(np.uint8)
            ms.append((time.perf_counter() - t0) * 1e3)
        lo, mid = low_mid(ms)
        how = "mr_host_ao" if args.by_hand == "mirror" else "ao_ref.py (NumPy)"
        emit(f"{tag} (h)  by hand: taps to the host, {how}, NumPy finalise: {lo:.1f} / {mid:.1f} ms (minimum / median of 3), frame {out.shape}")
    scene.close()


def main():
    api = scenes.product_api()
    emit(f"# {args.label + ': ' if args.label else ''}k_ao over {args.launches} frames, Scene.render() over {args.reps} alternated pairs")
    for name in args.scenes:
        for s in args.ss:
            measure(api, name, s)


if __name__ == "__main__":
    main()
