"""GPU box: what the light shafts cost (Scene.light_shafts) and what the same rays cost on the host.

  (k)  kernels    device us of k_shaft_source, k_shaft_march and k_shaft_composite inside real frames (HIP events round the
                  launches, mr_debug_light_shafts_times): minimum / median / maximum of --launches frames, for halvings 1 and
                  2 and samples 32, 64 and 128 at supersample 1, and for halvings 2, samples 64 at supersample 2.  Beside
                  the source and the composite: the bytes they move -- the source reads 12 bytes of F and 8 of Z a sample
                  and writes 16 a coarse sample, the composite reads and writes 12 a sample and reads R, 16 a coarse sample,
                  once -- divided by the span's minimum.  Beside the march: its time per tap, and the bytes its taps ask the
                  caches for -- four corners of 16 bytes a tap -- divided by the span's minimum, next to the size of S:
                  a rate memory cannot deliver is one the caches served.
  (f)  feature    Scene.render() of a scene without and of its twin with the pass, alternated frame by frame in one loop;
                  ms per frame, minimum / median of --reps, and the difference: the three launches, the full resolve, the
                  taps every tile now writes.
  (h)  the host   the same rays through the float tap and tests/shafts_ref.py: render with keep_float, read_frame_f32(),
                  read_z(), shafts_ref.reference(); ms, minimum / median of --host-reps.

    python tools/time_shafts.py --out profiles/shafts_time.txt [--label WORD] [--only kfh] [scene ...]
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c3_diablo_floor_1080p"])
ap.add_argument("--launches", type=int, default=24)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--only", default="kfh", help="which of the three parts to run")
ap.add_argument("--label", default="", help="a word for the header line (which build this is)")
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

LIGHT = (-0.5, 0.5, -3.0)             # in front of the scenes' camera at (0.5, 1, 2) and in view, where the sky is
CONFIGS = [(1, h, n) for h in (1, 2) for n in (32, 64, 128)] + [(2, 2, 64)]      # (supersample, halvings, samples)


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def spread(values):
    values = sorted(values)
    return values[0], values[len(values) // 2], values[-1]


def lit(api, name):
    import scenes
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    scene.light = api.Light(LIGHT, ambient_strength=0.1, specular_strength=0.1)
    return scene


def kernels(api, name):
    from py_numpy_renderer_amd import LightShafts, _native
    for s, halvings, n in CONFIGS:
        scene = lit(api, name)
        scene.supersample = s
        scene.light_shafts = LightShafts(halvings=halvings, samples=n)
        backend = scene._backend()
        for _ in range(3):                                   # the work lists, the float frame, S and R grow to what the view needs
            scene.render()
        us = {key: [] for key in backend.LIGHT_SHAFTS_TIME_NAMES}
        for _ in range(args.launches):
            scene.render()
            for key, ms in backend.light_shafts_times().items():
                us[key].append(ms * 1e3)
        _, hs, ws, d = backend.light_shafts_debug()
        hd, wd = _native.shafts_level(hs, ws, d)
        fine, coarse = hs * ws, hd * wd
        source, march, composite = (spread(us[key]) for key in backend.LIGHT_SHAFTS_TIME_NAMES)
        b_source, b_composite, b_taps = 20 * fine + 16 * coarse, 24 * fine + 16 * coarse, 64 * coarse * n
        total = spread([sum(t) for t in zip(*us.values())])
        emit(f"{name:22s} (k)  supersample {s}, LightShafts(halvings={halvings}, samples={n}) = d {d} on {hs} x {ws} samples, S and R {hd} x {wd} "
             f"({16 * coarse / 1e6:.2f} MB each): source {source[0]:.1f} / {source[1]:.1f} / {source[2]:.1f} us, {b_source / 1e6:.1f} MB, "
             f"{b_source / (source[0] * 1e-6) / 1e12:.2f} TB/s; march {march[0]:.1f} / {march[1]:.1f} / {march[2]:.1f} us, "
             f"{march[0] * 1e3 / (coarse * n):.4f} ns a tap, its taps ask for {b_taps / 1e6:.0f} MB, {b_taps / (march[0] * 1e-6) / 1e12:.2f} TB/s; "
             f"composite {composite[0]:.1f} / {composite[1]:.1f} / {composite[2]:.1f} us, {b_composite / 1e6:.1f} MB, "
             f"{b_composite / (composite[0] * 1e-6) / 1e12:.2f} TB/s; the pass {total[0]:.1f} / {total[1]:.1f} / {total[2]:.1f} us "
             f"(minimum / median / maximum of {args.launches} frames)")
        scene.close()


def feature(api, name):
    from py_numpy_renderer_amd import LightShafts
    scene, plain = lit(api, name), lit(api, name)
    for halvings, n in ((2, 64), (1, 128)):
        scene.light_shafts = LightShafts(halvings=halvings, samples=n)
        for _ in range(4):
            scene.render(), plain.render()
        per = {False: [], True: []}
        for rep in range(args.reps):
            for on in ((False, True) if rep % 2 == 0 else (True, False)):
                target = scene if on else plain
                t0 = time.perf_counter()
                target.render()
                per[on].append((time.perf_counter() - t0) * 1e3)
        off, with_pass = spread(per[False]), spread(per[True])
        emit(f"{name:22s} (f)  Scene.render() without / with LightShafts(halvings={halvings}, samples={n}), alternated: {off[0]:.3f} / {off[1]:.3f} ms and "
             f"{with_pass[0]:.3f} / {with_pass[1]:.3f} ms (minimum / median of {args.reps}): +{with_pass[0] - off[0]:.3f} ms at the minimum, "
             f"+{with_pass[1] - off[1]:.3f} ms at the median")
    scene.close(), plain.close()


def host(api, name):
    import shafts_ref
    from py_numpy_renderer_amd import LightShafts, _pack
    plain = lit(api, name)
    backend = plain._backend()
    for halvings, n in ((2, 64), (1, 128)):
        plain.light_shafts = LightShafts(halvings=halvings, samples=n)
        lx, ly, t, g, _, _, d, _ = _pack.light_shafts_constants(plain)
        shafts = plain.light_shafts
        plain.light_shafts = None
        ms = []
        for _ in range(args.host_reps + 1):
            t0 = time.perf_counter()
            backend.render(plain, keep_float=True, counters=False, keep_buffers=True, overlay=False)
            frame, z = backend.read_frame_f32(), backend.read_z()
            shafts_ref.reference(frame, z, (lx, ly), g, shafts.density, shafts.decay, n, t, d)
            ms.append((time.perf_counter() - t0) * 1e3)
        lo, mid, _ = spread(ms[1:])
        emit(f"{name:22s} (h)  the same rays on the host, LightShafts(halvings={halvings}, samples={n}): render(keep_float), read_frame_f32(), read_z() and "
             f"shafts_ref.reference() {lo:.1f} / {mid:.1f} ms (minimum / median of {args.host_reps}); the bytes of the result are not formed")
    plain.close()


def main():
    import scenes
    emit(f"# {args.label + ': ' if args.label else ''}the light shafts' three spans over {args.launches} frames, Scene.render() over {args.reps} alternated pairs")
    api = scenes.product_api()
    for name in args.scenes:
        if "k" in args.only:
            kernels(api, name)
        if "f" in args.only:
            feature(api, name)
        if "h" in args.only:
            host(api, name)


if __name__ == "__main__":
    main()
