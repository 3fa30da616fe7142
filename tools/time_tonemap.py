"""GPU box: what the tone mapping costs (Scene.tone_map) and what the same result costs on the host.

  (s)  synthetic  the three kernels on a uniform frame (every sample one bin: the worst case of the LDS atomics) and on a
                  seeded log-uniform noise frame, through mr_debug_tone_map_post with events of its own: device us, minimum /
                  median / maximum of --launches calls, for both forms of k_lum_hist (an LDS add a sample; an add per
                  distinct bin of a wavefront) and the grid caps of --caps.  Beside k_lum_hist and k_tone_apply: the bytes
                  they move (12 a sample read; 12 read and 12 written) divided by the minimum.
  (k)  kernels    the same three spans inside real frames (mr_debug_tone_map_times), and in the same run the streaming
                  yardsticks: k_accum_add of an accumulation's second sub-frame (two reads and a write of the float frame)
                  and k_bloom_composite of a frame with bloom (12 bytes read and written a sample, and the coarse level).
  (f)  feature    Scene.render() of a scene without and of its twin with the pass, alternated frame by frame in one loop;
                  ms per frame, minimum / median of --reps, and the difference.
  (h)  the host   the same result through the float tap and tests/tonemap_ref.py: render with keep_float, read_frame_f32(),
                  tonemap_ref.tone_map(); ms, minimum / median of --host-reps.

    python tools/time_tonemap.py --out profiles/tonemap_time.txt [--label WORD] [--only skfh] [scene ...]
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c3_diablo_floor_1080p"])
ap.add_argument("--size", default="1080x1920", help="rows x columns of the synthetic frames")
ap.add_argument("--caps", default="256,512,1024", help="grid caps of k_lum_hist for part (s)")
ap.add_argument("--launches", type=int, default=24)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--only", default="skfh", help="which of the four parts to run")
ap.add_argument("--label", default="", help="a word for the header line (which build this is)")
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FORMS = ("an add a sample", "an add per distinct bin of a wavefront")


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def spread(values):
    values = sorted(values)
    return values[0], values[len(values) // 2], values[-1]


def rate(n_bytes, us):
    return f"{n_bytes / 1e6:.1f} MB, {n_bytes / (us * 1e-6) / 1e12:.2f} TB/s" if us > 0 else "no time"


def synthetic():
    import numpy as np
    import tonemap_fields as tf
    import tonemap_ref as ref
    from py_numpy_renderer_amd import _native
    lib = _native.load_library()
    handle = lib.mr_scene_create()
    h, w = (int(v) for v in args.size.split("x"))
    frames = {"uniform": tf.uniform((h, w)), "noise": tf.noise((h, w), seed=7)}
    names = _native.DeviceRenderer.TONE_MAP_TIME_NAMES
    for label, frame in frames.items():
        case = tf.Case(label, frame)
        want = case.mirror(_native)
        bins = int((want[1] > 0).sum())
        for cap in (int(c) for c in args.caps.split(",")):
            for form in (0, 1):
                us = {key: [] for key in names}
                for k in range(args.launches + 2):
                    got = _native.debug_tone_map_post(handle, frame, case.desc(_native), None, cap, form, times=True)
                    if k == 0 and tf.same(got[:3], want) != (0, 0, 0):
                        raise SystemExit(f"{label}, cap {cap}, form {form}: the kernels are not the mirror: {tf.same(got[:3], want)}")
                    if k >= 2:
                        for key, ms in got[4].items():
                            us[key].append(ms * 1e3)
                lo = {key: spread(v) for key, v in us.items()}
                n = h * w
                emit(f"{label:8s} (s)  {h} x {w}, {bins} bins hold samples, grid cap {cap}, k_lum_hist with {FORMS[form]}: "
                     f"lum_hist {lo['lum_hist'][0]:.1f} / {lo['lum_hist'][1]:.1f} / {lo['lum_hist'][2]:.1f} us ({rate(12 * n, lo['lum_hist'][0])}); "
                     f"exposure {lo['exposure'][0]:.1f} / {lo['exposure'][1]:.1f} / {lo['exposure'][2]:.1f} us; "
                     f"tone_apply {lo['tone_apply'][0]:.1f} / {lo['tone_apply'][1]:.1f} / {lo['tone_apply'][2]:.1f} us ({rate(24 * n, lo['tone_apply'][0])}) "
                     f"(minimum / median / maximum of {args.launches} calls; e = {float(want[2])!r})")
    lib.mr_scene_destroy(handle)


def kernels(api, name):
    import scenes
    from py_numpy_renderer_amd import Bloom, ToneMap
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    scene.bloom = Bloom(threshold=0.5, intensity=0.5, levels=4)
    backend = scene._backend()
    for tone in (ToneMap(), ToneMap("reinhard"), ToneMap("linear", exposure=1.5)):
        scene.tone_map = tone
        for _ in range(3):
            scene.render()
        us = {key: [] for key in backend.TONE_MAP_TIME_NAMES}
        composite = []
        for _ in range(args.launches):
            scene.render()
            for key, ms in backend.tone_map_times().items():
                us[key].append(ms * 1e3)
            composite.append(backend.bloom_times()["composite"] * 1e3)
        _, hs, ws, grid = backend.tone_map_debug()[:4]
        n = hs * ws
        lo = {key: spread(v) for key, v in us.items()}
        comp = spread(composite)
        comp_bytes = 24 * n + 12 * ((hs + 1) // 2) * ((ws + 1) // 2)
        emit(f"{name:22s} (k)  {tone!r} on {hs} x {ws} samples, k_lum_hist on {grid} workgroups (MR_TONEMAP_HIST={os.environ.get('MR_TONEMAP_HIST', 'atomic')}): "
             f"lum_hist {lo['lum_hist'][0]:.1f} / {lo['lum_hist'][1]:.1f} / {lo['lum_hist'][2]:.1f} us ({rate(12 * n, lo['lum_hist'][0])}); "
             f"exposure {lo['exposure'][0]:.1f} / {lo['exposure'][1]:.1f} / {lo['exposure'][2]:.1f} us; "
             f"tone_apply {lo['tone_apply'][0]:.1f} / {lo['tone_apply'][1]:.1f} / {lo['tone_apply'][2]:.1f} us ({rate(24 * n, lo['tone_apply'][0])}); "
             f"the yardstick k_bloom_composite of the same frames {comp[0]:.1f} / {comp[1]:.1f} / {comp[2]:.1f} us ({rate(comp_bytes, comp[0])}) "
             f"(minimum / median / maximum of {args.launches} frames)")
    scene.tone_map = None
    scene.bloom = None
    adds = []
    for _ in range(args.launches):
        with scene.accumulate() as acc:
            acc.add(1.0)
            acc.add(1.0)
            adds.append(backend.accum_times()["accum_add"] * 1e3)
    _, _, hs, ws = backend.accum_debug()
    add = spread(adds)
    emit(f"{name:22s} (k)  the yardstick k_accum_add, the second sub-frame of an accumulation on {hs} x {ws} samples: "
         f"{add[0]:.1f} / {add[1]:.1f} / {add[2]:.1f} us ({rate(36 * hs * ws, add[0])}) (minimum / median / maximum of {args.launches})")
    scene.close()


def feature(api, name):
    import scenes
    from py_numpy_renderer_amd import ToneMap
    scene, plain = scenes.build(api, name), scenes.build(api, name)
    for s in (scene, plain):
        s.draw_debug_frustum = False
    for tone in (ToneMap(), ToneMap(speed=0.5), ToneMap("linear", exposure=1.5)):
        scene.tone_map = tone
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
        emit(f"{name:22s} (f)  Scene.render() without / with {tone!r}, alternated: {off[0]:.3f} / {off[1]:.3f} ms and "
             f"{with_pass[0]:.3f} / {with_pass[1]:.3f} ms (minimum / median of {args.reps}): +{with_pass[0] - off[0]:.3f} ms at the minimum, "
             f"+{with_pass[1] - off[1]:.3f} ms at the median")
    scene.close(), plain.close()


def host(api, name):
    import scenes
    import tonemap_ref as ref
    plain = scenes.build(api, name)
    plain.draw_debug_frustum = False
    backend = plain._backend()
    ms = []
    for _ in range(args.host_reps + 1):
        t0 = time.perf_counter()
        backend.render(plain, keep_float=True, counters=False, keep_buffers=True, overlay=False)
        frame = backend.read_frame_f32()
        ref.tone_map(frame, ref.Params())
        ms.append((time.perf_counter() - t0) * 1e3)
    lo, mid, _ = spread(ms[1:])
    emit(f"{name:22s} (h)  the same result on the host: render(keep_float), read_frame_f32() and tonemap_ref.tone_map() "
         f"{lo:.1f} / {mid:.1f} ms (minimum / median of {args.host_reps}); the bytes of the result are not formed")
    plain.close()


def main():
    import scenes
    emit(f"# {args.label + ': ' if args.label else ''}the tone mapping's three kernels over {args.launches} calls and frames, Scene.render() over {args.reps} alternated pairs")
    if "s" in args.only:
        synthetic()
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
