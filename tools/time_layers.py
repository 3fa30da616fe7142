"""GPU box: what the data layers cost (Scene.layers) and what the same arrays cost through the taps and NumPy.

  (k)  kernels    k_layers inside real frames (mr_debug_layers_times) with all nine layers and with depth alone; device us,
                  minimum / median / maximum of --launches frames, beside the bytes it moves (4 read and 4, 8 or 12 written a
                  sample and layer) divided by the minimum.  In the same run the streaming yardstick: k_tone_apply of the
                  same frames (12 bytes read and written a sample).
  (f)  feature    Scene.render() of a scene without and of its twin with the pass, alternated frame by frame in one loop;
                  ms per frame, minimum / median of --reps, and the difference; then the same with read_layers() behind
                  every frame of the twin (the host copy).
  (h)  the host   the same layers through the taps and tests/layers_ref.py: render with keep_buffers, read_winner(), the
                  face records, layers_ref.layers(); ms, minimum / median of --host-reps.

    python tools/time_layers.py --out profiles/layers_time.txt [--label WORD] [--only kfh] [scene ...]
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c4_torus200k_1080p"])
ap.add_argument("--launches", type=int, default=24)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--host-reps", type=int, default=2)
ap.add_argument("--only", default="kfh", help="which of the three parts to run")
ap.add_argument("--label", default="", help="a word for the header line (which build this is)")
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ALL = ("model", "face", "material", "barycentric", "depth", "position", "face_normal", "normal", "uv")
WORDS = dict(zip(ALL, (1, 1, 1, 3, 1, 3, 3, 3, 2)))


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


def kernels(api, name):
    import scenes
    from py_numpy_renderer_amd import Layers, ToneMap
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    scene.tone_map = ToneMap("linear", exposure=1.5)
    backend = scene._backend()
    for names in (ALL, ("depth",), ("model", "face", "material"), ("depth", "normal")):
        scene.layers = Layers(names)
        for _ in range(3):
            scene.render()
        us, apply = [], []
        for _ in range(args.launches):
            scene.render()
            us.append(backend.layers_time() * 1e3)
            apply.append(backend.tone_map_times()["tone_apply"] * 1e3)
        _, hs, ws, mask = backend.layers_debug()
        n = hs * ws
        lo, tone = spread(us), spread(apply)
        moved = n * 4 * (1 + sum(WORDS[k] for k in names))
        covered = float((backend.read_winner() >= 0).mean())
        emit(f"{name:22s} (k)  k_layers with {', '.join(names)} (mask {mask:#x}) on {hs} x {ws} samples, {100 * covered:.0f} % covered: "
             f"{lo[0]:.1f} / {lo[1]:.1f} / {lo[2]:.1f} us ({rate(moved, lo[0])}, the records not counted); the yardstick k_tone_apply of the same "
             f"frames {tone[0]:.1f} / {tone[1]:.1f} / {tone[2]:.1f} us ({rate(24 * n, tone[0])}) (minimum / median / maximum of {args.launches} frames)")
    scene.close()


def feature(api, name):
    import scenes
    from py_numpy_renderer_amd import Layers
    scene, plain = scenes.build(api, name), scenes.build(api, name)
    for s in (scene, plain):
        s.draw_debug_frustum = False
    for names in (ALL, ("depth",)):
        scene.layers = Layers(names)
        for copy in (False, True):
            for _ in range(4):
                scene.render(), plain.render()
            per = {False: [], True: []}
            for rep in range(args.reps):
                for on in ((False, True) if rep % 2 == 0 else (True, False)):
                    target = scene if on else plain
                    t0 = time.perf_counter()
                    target.render()
                    if on and copy:
                        target.read_layers()
                    per[on].append((time.perf_counter() - t0) * 1e3)
            off, with_pass = spread(per[False]), spread(per[True])
            emit(f"{name:22s} (f)  Scene.render() without / with Layers({', '.join(names)}){' and read_layers()' if copy else ''}, alternated: "
                 f"{off[0]:.3f} / {off[1]:.3f} ms and {with_pass[0]:.3f} / {with_pass[1]:.3f} ms (minimum / median of {args.reps}): "
                 f"+{with_pass[0] - off[0]:.3f} ms at the minimum, +{with_pass[1] - off[1]:.3f} ms at the median")
    scene.close(), plain.close()


def host(api, name):
    import numpy as np
    import layers_ref as ref
    import scenes
    from py_numpy_renderer_amd import _pack
    plain = scenes.build(api, name)
    plain.draw_debug_frustum = False
    backend = plain._backend()
    backend.render(plain, counters=False, keep_buffers=True, overlay=False)
    pos, attr = backend.read_face_records()            # (the records once: a static scene keeps them)
    face_off = np.cumsum([0] + [len(m._faces) for m in plain.models[:-1]]).astype(np.int32)
    ms = []
    for _ in range(args.host_reps + 1):
        t0 = time.perf_counter()
        backend.render(plain, counters=False, keep_buffers=True, overlay=False)
        winner = backend.read_winner()
        ref.layers(winner, pos, attr, face_off, _pack.layer_matrix(plain))
        ms.append((time.perf_counter() - t0) * 1e3)
    lo, mid, _ = spread(ms[1:])
    emit(f"{name:22s} (h)  the same nine layers on the host: render(keep_buffers), read_winner() and layers_ref.layers() "
         f"{lo:.1f} / {mid:.1f} ms (minimum / median of {args.host_reps})")
    plain.close()


def main():
    import scenes
    emit(f"# {args.label + ': ' if args.label else ''}k_layers over {args.launches} frames, Scene.render() over {args.reps} alternated pairs")
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
