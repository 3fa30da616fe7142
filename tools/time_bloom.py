"""GPU box: what the bloom costs (Scene.bloom) and what the same glow costs on the host.

  (k)  kernels    device us of the down chain, the up chain and the composite inside real frames (HIP events round the
                  launches, mr_debug_bloom_times): minimum / median / maximum of --launches frames, at supersample 1 and 2,
                  for Bloom(levels = 1, 4, 6) and each workgroup shape of k_bloom_down (MR_BLOOM_TILE is read once per
                  process: a fresh child of this tool times each).  Beside every span: the bytes its launches move --
                  every level read once and written once, 12 bytes a sample -- divided by the span's minimum.
  (f)  feature    Scene.render() of a scene without and of its twin with the pass, alternated frame by frame in one loop;
                  ms per frame, minimum / median of --reps, and the difference: the 2 L launches, the full resolve, the
                  taps every tile now writes.
  (h)  the host   the same glow through the float tap and tests/bloom_ref.py: render with keep_float, read_frame_f32(),
                  bloom_ref.reference(); ms, minimum / median of --host-reps.

    python tools/time_bloom.py --out profiles/bloom_time.txt [--label WORD] [--only kfh] [scene ...]
"""
import argparse
import os
import subprocess
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
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

SHAPES = ("32x8", "64x4", "16x16")
LEVELS = (1, 4, 6)


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def spread(values):
    values = sorted(values)
    return values[0], values[len(values) // 2], values[-1]


def chain_bytes(height, width, levels):
    """Bytes the down chain, the up chain and the composite move on a (height, width) sample grid: what every launch reads
    and writes once, 12 bytes a sample."""
    n = [height * width]
    for _ in range(levels):
        height, width = (height + 1) // 2, (width + 1) // 2
        n.append(height * width)
    down = sum(12 * (n[l - 1] + n[l]) for l in range(1, levels + 1))
    up = sum(12 * (2 * n[l] + n[l + 1]) for l in range(1, levels))
    composite = 12 * (2 * n[0] + n[1])
    return down, up, composite


def kernels(api, name):
    """Part (k) for the shape this process was started with."""
    import scenes
    from py_numpy_renderer_amd import Bloom
    shape = os.environ.get("MR_BLOOM_TILE", SHAPES[0])
    for s in (1, 2):
        scene = scenes.build(api, name)
        scene.draw_debug_frustum = False
        scene.supersample = s
        backend = scene._backend()
        for levels in LEVELS:
            scene.bloom = Bloom(threshold=0.5, intensity=0.5, levels=levels)
            for _ in range(3):                                   # the work lists, the float frame and the pyramid grow to what the view needs
                scene.render()
            us = {key: [] for key in backend.BLOOM_TIME_NAMES}
            for _ in range(args.launches):
                scene.render()
                for key, ms in backend.bloom_times().items():
                    us[key].append(ms * 1e3)
            _, hs, ws, on_grid = backend.bloom_debug()
            moved = dict(zip(backend.BLOOM_TIME_NAMES, chain_bytes(hs, ws, on_grid)))
            parts = []
            for key in backend.BLOOM_TIME_NAMES:
                lo, mid, hi = spread(us[key])
                rate = f", {moved[key] / 1e6:.1f} MB, {moved[key] / (lo * 1e-6) / 1e12:.2f} TB/s" if moved[key] and lo > 0 else ""
                parts.append(f"{key} {lo:.1f} / {mid:.1f} / {hi:.1f} us{rate}")
            total = spread([sum(t) for t in zip(*us.values())])
            emit(f"{name:22s} (k)  supersample {s}, Bloom(levels={levels}) = {on_grid} levels and {2 * on_grid} launches on {hs} x {ws} samples, "
                 f"k_bloom_down {shape}: " + "; ".join(parts) + f"; the pass {total[0]:.1f} / {total[1]:.1f} / {total[2]:.1f} us, "
                 f"{sum(moved.values()) / 1e6:.1f} MB, {sum(moved.values()) / (total[0] * 1e-6) / 1e12:.2f} TB/s "
                 f"(minimum / median / maximum of {args.launches} frames)")
        scene.close()


def feature(api, name):
    import scenes
    from py_numpy_renderer_amd import Bloom
    scene, plain = scenes.build(api, name), scenes.build(api, name)
    for s in (scene, plain):
        s.draw_debug_frustum = False
    for levels in LEVELS:
        scene.bloom = Bloom(threshold=0.5, intensity=0.5, levels=levels)
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
        emit(f"{name:22s} (f)  Scene.render() without / with Bloom(levels={levels}), alternated: {off[0]:.3f} / {off[1]:.3f} ms and "
             f"{with_pass[0]:.3f} / {with_pass[1]:.3f} ms (minimum / median of {args.reps}): +{with_pass[0] - off[0]:.3f} ms at the minimum, "
             f"+{with_pass[1] - off[1]:.3f} ms at the median")
    scene.close(), plain.close()


def host(api, name):
    import bloom_ref
    import scenes
    plain = scenes.build(api, name)
    plain.draw_debug_frustum = False
    backend = plain._backend()
    for levels in LEVELS:
        ms = []
        for _ in range(args.host_reps + 1):
            t0 = time.perf_counter()
            backend.render(plain, keep_float=True, counters=False, keep_buffers=True, overlay=False)
            frame = backend.read_frame_f32()
            bloom_ref.reference(frame, 0.5, 0.5, levels)
            ms.append((time.perf_counter() - t0) * 1e3)
        lo, mid, _ = spread(ms[1:])
        emit(f"{name:22s} (h)  the same glow on the host, Bloom(levels={levels}): render(keep_float), read_frame_f32() and bloom_ref.reference() "
             f"{lo:.1f} / {mid:.1f} ms (minimum / median of {args.host_reps}); the bytes of the result are not formed")
    plain.close()


def main():
    import scenes
    if args.child:
        api = scenes.product_api()
        for name in args.scenes:
            kernels(api, name)
        return
    emit(f"# {args.label + ': ' if args.label else ''}the bloom's three spans over {args.launches} frames, Scene.render() over {args.reps} alternated pairs")
    if "k" in args.only:
        for shape in SHAPES:                                    # one child at a time: each reads MR_BLOOM_TILE once
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--launches", str(args.launches), *args.scenes]
            if args.out:
                cmd += ["--out", args.out]
            proc = subprocess.run(cmd, env=dict(os.environ, MR_BLOOM_TILE=shape), timeout=600)
            if proc.returncode != 0:
                raise SystemExit(f"the child for MR_BLOOM_TILE={shape} ended with {proc.returncode}")
    api = scenes.product_api()
    for name in args.scenes:
        if "f" in args.only:
            feature(api, name)
        if "h" in args.only:
            host(api, name)


if __name__ == "__main__":
    main()
