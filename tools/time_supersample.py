"""GPU box: cost of supersampled anti-aliasing (Scene.supersample).  Wall-clock ms per frame of c4 and c2 at s = 1, 2, 4,
with and without the debug-frustum overlay, through Scene.render() (one frame at a time, uint8 frame on the host) and
Scene.render_frames() (two frames in flight), for the fused resolve (in k_tile) and MR_RESOLVE_PATH=separate
(k_resolve_full from the float frame).  Each resolve path runs in a child process of its own (the library reads the
variable once).  The plain frame of the same scene at the sample grid's resolution is timed beside, for comparison.

    python tools/time_supersample.py [--frames N] [scene ...]      (default: c4_torus200k_1080p c2_diablo_1080p)
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _time(fn, frames):
    for _ in range(3):
        fn(1)
    t = time.perf_counter()
    fn(frames)
    return (time.perf_counter() - t) * 1e3 / frames


def child(path, frames, names):
    import scenes
    api = scenes.product_api()
    for name in names:
        fn, kw = {**scenes.SMALL, **scenes.FULL, **scenes.HUGE}[name]
        shadows = name not in scenes.NO_SHADOW
        h, w = kw["resolution"]
        for s in (1, 2, 4):
            for overlay in (False, True):
                for mode in ("render", "render_frames"):
                    sc = fn(api, **kw)
                    sc.supersample = s
                    sc.draw_debug_frustum = overlay
                    view = [(sc.camera, sc.debug_camera)]

                    def run(n):
                        if mode == "render":
                            for _ in range(n):
                                sc.render(shadows=shadows)
                        else:
                            for _ in sc.render_frames(view * n, shadows=shadows):
                                pass
                    ms = _time(run, frames)
                    print(f"{name:22s} s={s} overlay={int(overlay)} {mode:13s} {path:8s} {ms:8.3f} ms/frame", flush=True)
                    sc.close()
            if s > 1 and path == "fused":              # the plain frame at the sample grid's resolution
                for overlay in (False, True):
                    sc = fn(api, **{**kw, "resolution": (s * h, s * w)})
                    sc.draw_debug_frustum = overlay
                    ms = _time(lambda n: [sc.render(shadows=shadows) for _ in range(n)], frames)
                    print(f"{name:22s} plain {s * w}x{s * h} overlay={int(overlay)} render        -        {ms:8.3f} ms/frame",
                          flush=True)
                    sc.close()


def main():
    args = sys.argv[1:]
    frames = 20
    if args[:1] == ["--frames"]:
        frames, args = int(args[1]), args[2:]
    if args[:1] == ["--child"]:
        return child(args[1], frames, args[2:])
    names = args or ["c4_torus200k_1080p", "c2_diablo_1080p"]
    for path in ("fused", "separate"):
        env = dict(os.environ)
        env.pop("MR_RESOLVE_PATH", None)
        if path == "separate":
            env["MR_RESOLVE_PATH"] = "separate"
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--frames", str(frames), "--child", path, *names],
                            env=env).returncode
        if rc:
            sys.exit(rc)


if __name__ == "__main__":
    main()
