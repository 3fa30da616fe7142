"""GPU box: what moving a model costs (Model.pose), frame-only mode (Scene.render(): kernels and the copy of the frame).
Per scene, with its first model (c4: the torus, c3: diablo) turned 3 degrees further on every frame, ms per frame,
minimum / median of --reps runs:

  (a) vertices   a new float64 vertex array assigned on every frame (the arrays are formed before the clock starts):
                 the scene is uploaded and committed again in front of every frame.  The only way on a build without
                 Model.pose -- run this tool on the commit before the feature for the parent's figure -- and still
                 there on this one.
  (b) pose       Model.pose assigned on every frame: the pose pass in front of every frame.
  (c) pass       the device time of the pass's five kernels (HIP events, mean over the frames of (b)'s last run).
  (a') both      new float64 vertices AND new float32 normals assigned on every frame (formed before the clock starts): what
                 a caller without Model.pose_normals does to have the shading normals follow -- run this tool on the
                 commit before that feature for the parent's figure.  Like (a) it uploads and commits the scene again.
  (b') normals   Model.pose assigned on every frame with Model.pose_normals on: the pose pass with its two further
                 kernels; (b') - (b) is what the normals cost.
  (c') kernels   the device time of k_pose_normals and k_pose_texels (HIP events, mean over frames of (b')).
  (d) standing   frames with nothing changing: the un-posed scene (float32 records), the scene with a pose left alone
                 and the same model committed as float64 -- the cost of float64 face and edge records, which the
                 definition of a pose accepts.

    python tools/time_pose.py --out profiles/pose_time.txt [--frames N] [--commit-frames M] [--reps R] [scene ...]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c4_torus200k_1080p", "c3_diablo_floor_1080p"])
ap.add_argument("--frames", type=int, default=100, help="frames per run of (b) and (d)")
ap.add_argument("--commit-frames", type=int, default=8, help="frames per run of (a)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()

import numpy as np
import scenes
from py_numpy_renderer_amd import _fp


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def turn(api, i):
    return np.asarray(api.rotate_xyz((0, 0, 3.0 * i))).astype(np.float64)


def runs(fn, frames):
    """ms per frame of *frames* calls of fn(i), --reps times: (minimum, median)."""
    fn(0)
    per = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for i in range(1, frames + 1):
            fn(i)
        per.append((time.perf_counter() - t0) * 1e3 / frames)
    per.sort()
    return per[0], per[len(per) // 2]


def measure(api, name):
    has_pose = hasattr(api.Model, "pose")
    has_normals = hasattr(api.Model, "pose_normals")
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    model = scene.models[0]
    own = model.vertices
    backend = scene._backend()
    for _ in range(4):                                              # the work lists grow to what the scene needs
        scene.render()

    standing = {"un-posed": runs(lambda i: scene.render(), args.frames)}

    arrays = [_fp.matmul_chain(np.asarray(own).astype(np.float64), turn(api, i)) for i in range(args.commit_frames + 1)]

    def by_vertices(i):
        model.vertices = arrays[i % len(arrays)]
        scene.render()
    a = runs(by_vertices, args.commit_frames)
    model.vertices = arrays[1]
    scene.render()
    standing["float64 model"] = runs(lambda i: scene.render(), args.frames)
    model.vertices = own
    scene.render()
    emit(f"{name:22s} (a) new vertices on every frame   {a[0]:9.3f} / {a[1]:9.3f} ms per frame")
    if model.normals is not None:
        own_normals = model.normals
        turned = [_fp.matmul_chain(np.asarray(own_normals, dtype=np.float32).astype(np.float64), turn(api, i)[:3, :3]).astype(np.float32)
                  for i in range(args.commit_frames + 1)]                  # (a rotation is its own normal matrix)

        def by_both(i):
            model.vertices, model.normals = arrays[i % len(arrays)], turned[i % len(turned)]
            scene.render()
        a2 = runs(by_both, args.commit_frames)
        model.vertices, model.normals = own, own_normals
        scene.render()
        emit(f"{name:22s} (a') new vertices and normals     {a2[0]:9.3f} / {a2[1]:9.3f} ms per frame")
    if has_pose:
        def by_pose(i):
            model.pose = turn(api, i)
            scene.render()
        b = runs(by_pose, args.frames)
        emit(f"{name:22s} (b) a new pose on every frame     {b[0]:9.3f} / {b[1]:9.3f} ms per frame     (a) / (b) = {a[0] / b[0]:.1f}")
        acc = dict.fromkeys(backend.POSE_TIME_NAMES, 0.0)
        for i in range(1, 17):
            by_pose(i)
            for k, v in backend.pose_times().items():
                acc[k] += v / 16
        emit(f"{name:22s} (c) the pass, device us           " + "  ".join(f"k_{k} {v * 1e3:.1f}" for k, v in acc.items())
             + f"  sum {sum(acc.values()) * 1e3:.1f}")
        if has_normals:
            model.pose_normals = True
            b2 = runs(by_pose, args.frames)
            emit(f"{name:22s} (b') ... with pose_normals        {b2[0]:9.3f} / {b2[1]:9.3f} ms per frame     (b') - (b) = "
                 f"{b2[0] - b[0]:.3f} / {b2[1] - b[1]:.3f}")
            acc = dict.fromkeys(backend.POSE_NORMALS_TIME_NAMES, 0.0)
            for i in range(1, 17):
                by_pose(i)
                for k, v in backend.pose_normals_times().items():
                    acc[k] += v / 16
            emit(f"{name:22s} (c') its two kernels, device us   " + "  ".join(f"k_{k} {v * 1e3:.1f}" for k, v in acc.items()))
            model.pose_normals = False
        model.pose = turn(api, 1)
        scene.render()
        standing["posed"] = runs(lambda i: scene.render(), args.frames)
        model.pose = None
    emit(f"{name:22s} (d) standing frames               " + "   ".join(f"{k} {v[0]:.4f} / {v[1]:.4f}" for k, v in standing.items())
         + " ms per frame")
    scene.close()


def main():
    api = scenes.product_api()
    emit(f"# frames {args.frames} ((a): {args.commit_frames}) x reps {args.reps}; ms per frame, minimum / median of the runs; "
         f"Model.pose {'present' if hasattr(api.Model, 'pose') else 'absent (the build before the feature)'}")
    for name in args.scenes:
        measure(api, name)


if __name__ == "__main__":
    main()
