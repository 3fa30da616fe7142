"""GPU box: what deforming a model costs (Model.skin / Model.bones), frame-only mode (Scene.render(): kernels and the
copy of the frame).  Per scene, its first model (c4: the torus, c3: diablo) under a `bend` rig -- 3 bones along the
model's longest axis, tent weights -- whose bones turn 3 degrees further on every frame; ms per frame, minimum / median of
--reps runs:

  (a) vertices   a new skinned float64 vertex array assigned on every frame (the arrays are formed before the clock
                 starts): the scene is uploaded and committed again in front of every frame.  The only way on a build
                 without Model.skin -- run this tool on the commit before the feature for the parent's figure -- and
                 still there on this one.
  (b) bones      Model.bones assigned on every frame: the pose pass with k_skin_vertices in front of every frame.
  (b') normals   the same with Skin(..., normals=True): k_skin_normals too; (b') - (b) is what the normals cost.
  (c) kernels    the device time of k_skin_vertices and k_skin_normals (HIP events, mean over 16 frames of (b')) beside
                 the pass's five spans under bones and under a plain pose in the same session.
  (d) standing   frames with nothing changing: the scene at rest, with bones left alone, with a pose left alone.

    python tools/time_skin.py --out profiles/skin_time.txt [--frames N] [--commit-frames M] [--reps R] [scene ...]
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


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def bend(model):
    """(joints, weights) of the rig: three bones along the longest axis, tent weights that sum to 1."""
    xyz = np.asarray(model.vertices, dtype=np.float64)[:, :3]
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    axis = int(np.argmax(hi - lo))
    u = 2.0 * (xyz[:, axis] - lo[axis]) / (hi[axis] - lo[axis])
    joints = np.tile(np.array([0, 1, 2, 0]), (len(xyz), 1))
    weights = np.stack([np.maximum(0.0, 1.0 - u), 1.0 - np.abs(u - 1.0), np.maximum(0.0, u - 1.0), np.zeros_like(u)], axis=1)
    return joints, weights


def bones(api, i):
    """Bone k turns k * (12 + 3 i) degrees about z and moves a few hundredths."""
    out = []
    for k in range(3):
        m = np.asarray(api.rotate_xyz((0, 0, k * (12.0 + 3.0 * i)))).astype(np.float64)
        out.append(m @ np.asarray(api.translation((0.05 * k, -0.03 * k, 0.04 * k)), dtype=np.float64))
    return np.array(out)


def skinned(vertices, joints, weights, b):
    """The skinned vertices in plain NumPy (the timing does not depend on the last bit)."""
    blend = np.einsum("nk,nkrc->nrc", weights, b[joints])
    return np.einsum("nr,nrc->nc", np.asarray(vertices).astype(np.float64), blend)


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


def mean_times(step, read, names):
    acc = dict.fromkeys(names, 0.0)
    for i in range(1, 17):
        step(i)
        for k, v in read().items():
            acc[k] += v / 16
    return acc


def measure(api, name):
    has_skin = hasattr(api.Model, "skin")
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    model = scene.models[0]
    own = model.vertices
    backend = scene._backend()
    for _ in range(4):                                              # the work lists grow to what the scene needs
        scene.render()
    standing = {"at rest": runs(lambda i: scene.render(), args.frames)}
    joints, weights = bend(model)
    arrays = [skinned(own, joints, weights, bones(api, i)) for i in range(args.commit_frames + 1)]

    def by_vertices(i):
        model.vertices = arrays[i % len(arrays)]
        scene.render()
    a = runs(by_vertices, args.commit_frames)
    model.vertices = own
    scene.render()
    emit(f"{name:22s} (a) new vertices on every frame   {a[0]:9.3f} / {a[1]:9.3f} ms per frame")
    if has_skin:
        from py_numpy_renderer_amd import Skin
        tables = [bones(api, i) for i in range(args.frames + 1)]

        def by_bones(i):
            model.bones = tables[i % len(tables)]
            scene.render()
        model.skin = Skin(joints, weights)
        b = runs(by_bones, args.frames)
        emit(f"{name:22s} (b) new bones on every frame      {b[0]:9.3f} / {b[1]:9.3f} ms per frame     (a) / (b) = {a[0] / b[0]:.1f}")
        model.skin = Skin(joints, weights, normals=True)
        b2 = runs(by_bones, args.frames)
        emit(f"{name:22s} (b') ... with normals=True        {b2[0]:9.3f} / {b2[1]:9.3f} ms per frame     (b') - (b) = "
             f"{b2[0] - b[0]:.3f} / {b2[1] - b[1]:.3f}")
        acc = mean_times(by_bones, backend.skin_times, backend.SKIN_TIME_NAMES)
        emit(f"{name:22s} (c) the skin kernels, device us   " + "  ".join(f"k_{k} {v * 1e3:.1f}" for k, v in acc.items()))
        acc = mean_times(by_bones, backend.pose_times, backend.POSE_TIME_NAMES)
        emit(f"{name:22s} (c) the pass under bones, us      " + "  ".join(f"{k} {v * 1e3:.1f}" for k, v in acc.items())
             + f"  sum {sum(acc.values()) * 1e3:.1f}   (the first span holds k_skin_vertices)")
        by_bones(1)
        standing["bones left alone"] = runs(lambda i: scene.render(), args.frames)
        model.skin = None
        scene.render()

        def by_pose(i):
            model.pose = np.asarray(api.rotate_xyz((0, 0, 3.0 * i))).astype(np.float64)
            scene.render()
        by_pose(0)
        acc = mean_times(by_pose, backend.pose_times, backend.POSE_TIME_NAMES)
        emit(f"{name:22s} (c) the pass under a pose, us     " + "  ".join(f"{k} {v * 1e3:.1f}" for k, v in acc.items())
             + f"  sum {sum(acc.values()) * 1e3:.1f}")
        standing["a pose left alone"] = runs(lambda i: scene.render(), args.frames)
        model.pose = None
    emit(f"{name:22s} (d) standing frames               " + "   ".join(f"{k} {v[0]:.4f} / {v[1]:.4f}" for k, v in standing.items())
         + " ms per frame")
    scene.close()


def main():
    api = scenes.product_api()
    emit(f"# frames {args.frames} ((a): {args.commit_frames}) x reps {args.reps}; ms per frame, minimum / median of the runs; "
         f"Model.skin {'present' if hasattr(api.Model, 'skin') else 'absent (the build before the feature)'}")
    for name in args.scenes:
        measure(api, name)


if __name__ == "__main__":
    main()
