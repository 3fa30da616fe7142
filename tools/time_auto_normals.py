"""GPU box: what rebuilt vertex normals cost (Model.auto_normals), frame-only mode (Scene.render(): kernels and the copy
of the frame).  Per scene, its first model (c4: the torus, c3: diablo) under the `bands` shape of tests/morph_ref.py with
weights that change on every frame; ms per frame, minimum / median of --reps runs:

  (a)  arrays     new morphed float64 `vertices` and recomputed float32 `normals` arrays assigned on every frame (the
                  arrays are formed before the clock starts): the scene is uploaded and committed again in front of every
                  frame.  The only way on a build without Model.auto_normals -- run this tool with --tree on a built
                  checkout of the commit before the feature for the parent's figure.
  (b)  flag on    Model.morph_weights assigned on every frame with auto_normals = True: the pose pass with
                  k_morph_vertices and k_auto_normals in front of every frame.
  (b0) flag off   the same with auto_normals = False.
  (c)  kernel     the device time of k_auto_normals (HIP events, mean over 16 frames of (b)) beside the pass's five spans.
  (d)  lists      entries (padding included) and bytes of the face lists on the device.

    python tools/time_auto_normals.py --out profiles/auto_normals_time.txt [--tree DIR] [--label WORD] [scene ...]
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("scenes", nargs="*", default=["c4_torus200k_1080p", "c3_diablo_floor_1080p"])
ap.add_argument("--frames", type=int, default=100, help="frames per run of (b) and (b0)")
ap.add_argument("--commit-frames", type=int, default=8, help="frames per run of (a)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--tree", default=None, help="a built checkout to measure instead of this one (the commit before the feature)")
ap.add_argument("--label", default="", help="a word for the header line (which build this is)")
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()

ROOT = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np
import morph_ref
import scenes


def emit(line):
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def weights_of(base, i):
    return base + 0.06 * np.cos(np.arange(len(base)) + 0.5 * i)


def morphed(vertices, targets, weights):
    """The morphed vertices in plain NumPy (the timing does not depend on the last bit)."""
    out = np.asarray(vertices).astype(np.float64)
    for (index, delta), w in zip(targets, weights):
        out[index, :3] += w * delta
    return out


def rebuilt(model, verts):
    """Area-weighted vertex normals in plain NumPy (a face that names a normal twice counts twice: timing only)."""
    faces = np.asarray(model._faces)
    v, q = faces[..., 0] % len(verts), faces[..., 2] % len(model.normals)
    cross = np.cross(verts[v[:, 1], :3] - verts[v[:, 0], :3], verts[v[:, 2], :3] - verts[v[:, 0], :3])
    acc = np.zeros((len(model.normals), 3))
    for k in range(3):
        np.add.at(acc, q[:, k], cross)
    length = np.linalg.norm(acc, axis=1, keepdims=True)
    return np.where(length > 0, acc / np.where(length > 0, length, 1), np.asarray(model.normals)[:, :3]).astype(np.float32)


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
    has_flag = hasattr(api.Model, "auto_normals")
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    model = scene.models[0]
    own, own_normals = model.vertices, model.normals
    backend = scene._backend()
    tag = f"{name:22s}"
    for _ in range(4):                                              # the work lists grow to what the scene needs
        scene.render()
    targets, _, base = morph_ref.shape(model, "bands")
    arrays = [morphed(own, targets, weights_of(base, i)) for i in range(args.commit_frames + 1)]
    normals = [rebuilt(model, v) for v in arrays]

    def by_arrays(i):
        model.vertices, model.normals = arrays[i % len(arrays)], normals[i % len(arrays)]
        scene.render()
    a = runs(by_arrays, args.commit_frames)
    model.vertices, model.normals = own, own_normals
    scene.render()
    emit(f"{tag} (a)  new vertices and normals arrays on every frame   {a[0]:9.3f} / {a[1]:9.3f} ms per frame")
    if not has_flag:
        scene.close()
        return
    from py_numpy_renderer_amd import Morph
    tables = [weights_of(base, i) for i in range(args.frames + 1)]

    def by_weights(i):
        model.morph_weights = tables[i % len(tables)]
        scene.render()
    model.morph = Morph(targets)
    model.auto_normals = False
    b0 = runs(by_weights, args.frames)
    model.auto_normals = True
    b = runs(by_weights, args.frames)
    emit(f"{tag} (b)  new weights on every frame, auto_normals on      {b[0]:9.3f} / {b[1]:9.3f} ms per frame     (a) / (b) = {a[0] / b[0]:.1f}")
    emit(f"{tag} (b0) new weights on every frame, auto_normals off     {b0[0]:9.3f} / {b0[1]:9.3f} ms per frame     (b) - (b0) = "
         f"{b[0] - b0[0]:.3f} / {b[1] - b0[1]:.3f}")
    acc = mean_times(by_weights, backend.auto_normals_times, backend.AUTO_NORMALS_TIME_NAMES)
    emit(f"{tag} (c)  k_auto_normals, device us  " + "  ".join(f"{v * 1e3:.1f}" for v in acc.values()))
    acc = mean_times(by_weights, backend.pose_times, backend.POSE_TIME_NAMES)
    emit(f"{tag} (c)  the pass under weights, us    " + "  ".join(f"{k} {v * 1e3:.1f}" for k, v in acc.items())
         + f"  sum {sum(acc.values()) * 1e3:.1f}   (the first span holds k_morph_vertices and k_auto_normals)")
    counters = backend.auto_normals_counters()
    emit(f"{tag} (d)  lists: {counters[1]} normals, {len(model._faces)} faces, {counters[2]} entries of 4 bytes = "
         f"{counters[2] * 4} bytes on the device; {counters[3]} normals kept their authored value")
    model.morph = None
    scene.close()


def main():
    api = scenes.product_api()
    emit(f"# {args.label + ': ' if args.label else ''}frames {args.frames} ((a): {args.commit_frames}) x reps {args.reps}; ms per frame, "
         f"minimum / median of the runs; Model.auto_normals {'present' if hasattr(api.Model, 'auto_normals') else 'absent (the build before the feature)'}")
    for name in args.scenes:
        measure(api, name)


if __name__ == "__main__":
    main()
