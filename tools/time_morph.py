"""GPU box: what morph targets cost (Model.morph / Model.morph_weights), frame-only mode (Scene.render(): kernels and the
copy of the frame).  Per scene, its first model (c4: the torus, c3: diablo) under the `bands` shape of tests/morph_ref.py
-- five sparse targets on overlapping bands along the model's longest axis -- and under `bands50`, fifty such bands, with
weights that change on every frame; ms per frame, minimum / median of --reps runs:

  (a) vertices   a new morphed float64 vertex array assigned on every frame (the arrays are formed before the clock
                 starts): the scene is uploaded and committed again in front of every frame.  The only way on a build
                 without Model.morph -- run this tool on the commit before the feature for the parent's figure -- and
                 still there on this one.
  (b) weights    Model.morph_weights assigned on every frame: the pose pass with k_morph_vertices in front of every frame.
  (b') normals   the same with normal_targets on the normals those vertices own: k_morph_normals too.
  (c) kernels    the device time of k_morph_vertices and k_morph_normals (HIP events, mean over 16 frames of (b')) beside
                 the pass's five spans.
  (d) standing   frames with nothing changing: the scene at rest, with weights left alone.

    python tools/time_morph.py --out profiles/morph_time.txt [--frames N] [--commit-frames M] [--reps R] [scene ...]
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
ap.add_argument("--label", default="", help="a word for the header line (which build this is)")
ap.add_argument("--out", default=None, help="also append the lines to this file")
args = ap.parse_args()

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


def measure(api, name, shape):
    has_morph = hasattr(api.Model, "morph")
    scene = scenes.build(api, name)
    scene.draw_debug_frustum = False
    model = scene.models[0]
    own = model.vertices
    backend = scene._backend()
    tag = f"{name:22s} {shape:8s}"
    for _ in range(4):                                              # the work lists grow to what the scene needs
        scene.render()
    standing = {"at rest": runs(lambda i: scene.render(), args.frames)}
    targets, _, base = morph_ref.shape(model, shape)
    arrays = [morphed(own, targets, weights_of(base, i)) for i in range(args.commit_frames + 1)]

    def by_vertices(i):
        model.vertices = arrays[i % len(arrays)]
        scene.render()
    a = runs(by_vertices, args.commit_frames)
    model.vertices = own
    scene.render()
    emit(f"{tag} (a) new vertices on every frame   {a[0]:9.3f} / {a[1]:9.3f} ms per frame")
    if has_morph:
        from py_numpy_renderer_amd import Morph
        tables = [weights_of(base, i) for i in range(args.frames + 1)]

        def by_weights(i):
            model.morph_weights = tables[i % len(tables)]
            scene.render()
        model.morph = Morph(targets)
        b = runs(by_weights, args.frames)
        listed = sum(len(i) for i, _ in targets)
        emit(f"{tag} (b) new weights on every frame    {b[0]:9.3f} / {b[1]:9.3f} ms per frame     (a) / (b) = {a[0] / b[0]:.1f}"
             f"     ({len(model.vertices)} vertices, {len(targets)} targets, {listed} listed, {backend.morph_counters()[4]} entries on the device)")
        if model.normals is not None:
            owners = np.asarray(morph_ref.skin_ref.normal_owners(model))
            normal_targets = []
            for k, (index, _) in enumerate(targets):
                owned = np.flatnonzero(np.isin(owners, index))
                normal_targets.append((owned, np.tile([0.3 * np.cos(k), 0.3 * np.sin(k), 0.1], (len(owned), 1))))
            model.morph_weights = None
            model.morph = Morph(targets, normal_targets)
            b2 = runs(by_weights, args.frames)
            emit(f"{tag} (b') ... with normal_targets      {b2[0]:9.3f} / {b2[1]:9.3f} ms per frame     (b') - (b) = "
                 f"{b2[0] - b[0]:.3f} / {b2[1] - b[1]:.3f}")
        acc = mean_times(by_weights, backend.morph_times, backend.MORPH_TIME_NAMES)
        emit(f"{tag} (c) the morph kernels, device us  " + "  ".join(f"k_{k} {v * 1e3:.1f}" for k, v in acc.items()))
        acc = mean_times(by_weights, backend.pose_times, backend.POSE_TIME_NAMES)
        emit(f"{tag} (c) the pass under weights, us    " + "  ".join(f"{k} {v * 1e3:.1f}" for k, v in acc.items())
             + f"  sum {sum(acc.values()) * 1e3:.1f}   (the first span holds k_morph_vertices)")
        by_weights(1)
        standing["weights left alone"] = runs(lambda i: scene.render(), args.frames)
        model.morph = None
        scene.render()
    emit(f"{tag} (d) standing frames               " + "   ".join(f"{k} {v[0]:.4f} / {v[1]:.4f}" for k, v in standing.items())
         + " ms per frame")
    scene.close()


def main():
    api = scenes.product_api()
    emit(f"# {args.label + ': ' if args.label else ''}frames {args.frames} ((a): {args.commit_frames}) x reps {args.reps}; ms per frame, "
         f"minimum / median of the runs; Model.morph {'present' if hasattr(api.Model, 'morph') else 'absent (the build before the feature)'}")
    for name in args.scenes:
        for shape in ("bands", "bands50"):
            measure(api, name, shape)


if __name__ == "__main__":
    main()
