"""GPU: the edge stage of ``k_setup`` (kernels_geometry.h, ``edge_block<ML>``) at forced spreads, on small scenes.

``MR_EDGE_SPREAD`` decides which edges a lane takes: -1 two per lane (dense), s >= 0 one in every (1 << s)-th lane.
By default a small scene only ever runs s = 2, and the dense layout meets several lights only in the full-size c4
test.  Here every spread meets both edge-record layouts (``EdgeRec32`` and ``EdgeRec`` with extra incidences), one and
three lights, and -- with one light, rendered three times -- the capture epilogue and the cached path's ``quad_block``.

The variable is read once per process, so a child process per value renders and saves; this process builds the
expectation (the committed captures for one light, ``multilight_ref.compose`` over the oracle for three) and compares.
Bars, the project's: z, winner, every light's stencil and the counters exact, the silhouette exact as a set, uint8 +-1.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import scenes
from conftest import load_golden
from multilight_ref import compose, extra_lights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

SCENES = ["cube_small", "fins_nonmanifold", "torus_spot", "diablo_small"]
SPREADS = [-1, 0, 4]
FUSED, CAPTURE, CACHED = 0, 1, 2
COUNTERS = ("frag_tri", "frag_quad", "n_quads", "n_quads_drawn", "covered_px", "lit_px", "stencil_updates")

CHILD = r'''
import os, sys
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import scenes
from multilight_ref import extra_lights
COUNTERS = sys.argv[3].split(",")
api = scenes.product_api()

def frame(backend, scene, n_lights, tag, save):
    save[tag + "out"] = backend.render(scene, shadows=True, keep_float=True).copy()
    save[tag + "z"] = backend.read_z()
    save[tag + "winner"] = backend.read_winner()
    for k in range(n_lights):
        save[tag + "stencil%d" % k] = backend.read_stencil(light=k)
        save[tag + "silhouette%d" % k] = backend.read_silhouette(light=k)
    save[tag + "counters"] = np.array([backend.last_stats[c] for c in COUNTERS], dtype=np.int64)

for name in sys.argv[4:]:
    save = {}
    # one light, three frames of an unchanged light: fused, capture, cached
    scene = scenes.build(api, name)
    backend = scene._backend()
    paths = []
    for i in range(3):
        frame(backend, scene, 1, "one%d_" % i, save)
        paths.append(backend.sil_cache()[0])
    save["paths"] = np.array(paths)
    save["captures"] = np.array(backend.sil_cache()[2])
    scene.close()
    # three lights
    scene = scenes.build(api, name)
    for light in extra_lights(api)[:2]:
        scene.add_light(light)
    frame(scene._backend(), scene, 3, "three_", save)
    scene.close()
    np.savez(os.path.join(OUT, name + ".npz"), **save)
    print("ok", name)
'''


def _edge_counts(scene):
    """(unique undirected edges, most faces on one edge), per model by the raw vertex ids as the edge table is built.

    This mirrors the host's rule (csrc/host_scene.h, build_edge_table: ``edge_compact`` when every model's vertices are
    float32 and no edge has more than two incident faces); the layout the host chose is not exposed, so the test
    restates the rule.  If build_edge_table's rule changes, this and ``layout`` in ``expected`` change with it."""
    total, most = 0, 0
    for model in scene.models:
        tri = np.asarray(model._faces)[..., 0].reshape(-1, 3)
        ends = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
        unique, faces = np.unique(ends, axis=0, return_counts=True)
        total, most = total + len(unique), max(most, int(faces.max()))
    return total, most


def _sil(rows):
    return set(map(tuple, np.asarray(rows).tolist()))


@pytest.fixture(scope="module")
def expected(api, oracle_mod):
    """Per scene, computed once and left alone: the capture for one light, the composed reference for three, the edges."""
    want = {}
    for name in SCENES:
        scene = scenes.build(api, name)
        n_edges, most = _edge_counts(scene)
        f32 = all(np.asarray(m.vertices).dtype == np.float32 for m in scene.models)
        for light in extra_lights(api)[:2]:
            scene.add_light(light)
        assert len(scene.lights) == 3
        want[name] = dict(golden=load_golden(name), three=compose(oracle_mod, scene), n_edges=n_edges,
                          layout="EdgeRec32" if f32 and most <= 2 else "EdgeRec")
        scene.close()
    return want


@pytest.fixture(scope="module")
def rendered(tmp_path_factory):
    """spread -> directory of the child's .npz files; one child per spread."""
    done = {}

    def run(spread):
        if spread not in done:
            out = tmp_path_factory.mktemp("spread_" + str(spread).replace("-", "m"))
            script = out / "child.py"
            script.write_text(CHILD)
            env = dict(os.environ, MR_EDGE_SPREAD=str(spread))
            env.pop("MR_SIL_CACHE", None)
            got = subprocess.run([sys.executable, str(script), ROOT, str(out), ",".join(COUNTERS)] + SCENES, env=env,
                                 capture_output=True, text=True, timeout=300)
            assert got.returncode == 0, got.stdout[-2000:] + got.stderr[-3000:]
            assert got.stdout.count("ok ") == len(SCENES), got.stdout
            done[spread] = out
        return done[spread]
    return run


def test_the_reference_makes_the_cases_count(expected):
    """What keeps the comparisons below from passing vacuously, from the reference alone."""
    layouts = {name: expected[name]["layout"] for name in SCENES}
    print(layouts)
    assert set(layouts.values()) == {"EdgeRec32", "EdgeRec"}, layouts
    # dense: second edges exist (a lane's second edge is e[0] + 256), and some wavefront needs more than one round -- 128
    # edges per wavefront, so with more than four silhouette edges per wavefront on average one holds more than four
    d = expected["diablo_small"]
    assert d["n_edges"] > 256
    bound = 4 * math.ceil(d["n_edges"] / 128)
    g, meta = d["golden"]
    per_light = [meta["counts"]["n_quads"]] + [r.stats["n_quads"] for r in d["three"].per]
    print(f"diablo_small: {d['n_edges']} edges, bound {bound}, silhouette edges per light {per_light}")
    assert len(g["silhouette"]) == per_light[0] and all(n > bound for n in per_light), (per_light, bound)
    for name in SCENES:
        sets = [_sil(r.silhouette) for r in expected[name]["three"].per]
        assert all(sets[a] != sets[b] for a in range(3) for b in range(a)), f"{name}: two lights share a silhouette"


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("spread", SPREADS)
def test_one_light_fused_capture_and_cached(expected, rendered, spread, name):
    got = np.load(os.path.join(rendered(spread), name + ".npz"))
    g, meta = expected[name]["golden"]
    paths = got["paths"].tolist()
    print(f"spread {spread} {name}: paths {paths}, captures {int(got['captures'])}")
    # (a first frame that outgrew a work list is rendered twice, and the repeat already captures)
    assert CAPTURE in paths and paths[-1] == CACHED and int(got["captures"]) >= 1, paths
    # every counter from the reference: the capture's own counts, what its winner and stencil imply, and -- for the two
    # the capture does not record -- the oracle's run with the scene's own light alone (light 0 of the composed reference)
    covered, own = g["winner"] >= 0, expected[name]["three"].per[0].stats
    want_counters = dict(frag_tri=meta["counts"]["frag_tri_pass1"], frag_quad=meta["counts"]["frag_quad"],
                         n_quads=meta["counts"]["n_quads"], n_quads_drawn=own["n_quads_drawn"],
                         covered_px=int(covered.sum()), lit_px=int((covered & (g["stencil"] == 0)).sum()),
                         stencil_updates=own["stencil_updates"])
    for i, path in enumerate(paths):
        tag, label = f"one{i}_", f"spread {spread} {name} frame {i} (path {path})"
        assert np.array_equal(got[tag + "z"].view(np.uint64), g["z"].view(np.uint64)), f"{label}: z"
        assert np.array_equal(got[tag + "winner"], g["winner"]), f"{label}: winner"
        assert np.array_equal(got[tag + "stencil0"], g["stencil"]), f"{label}: stencil"
        assert len(got[tag + "silhouette0"]) == len(g["silhouette"]), f"{label}: silhouette length"
        assert _sil(got[tag + "silhouette0"]) == _sil(g["silhouette"]), f"{label}: silhouette"
        counters = dict(zip(COUNTERS, got[tag + "counters"].tolist()))
        print(f"  frame {i}: {counters}")
        assert counters == want_counters, f"{label}: counters, expected {want_counters}"
        worst = int(np.abs(got[tag + "out"].astype(np.int16) - g["out"].astype(np.int16)).max())
        assert worst <= 1, f"{label}: uint8 off by {worst}"


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("spread", SPREADS)
def test_three_lights(expected, rendered, spread, name):
    got = np.load(os.path.join(rendered(spread), name + ".npz"))
    ref = expected[name]["three"]
    label = f"spread {spread} {name}"
    covered = ref.winner >= 0
    assert np.array_equal(got["three_z"].view(np.uint64), ref.z.view(np.uint64)), f"{label}: z"
    assert np.array_equal(got["three_winner"], ref.winner), f"{label}: winner"
    for k, r in enumerate(ref.per):
        assert np.array_equal(got[f"three_stencil{k}"], r.stencil), f"{label}: stencil of light {k}"
        assert len(got[f"three_silhouette{k}"]) == r.stats["n_quads"], f"{label}: silhouette length of light {k}"
        assert _sil(got[f"three_silhouette{k}"]) == _sil(r.silhouette), f"{label}: silhouette of light {k}"
    st = dict(zip(COUNTERS, got["three_counters"].tolist()))
    print(f"{label}: {st}")
    assert st["frag_tri"] == ref.per[0].stats["frag_tri_pass1"]
    assert st["covered_px"] == int(covered.sum())
    for key in ("frag_quad", "n_quads", "n_quads_drawn", "stencil_updates"):
        assert st[key] == sum(r.stats[key] for r in ref.per), f"{label}: {key}"
    assert st["lit_px"] == sum(int((covered & (r.stencil == 0)).sum()) for r in ref.per)
    worst = int(np.abs(got["three_out"].astype(np.int16) - ref.out.astype(np.int16)).max())
    assert worst <= 1, f"{label}: uint8 off by {worst}"
