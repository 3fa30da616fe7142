"""CPU: the replay of k_tile's dealing rule for small pairs (tools/sim_pair_log.py) and the generated tiles of
test_pair_log_gpu.py.

The replay produced the figures the pair log (kernels_tile.h, PairLog) was sized by: how many samples the winners' sweep
walks again when a lane may log 0, 1, 2, ... covered samples.  Here it is held to two properties that follow from the
rule alone, on a reduced torus, and it tells whether the generated tiles hold the lanes they were made for.
"""
import os
import sys

import pytest

import scenes
import test_pair_log_gpu as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sim_pair_log                       # noqa: E402

LOG_K, GEN_TILE, LENGTHS, pair_log_scene = T.LOG_K, T.GEN_TILE, T.LENGTHS, T.pair_log_scene


@pytest.fixture(scope="module")
def torus(api):
    scene = scenes.torus_floor(api, resolution=(180, 320), nu=40, nv=25)
    r = sim_pair_log.replay(scene, (0, 1, 2, 3, 4, 8))
    scene.close()
    return r


def test_capacity_zero_walks_everything_again(torus):
    print({k: v for k, v in torus.items() if k != "most_in_a_pair"})
    assert torus["tiles"] > 0 and torus["walked"] > torus["covered"] > 0
    assert torus["again"][0] == torus["walked"] and torus["again_pairs"][0] == torus["lane_pairs"]


def test_walked_again_never_grows_with_the_capacity(torus):
    caps = sorted(torus["again"])
    for a, b in zip(caps, caps[1:]):
        assert torus["again"][b] <= torus["again"][a] and torus["again_pairs"][b] <= torus["again_pairs"][a], (a, b)
    assert torus["again"][caps[-1]] < torus["again"][0]


def test_generated_tiles_hold_what_they_were_made_for(api):
    """From the CPU replay of the dealing rule (tools/sim_pair_log.py), no GPU: every generated tile lists exactly its
    number of small pairs, and some lane covers exactly 1 and some lane exactly 2 samples inside one pair (capacity 1 and
    1 + 1); where 4 or 2 lanes share a pair also exactly 4 and exactly 5 (the default capacity and one more).  With 8
    lanes (lists of at most 32) a box of at most 24 samples leaves a lane at most 3: there, exactly 3."""
    for n in LENGTHS:
        scene = pair_log_scene(api, n)
        pts, boxes = sim_pair_log.screen_faces(scene)
        lists = sim_pair_log.small_lists(boxes)
        scene.close()
        assert len(lists.get(GEN_TILE, ())) == n, f"{n}: the replay lists {len(lists.get(GEN_TILE, ()))} small pairs in the tile"
        hist = {}
        for pairs in sim_pair_log.lane_walks(pts, boxes, GEN_TILE, lists[GEN_TILE]).values():
            for p in pairs:
                hist[int(sum(p))] = hist.get(int(sum(p)), 0) + 1
        print(f"{n} pairs, {sim_pair_log.lanes_per_pair(n)} lanes per pair: covered samples of a lane in one pair -> lane-pairs {dict(sorted(hist.items()))}")
        for k in (1, 2) + ((LOG_K, LOG_K + 1) if n > 32 else (3,)):
            assert hist.get(k, 0) > 0, f"{n}: no lane covers exactly {k} samples inside one pair"
