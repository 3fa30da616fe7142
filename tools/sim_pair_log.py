"""CPU replay of how k_tile deals the samples of a tile's small (triangle, tile) pairs to its lanes (kernels_tile.h,
phase 2), and of what the winners' sweep has to walk again for a given capacity of the lanes' logs (PairLog).

An estimate, not the kernel: the lists are taken in face order (the device fills them in the order its atomics land),
coverage is plain float64 barycentrics at the integer sample positions (the kernel's are rounded to float32), and no face
is assumed to need the per-fragment clip test (such a face is a big pair whatever its box).  What it shares with the
kernel is the rule: pixel boxes as ceil(min) .. ceil(max) clamped to the frame, 16 x 16 tiles, a pair small when its box
inside the tile holds at most BIG_PAIR_PX samples, 8 / 4 / 2 lanes per pair by the list length (<= 32, <= 64, more), pair
i of the list in round i // (256 / lanes), the box's samples dealt to the pair's lanes round-robin in row-major order, a
log entry per covered sample through all rounds, and -- from the first covered sample that does not fit -- everything the
lane walks walked again.  Capacity 0 walks everything again, from the lane's first sample.

    python3 tools/sim_pair_log.py [recipe of tests/scenes.py] [tiles to sample, 0 = all]
"""
import os
import sys

import numpy as np

TILE, TILE_PX, BIG_PAIR_PX = 16, 256, 24


def lanes_per_pair(n_small):
    return 2 if n_small > 64 else 4 if n_small > 32 else 8


def screen_faces(scene):
    """(F, 3, 2) float64 screen corners and the pixel boxes (F, 4) as x0, x1, y0, y1 of the faces that survive the cull
    and have a box; in face order, models in order."""
    cam = scene.camera
    h, w = scene.resolution
    pts, boxes = [], []
    for model in scene.models:
        corners = np.asarray(model._faces)[:, :, 0]
        clip = np.asarray(model.vertices, dtype=np.float64)[corners] @ cam.MVP
        with np.errstate(divide="ignore", invalid="ignore"):
            screen = (clip / clip[..., 3:4]) @ cam.viewport
        xy = screen[..., :2]
        e1, e2 = xy[:, 1] - xy[:, 0], xy[:, 2] - xy[:, 0]
        n_z = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        lo = np.ceil(np.maximum(xy.min(axis=1), 0))
        hi = np.ceil(np.minimum(xy.max(axis=1), (w, h)))
        keep = np.isfinite(xy).all(axis=(1, 2)) & (hi > lo).all(axis=1) & (n_z != 0)
        if cam.backface_culling:
            keep &= n_z > 0
        pts.append(xy[keep])
        boxes.append(np.stack([lo[keep, 0], hi[keep, 0], lo[keep, 1], hi[keep, 1]], axis=1).astype(np.int64))
    return np.concatenate(pts), np.concatenate(boxes)


def small_lists(boxes):
    """tile (tx, ty) -> indices of the faces whose pair with the tile is small, in face order."""
    lists = {}
    for f, (x0, x1, y0, y1) in enumerate(boxes.tolist()):
        for ty in range(y0 // TILE, (y1 - 1) // TILE + 1):
            for tx in range(x0 // TILE, (x1 - 1) // TILE + 1):
                bw = min(x1, tx * TILE + TILE) - max(x0, tx * TILE)
                bh = min(y1, ty * TILE + TILE) - max(y0, ty * TILE)
                if bw * bh <= BIG_PAIR_PX:
                    lists.setdefault((tx, ty), []).append(f)
    return lists


def covered(tri, x, y):
    (ax, ay), (bx, by), (cx, cy) = tri
    den = (by - cy) * (ax - cx) + (cx - bx) * (ay - cy)
    u = ((by - cy) * (x - cx) + (cx - bx) * (y - cy)) / den
    v = ((cy - ay) * (x - cx) + (ax - cx) * (y - cy)) / den
    return u >= 0 and v >= 0 and 1 - u - v >= 0


def lane_walks(pts, boxes, tile, faces):
    """One tile's small pairs as the lanes walk them: thread -> list over its rounds of the pair's coverage flags, one
    flag per sample in the order the lane walks them."""
    tx, ty = tile
    spl = lanes_per_pair(len(faces))
    per_round = TILE_PX // spl
    threads = {}
    for i, f in enumerate(faces):
        x0, x1, y0, y1 = boxes[f].tolist()
        x0, x1 = max(x0, tx * TILE), min(x1, tx * TILE + TILE)
        y0, y1 = max(y0, ty * TILE), min(y1, ty * TILE + TILE)
        bw = x1 - x0
        samples = [(x0 + k % bw, y0 + k // bw) for k in range(bw * (y1 - y0))]
        for sub in range(spl):
            flags = [covered(pts[f], x, y) for x, y in samples[sub::spl]]
            threads.setdefault((i % per_round) * spl + sub, []).append(flags)
    return threads


def replay_lane(pairs, capacity):
    """(samples walked, samples covered, lane-pairs walked again, samples walked again) of one lane."""
    walked = sum(len(p) for p in pairs)
    n_cov = sum(sum(p) for p in pairs)
    logged, again_pairs, again = 0, 0, 0
    resumed = capacity == 0
    for flags in pairs:
        if resumed:
            again_pairs += 1
            again += len(flags)
            continue
        for pos, c in enumerate(flags):
            if not c:
                continue
            if logged < capacity:
                logged += 1
            else:
                resumed = True
                again_pairs += 1
                again += len(flags) - pos
                break
    return walked, n_cov, again_pairs, again


def replay(scene, capacities, n_tiles=0, seed=0):
    """dict of totals over the tiles that list small pairs (*n_tiles* random ones of them, 0 = all): tiles, lane_pairs,
    walked, covered, and per capacity c ``again_pairs[c]`` / ``again[c]``; ``most_in_a_pair`` maps a capacity-free
    histogram: covered samples of a lane inside one pair -> how many lane-pairs."""
    pts, boxes = screen_faces(scene)
    lists = small_lists(boxes)
    tiles = sorted(lists)
    if n_tiles and n_tiles < len(tiles):
        pick = np.random.default_rng(seed).choice(len(tiles), n_tiles, replace=False)
        tiles = [tiles[k] for k in sorted(pick.tolist())]
    tot = dict(tiles=len(lists), sampled=len(tiles), lane_pairs=0, walked=0, covered=0, longest=max(map(len, lists.values()), default=0),
               again_pairs={c: 0 for c in capacities}, again={c: 0 for c in capacities}, most_in_a_pair={})
    for t in tiles:
        for pairs in lane_walks(pts, boxes, t, lists[t]).values():
            tot["lane_pairs"] += len(pairs)
            for p in pairs:
                tot["most_in_a_pair"][sum(p)] = tot["most_in_a_pair"].get(sum(p), 0) + 1
            for c in capacities:
                walked, n_cov, again_pairs, again = replay_lane(pairs, c)
                tot["again_pairs"][c] += again_pairs
                tot["again"][c] += again
            tot["walked"] += walked
            tot["covered"] += n_cov
    return tot


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "tests")]
    import scenes
    name = sys.argv[1] if len(sys.argv) > 1 else "c4_torus200k_1080p"
    scene = scenes.build(scenes.product_api(), name)
    scene.models = scene.models[:1]                      # the mesh; the floor's pairs are big
    r = replay(scene, (0, 1, 2, 3, 4), int(sys.argv[2]) if len(sys.argv) > 2 else 400)
    print(f"{name}: {r['tiles']} tiles list small pairs (longest list {r['longest']}), {r['sampled']} replayed: "
          f"{r['lane_pairs']} lane-pairs, {r['walked']} samples walked, {r['covered']} covered")
    for c in sorted(r["again"]):
        print(f"  log of {c}: {r['again_pairs'][c]} lane-pairs / {r['again'][c]} samples walked again")
