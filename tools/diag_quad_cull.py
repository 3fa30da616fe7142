"""Diagnostic (GPU box): per view of bench.py's camera swing, one frame-only frame of each scene named with
MR_QUAD_TILE_CULL=count0 and one with count (word 8 of the tile records: the shadow quads k_tile staged): the tiles that
list quads, those among them that draw a triangle (they walk their quads with the rule off), the quads they list, the
quads kept, and the tiles that skipped phase 3 altogether (profiles/quad_tile_cull_ab.txt).
    python tools/diag_quad_cull.py c4_torus200k_1080p c3_diablo_floor_1080p"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import scenes
import bench
api = scenes.product_api()
for name in sys.argv[1:]:
    sc = scenes.build(api, name)
    be = sc._backend()
    views = bench.swing_cameras(api, sc, bench.N_VIEWS)
    for k, (cam, dbg) in enumerate(views):
        sc.camera, sc.debug_camera = cam, dbg
        rec = {}
        for value in ("count0", "count"):
            os.environ["MR_QUAD_TILE_CULL"] = value
            be.render(sc, shadows=True, counters=False)
            rec[value] = be.read_tile_records().astype(np.int64)
        listed, off, on = rec["count"][:, 7], rec["count0"][:, 8], rec["count"][:, 8]
        walks = off > 0
        print(f"{name} view {k}: tiles {len(listed)} | listing quads {int((listed > 0).sum())} ({int(listed.sum())} quads) | "
              f"of them drawing a triangle {int(walks.sum())} ({int(listed[walks].sum())} quads) | quads kept {int(on.sum())} | "
              f"tiles that skipped phase 3 {int((walks & (on == 0)).sum())}", flush=True)
    os.environ.pop("MR_QUAD_TILE_CULL", None)
    sc.close()
