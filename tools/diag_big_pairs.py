"""Diagnostic (GPU box): per view of bench.py's camera swing, one counted frame of each scene named: the tiles that list a
big (triangle, tile) pair and cover no pixel, the big pairs summed over the tiles, and what k_bin_work rejected
(MR_BIG_TRI_REJECT=0 | 1; profiles/big_tri_reject_ab.txt)."""
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
    shadows = name not in scenes.NO_SHADOW
    views = bench.swing_cameras(api, sc, bench.N_VIEWS)
    for k, (cam, dbg) in enumerate(views):
        sc.camera, sc.debug_camera = cam, dbg
        be.render(sc, shadows=shadows)
        st = dict(be.last_stats)
        r = be.read_tile_records().astype(np.int64)
        cov, small, big, quads = r[:, 3], r[:, 5], r[:, 6], r[:, 7]
        listed = (small + big + quads) > 0
        rej = be.big_tri_rejects() if hasattr(be, "big_tri_rejects") else -1
        print(f"{name} view {k}: tiles {len(r)} | n_big>0 & covered==0: {int(((big > 0) & (cov == 0)).sum())} | sum n_big {int(big.sum())} | "
              f"listed {int(listed.sum())} listed & covered==0 {int((listed & (cov == 0)).sum())} covered>0 {int((cov > 0).sum())} | "
              f"tri_bin_entries {st['tri_bin_entries']} frag_tri {st['frag_tri']} rejects {rej}", flush=True)
    sc.close()
