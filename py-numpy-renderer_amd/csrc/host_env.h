// host_env.h -- the environment switches of the library, all of them.
//
//   name              default   meaning
//   MR_VERTEX_PATH    (inline)  mfma: vertex transform once per unique vertex on the matrix cores, as a launch of its own
//                               in front of k_setup (same bits; for A/B timing and the MFMA counters)
//   MR_RESOLVE_PATH   (fused)   separate: a supersampled frame is resolved by k_resolve_full from the float frame instead
//                               of inside k_tile (the yardstick of the fused resolve, and its A/B)
//   MR_EDGE_SPREAD    -2        lanes per edge in k_setup's edge half, as a shift: -2 by the size of the mesh, -1 dense
//                               (two edges per lane), 0 .. 4 forced
//   MR_TILE_ORDER     (auto)    rowmajor | heaviest: the order k_tile takes the tiles in (auto: see launch_tile)
//   MR_TILE_SPLIT     -1        0 | 1: sharing a heavy tile's quads out over HEAVY_SPLIT workgroups off / on for every grid
//   MR_SPLIT_COST     400       a whole frame's tile (MR_TILE_SPLIT=1: by default only small grids split) is shared out from this estimated cost ...
//   MR_SPLIT_QUADS    48        ... and this many shadow quads
//   MR_QUAD_WALK      (auto)    strips | spans: how k_tile's single-light instantiations walk a tile's shadow quads -- one quad
//                               at a time over the wavefront's strip, or sixteen (quad, row) spans to a round wherever
//                               that walk is defined (auto: by the quad and the strip, see k_tile phase 3)
//   MR_PAIR_LOG       4         0 .. 4 (mr::PAIR_LOG_K): the covered samples a lane of k_tile's small pairs logs for the winners'
//                               sweep; past them the lane walks its pairs again (0: every sample is walked again; same bits)
//   MR_CLUSTER_CULL   (auto)    0 | 1 | box | count: cluster culling off / on / boxes only / on and counted (auto: see
//                               cluster_cull_mode)
//   MR_SIL_CACHE      1         0: no frame reads or fills the silhouette cache
//   MR_BIG_TRI_REJECT 1         0: k_bin_work lists a large triangle in every tile of its box again, not only in those it can
//                               cover (tri_touches_tile; same frames, for the A/B and the tests)
//   MR_QUAD_TILE_CULL 1         0: k_tile's frame-only single-light kernels stage and classify every shadow quad a tile lists again, not
//                               only those that k_bin_work's bound lets pass against the tile's z (quad_reject.h; same frames,
//                               for the A/B and the tests).  count | count0: on | off, and those kernels leave the number of
//                               quads a tile staged in word 8 of its record (mr_debug_read_tile_records; zero otherwise)
//   MR_AO_TILE        64x64     32x32 | 64x16: the other workgroup shapes of k_ao (same bits; for the A/B)
//   MR_DOF_TILE       32x32     32x32x256 | 16x16: the other workgroup shapes of k_dof -- 32 x 32 samples with 256 threads, not
//                               1 024, or 16 x 16 samples with 256 (same bits; for the A/B)
//   MR_MBLUR_TILE     32x32     32x32x256 | 16x16: the other workgroup shapes of k_mblur, as for k_dof (same bits; for the A/B)
//   MR_TAA_TILE       32x8      64x4 | 16x16: the other workgroup shapes of k_taa, 256 threads each (same bits; for the A/B)
//   MR_BLOOM_TILE     32x8      64x4 | 16x16: the other workgroup shapes of k_bloom_down, 256 threads each (same bits; for the A/B)
//   MR_TONEMAP_HIST   atomic    ballot: k_lum_hist adds once per distinct bin of a wavefront, not once a sample (same bits; for the A/B)
//   MR_TONEMAP_GRID   256       1 .. 1024: the cap of k_lum_hist's grid, the rows of a frame slot's slab (same bits; for the A/B)
//
// MR_CLUSTER_CULL, MR_SIL_CACHE, MR_BIG_TRI_REJECT and MR_QUAD_TILE_CULL are looked up for every frame, because the tests switch them inside
// one process; the rest are read once per process.
#pragma once

namespace {

struct Env {
    bool vertex_mfma, resolve_separate, sil_cache, big_tri_reject;
    int edge_spread, tile_split, tile_order;      // tile_order: 0 auto, 1 row-major, 2 heaviest first
    int quad_tile_cull;                           // bit 0: on; bit 1: the tile records count (mr::TileArgs::quad_cull)
    int quad_walk;                                // 0 auto, 1 strips, 2 spans (mr::QUAD_WALK_*)
    int pair_log;                                 // 0 .. mr::PAIR_LOG_K
    int ao_shape, dof_shape, mblur_shape, taa_shape;   // 0 .. 2: the `shape` of ao.hip's, dof.hip's, motion.hip's and taa.hip's launch
    int bloom_shape;                              // 0 .. 2: the `shape` of bloom.hip's launch_down
    int tone_form, tone_grid;                     // the `form` and the grid cap of tonemap.hip's launch_hist
    unsigned split_cost, split_quads;
    const char *cluster_cull;                     // as set, or NULL
};

Env read_env()
{
    static const Env once = [] {
        auto is = [](const char *name, const char *value) { const char *e = getenv(name); return e && !strcmp(e, value); };
        auto number = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
        // a workgroup shape by its three spellings; unset or unknown: shape 0
        auto shape = [&](const char *name, const char *s0, const char *s1, const char *s2) {
            return is(name, s0) ? 0 : is(name, s1) ? 1 : is(name, s2) ? 2 : 0;
        };
        Env e = {};
        e.vertex_mfma = is("MR_VERTEX_PATH", "mfma");
        e.resolve_separate = is("MR_RESOLVE_PATH", "separate");
        e.edge_spread = number("MR_EDGE_SPREAD", -2);
        e.tile_order = is("MR_TILE_ORDER", "rowmajor") ? 1 : is("MR_TILE_ORDER", "heaviest") ? 2 : 0;
        e.quad_walk = is("MR_QUAD_WALK", "strips") ? 1 : is("MR_QUAD_WALK", "spans") ? 2 : 0;
        e.pair_log = std::min(std::max(number("MR_PAIR_LOG", mr::PAIR_LOG_K), 0), (int)mr::PAIR_LOG_K);
        e.tile_split = number("MR_TILE_SPLIT", -1);
        e.split_cost = (unsigned)number("MR_SPLIT_COST", 400);
        e.split_quads = (unsigned)number("MR_SPLIT_QUADS", 48);
        e.ao_shape = shape("MR_AO_TILE", "64x64", "32x32", "64x16");
        e.dof_shape = shape("MR_DOF_TILE", "32x32", "32x32x256", "16x16");
        e.mblur_shape = shape("MR_MBLUR_TILE", "32x32", "32x32x256", "16x16");
        e.taa_shape = shape("MR_TAA_TILE", "32x8", "64x4", "16x16");
        e.bloom_shape = shape("MR_BLOOM_TILE", "32x8", "64x4", "16x16");
        e.tone_form = is("MR_TONEMAP_HIST", "ballot") ? 1 : 0;
        e.tone_grid = std::min(std::max(number("MR_TONEMAP_GRID", (int)mr::TONE_HIST_BLOCKS), 1), (int)mr::TONE_MAX_BLOCKS);
        return e;
    }();
    Env e = once;
    e.cluster_cull = getenv("MR_CLUSTER_CULL");
    const char *sil = getenv("MR_SIL_CACHE");
    e.sil_cache = !(sil && !strcmp(sil, "0"));
    const char *rej = getenv("MR_BIG_TRI_REJECT");
    e.big_tri_reject = !(rej && !strcmp(rej, "0"));
    const char *cull = getenv("MR_QUAD_TILE_CULL");
    e.quad_tile_cull = !cull ? 1 : !strcmp(cull, "0") ? 0 : !strcmp(cull, "count") ? 3 : !strcmp(cull, "count0") ? 2 : 1;
    return e;
}

}  // namespace
