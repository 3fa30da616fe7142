// host_quad_cull_check.cpp -- the tile-level depth rule of a shadow quad (csrc/quad_reject.h: quad_tile_bound in
// k_bin_work, quad_tile_none in k_tile) held on the CPU to the two rules it stands in front of: plain C++, no HIP runtime.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -I py-numpy-renderer_amd/csrc tools/host_quad_cull_check.cpp
//       -o /tmp/host_quad_cull_check && /tmp/host_quad_cull_check [cases]
//   (also with -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all)
//
// A case is a quad's plane, a tile, a frame (near / far pair, right- or left-handed) and the float32 bound k_bin_work
// would store.  Planes run from flat (1e-9 of the depth range per pixel) to steep (the whole range in a pixel), with nz
// from 1e-12 to 1 and the record scaled by 1e-6 .. 1e6; the plane's zero line lies up to 8 192 pixels either side of
// the tile; one case in sixteen has nz == 0 or a term that is not finite; one in three lies beyond the pole of the depth,
// where every denominator is negative (the frames of a right-handed camera: the bound is then negative and the mirrored
// comparison applies).  For every case and a handful of tile limits zt around the value at which the rule starts to cull:
//   safety    if quad_tile_none culls, then (a) with a positive bound the strip rule -- quad_rect_bounds, quad_rect_sane,
//             quad_rect_verdict, as k_tile evaluates it -- says `sane` and `none` for each of the tile's four 16 x 4
//             strips at zt and at limits less favourable than zt (the strip rule knows no negative denominators: it
//             keeps such a quad and the walk finds every sample failing), and (b) with either, quad_depth_pass is false
//             at all 256 samples of the tile against zt and against its two float64 neighbours;
//   vacuity   where the tile is sane and the quad's exact depth loses at every sample by a relative 1e-6, the rule culls.
// The reciprocal is the kernels' to an ulp or two; here it is the quotient pushed up to two ulps either way, by a hash
// of the operand (the same value wherever the same nz is looked at, as on the device).
// Exit status 0 and "host_quad_cull_check: ok" when both hold over at least a million cases (with the default count).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>

namespace {
double model_rcp(double x)
{
    double r = 1.0 / x;
    if (!std::isfinite(r) || r == 0) return r;
    uint64_t b;
    std::memcpy(&b, &x, 8);
    const int step = (int)((b * 0x9e3779b97f4a7c15ull) >> 61) - 3;      // -3 .. 4, clipped to +-2
    for (int i = 0; i < std::min(std::abs(step), 2); ++i) r = std::nextafter(r, step < 0 ? -INFINITY : INFINITY);
    return r;
}
}  // namespace
#define MR_QUAD_HOST_RCP(x) model_rcp(x)
#include "quad_reject.h"

namespace {

constexpr int TW = 16, TH = 16, STRIP_H = 4;

struct Frame { double n, f; };
const Frame FRAMES[] = { { 0.1, 100.0 }, { 1.0, 1000.0 }, { 0.01, 10.0 }, { 0.5, 50000.0 }, { 2.0, 6.0 } };

struct Case {
    double nx, ny, nz, d;
    int gx, gy;
    double fpn, fmn, tnf;
    bool rh;
};

long long failures = 0, culled_neg = 0;
void fail(const char *what, const Case &c, double zt)
{
    if (++failures <= 10)
        std::printf("FAIL %s: n=(%.17g, %.17g, %.17g) d=%.17g tile=(%d, %d) fpn=%g fmn=%g tnf=%g rh=%d zt=%.17g\n", what, c.nx, c.ny, c.nz,
                    c.d, c.gx, c.gy, c.fpn, c.fmn, c.tnf, (int)c.rh, zt);
}

// the strip rule as k_tile's classification evaluates it: rejected by depth?
bool strip_none(const Case &c, int strip, double zlim)
{
    const double xa = c.gx, xb = c.gx + TW - 1, ya = c.gy + strip * STRIP_H, yb = ya + (STRIP_H - 1);
    const mr::QuadRectBounds b = mr::quad_rect_bounds(c.nx, c.ny, c.nz, c.d, xa, xb, ya, yb, c.fpn, c.fmn);
    const bool sane = mr::quad_rect_sane(b, c.nz, c.fmn, c.tnf, c.fpn);
    const mr::QuadRectVerdict v = mr::quad_rect_verdict(b, c.tnf, zlim, zlim, c.rh);
    return sane && v.none;
}

bool any_sample_passes(const Case &c, double z)
{
    const double a0 = c.fpn * c.nz, b0 = c.tnf * c.nz;          // as staged by k_tile
    for (int y = 0; y < TH; ++y)
        for (int x = 0; x < TW; ++x)
            if (mr::quad_depth_pass(c.nx, c.ny, c.nz, c.d, a0, b0, (double)(c.gx + x), (double)(c.gy + y), z, c.rh, true, c.fpn, c.fmn, c.tnf))
                return true;
    return false;
}

// safety at one tile limit; returns whether the rule culled
bool check_limit(const Case &c, float bound, double zt, long long &culled)
{
    if (!mr::quad_tile_none(bound, zt, c.tnf, c.rh)) return false;
    ++culled;
    const double inf = INFINITY;
    // limits no more favourable than zt: a smaller z in a right-handed frame, a larger one otherwise
    const double worse[] = { zt, std::nextafter(zt, c.rh ? -inf : inf), c.rh ? zt * 0.5 : zt * 2.0, c.rh ? zt - std::fabs(zt) * 3.0 : zt * 1e6,
                             c.rh ? 0.0 : 1e300, c.rh ? -inf : inf };
    // (a negative bound is the mirrored case, which the strip rule does not know: the samples alone answer for it)
    if (bound > 0)
        for (int s = 0; s < TH / STRIP_H; ++s)
            for (double zl : worse)
                if (c.rh ? zl <= zt : zl >= zt)
                    if (!strip_none(c, s, zl)) { fail("strip rule keeps what the tile rule culls", c, zl); return true; }
    if (bound < 0) ++culled_neg;
    for (double z : { zt, std::nextafter(zt, -inf), std::nextafter(zt, inf) })
        if (std::isfinite(z) && any_sample_passes(c, z)) { fail("a sample passes in a culled tile", c, z); return true; }
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    const long long cases = argc > 1 ? std::atoll(argv[1]) : 1000000;
    std::mt19937_64 rng(20240521);
    auto uni = [&](double a, double b) { return a + (b - a) * (double)(rng() >> 11) * 0x1p-53; };
    auto logu = [&](double a, double b) { return std::exp(uni(std::log(a), std::log(b))); };
    long long culled = 0, sane_tiles = 0, vac = 0, wild = 0, limits = 0;
    for (long long it = 0; it < cases; ++it) {
        Case c;
        const Frame &fr = FRAMES[rng() % (sizeof(FRAMES) / sizeof(FRAMES[0]))];
        c.fpn = fr.f + fr.n; c.fmn = fr.f - fr.n; c.tnf = 2.0 * fr.n * fr.f;
        c.rh = (rng() & 1) != 0;
        c.gx = (int)(rng() % 512) * TW; c.gy = (int)(rng() % 512) * TH;          // tiles out to 8 192
        // NDC depth -t / nz = sx (x - cx) + sy (y - cy) + dc about a point up to 8 192 pixels from the tile
        const double slope = logu(1e-9, 2.0), ang = uni(0, 6.283185307179586);
        const double sx = slope * std::cos(ang), sy = slope * std::sin(ang);
        const bool far_line = (rng() & 3) == 0;
        const double cx = c.gx + (far_line ? uni(-8192, 8192) : uni(-24, 40)), cy = c.gy + (far_line ? uni(-8192, 8192) : uni(-24, 40));
        // (one case in three beyond the pole of the depth, where every denominator is negative: a right-handed camera's frames)
        const double dc = (rng() & 7) == 0 ? uni(-3, 3) : rng() % 3 == 0 ? uni(1.2, 40.0) : uni(-1.0, 1.0);
        const double scale = logu(1e-6, 1e6);
        c.nz = ((rng() & 1) ? -1.0 : 1.0) * logu(1e-12, 1.0) * scale;
        c.nx = -sx * c.nz; c.ny = -sy * c.nz;
        c.d = -(dc - sx * cx - sy * cy) * c.nz;
        if ((rng() & 15) == 0) {                     // nz == 0, or a term that is not finite, or a denormal nz
            ++wild;
            switch (rng() % 6) {
            case 0: c.nz = 0; break;
            case 1: c.nx = INFINITY; break;
            case 2: c.d = NAN; break;
            case 3: c.nz = 4e-320; break;
            case 4: c.ny = -INFINITY; c.d = INFINITY; break;
            default: c.nz = NAN; break;
            }
        }
        const float bound = mr::quad_tile_bound(c.nx, c.ny, c.nz, c.d, c.gx, c.gy, TW, TH, c.fpn, c.fmn, c.tnf, c.rh);
        // the stored value is den_hi rounded up (den_lo rounded down), never the other way
        {
            const mr::QuadRectBounds b = mr::quad_rect_bounds(c.nx, c.ny, c.nz, c.d, c.gx, c.gx + TW - 1, c.gy, c.gy + TH - 1, c.fpn, c.fmn);
            // positive: den_hi rounded up (den_lo down); negative: den_hi rounded up towards zero (den_lo down, away from it)
            if (bound == bound && !(c.rh ? (double)bound >= b.den_hi : (double)bound <= b.den_lo) ) fail("bound rounded inwards", c, 0);
            if (bound == bound && (bound > 0) != ((c.rh ? b.den_hi : b.den_lo) > 0)) fail("bound of the wrong sign", c, 0);
            if (bound == bound) ++sane_tiles;
        }
        // tile limits around the threshold of the rule, tnf / bound, and a few that have nothing to do with it
        const double thr = bound == bound ? c.tnf / (double)bound : uni(fr.n, fr.f);
        const double worse_side = c.rh ? -1.0 : 1.0;      // a right-handed tile limit gets less favourable downwards
        const double zts[] = { std::nextafter(thr, worse_side * INFINITY), thr + worse_side * std::fabs(thr) * 3e-8, thr + worse_side * std::fabs(thr) * 0.5,
                               (thr < 0 ? -1.0 : 1.0) * uni(fr.n, fr.f), c.rh ? -1e-300 : 1e300 };
        for (double zt : zts) { ++limits; check_limit(c, bound, zt, culled); }
        // vacuity: the exact depth of the quad at its most favourable sample, and a tile z that loses against it by 1e-6
        if (bound == bound) {
            long double best = c.rh ? INFINITY : -INFINITY;
            bool ok = true;
            for (int y = 0; y < TH && ok; y += TH - 1)
                for (int x = 0; x < TW; x += TW - 1) {
                    const long double t = ((long double)c.nx * (c.gx + x) + (long double)c.ny * (c.gy + y)) + (long double)c.d;
                    const long double den = (long double)c.fpn + (t / (long double)c.nz) * (long double)c.fmn;
                    if (!(bound > 0 ? den > 0 : den < 0)) { ok = false; break; }
                    const long double zq = (long double)c.tnf / den;
                    best = c.rh ? std::fmin(best, zq) : std::fmax(best, zq);
                }
            if (ok && std::isfinite((double)best)) {
                ++vac;
                const double zt = (double)(c.rh ? best - fabsl(best) * 1e-6L : best + fabsl(best) * 1e-6L);
                if (!mr::quad_tile_none(bound, zt, c.tnf, c.rh)) fail("a quad that loses everywhere by 1e-6 is kept", c, zt);
                else check_limit(c, bound, zt, culled);
            }
        }
    }
    std::printf("host_quad_cull_check: %lld cases (%lld with nz == 0 or a term that is not finite), %lld sane tiles, %lld limits tried, "
                "%lld culls checked against the strips and the samples, %lld of them with negative denominators (the samples alone), "
                "%lld vacuity cases, %lld failures\n",
                cases, wild, sane_tiles, limits, culled, culled_neg, vac, failures);
    if (failures || cases < 1000 || culled < cases || culled_neg < cases / 4 || culled - culled_neg < cases / 4 || vac < cases / 2) { std::printf("host_quad_cull_check: FAILED\n"); return 1; }
    std::printf("host_quad_cull_check: ok\n");
    return 0;
}
