// host_tri_reject_check.cpp -- tri_touches_tile (csrc/tri_reject.h), the rule by which k_bin_work leaves a large
// triangle out of a tile's list, held to the kernels' own coverage test on the CPU: plain C++, no HIP runtime.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -I py-numpy-renderer_amd/csrc tools/host_tri_reject_check.cpp
//       -o /tmp/host_tri_reject_check && /tmp/host_tri_reject_check [triangles per class]
//   (also with -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all)
//
// Records are built with the arithmetic of tri_setup_record (kernels_geometry.h) from seeded triangles on a 1920 x
// 1080 frame: well-shaped large ones, slivers down to a thousandth of a pixel, near-degenerate ones (den tiny), ones
// with vertices far off the screen, and c4's two floor triangles, transformed from the capture's matrices exactly as
// xform_vertex does.  For every tile of a record's box:
//   safety    if the rule rejects the tile, none of its 256 samples passes  u >= 0 && v >= 0 && w >= 0  of tri_bary
//             (float32, -ffp-contract=off, in both summation orders of the float64 dots);
//   vacuity   for a triangle with smallest angle >= 5 degrees and vertices within +-8192: a tile whose samples all lie
//             more than one pixel outside one edge's line (float64 geometry) must be rejected.
// Exit status 0 and "host_tri_reject_check: ok" when both hold over at least a million pairs (with the default count).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "tri_reject.h"

namespace {

constexpr int W = 1920, H = 1080;

// rast_math.h: chain2 / gemv2 / chain4
double chain2(double a0, double a1, double b0, double b1) { return std::fma(a1, b1, a0 * b0); }
double gemv2(double a0, double a1, double b0, double b1) { return std::fma(a0, b0, a1 * b1); }
double chain4(const double v[4], const double *m, int j)
{
    return std::fma(v[3], m[12 + j], std::fma(v[2], m[8 + j], std::fma(v[1], m[4 + j], v[0] * m[j])));
}

// tri_bary (rast_math.h) and the coverage test every consumer applies to it
bool covered(const mr::TriRec &t, int px, int py, bool single)
{
    const double rx = (double)px - t.ax, ry = (double)py - t.ay;
    const float d20 = (float)(single ? chain2(rx, ry, t.v0x, t.v0y) : gemv2(rx, ry, t.v0x, t.v0y));
    const float d21 = (float)(single ? chain2(rx, ry, t.v1x, t.v1y) : gemv2(rx, ry, t.v1x, t.v1y));
    const float v = (t.d11 * d20 - t.d01 * d21) * t.inv_den;
    const float w = (t.d00 * d21 - t.d01 * d20) * t.inv_den;
    const float u = 1.0f - v - w;
    return u >= 0 && v >= 0 && w >= 0;
}

// tri_setup_record's fields from the screen corners; false: the set-up drops the face (den == 0, no box)
bool make_record(const double sx[3], const double sy[3], mr::TriRec &t, int box[4])
{
    t = mr::TriRec{};
    t.ax = sx[0]; t.ay = sy[0];
    t.v0x = sx[1] - sx[0]; t.v0y = sy[1] - sy[0];
    t.v1x = sx[2] - sx[0]; t.v1y = sy[2] - sy[0];
    t.d00 = (float)chain2(t.v0x, t.v0y, t.v0x, t.v0y);
    t.d01 = (float)chain2(t.v0x, t.v0y, t.v1x, t.v1y);
    t.d11 = (float)chain2(t.v1x, t.v1y, t.v1x, t.v1y);
    const float den = t.d00 * t.d11 - t.d01 * t.d01;
    if (den == 0) return false;
    t.inv_den = 1.0f / den;
    // a pixel box that holds the kernels' (every sample within the corners' extent, a sample of margin, on the frame)
    const double x0 = std::fmin(sx[0], std::fmin(sx[1], sx[2])), x1 = std::fmax(sx[0], std::fmax(sx[1], sx[2]));
    const double y0 = std::fmin(sy[0], std::fmin(sy[1], sy[2])), y1 = std::fmax(sy[0], std::fmax(sy[1], sy[2]));
    if (!(x1 >= 0 && y1 >= 0 && x0 <= W && y0 <= H)) return false;
    box[0] = (int)std::fmax(std::floor(x0) - 1, 0.0); box[1] = (int)std::fmin(std::ceil(x1) + 2, (double)W);
    box[2] = (int)std::fmax(std::floor(y0) - 1, 0.0); box[3] = (int)std::fmin(std::ceil(y1) + 2, (double)H);
    return box[0] < box[1] && box[2] < box[3];
}

// smallest angle of the triangle, degrees (float64)
double min_angle(const double sx[3], const double sy[3])
{
    double best = 180.0;
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const double ax = sx[j] - sx[i], ay = sy[j] - sy[i], bx = sx[k] - sx[i], by = sy[k] - sy[i];
        best = std::fmin(best, std::atan2(std::fabs(ax * by - ay * bx), ax * bx + ay * by) * (180.0 / 3.14159265358979323846));
    }
    return best;
}

// do all samples of the tile lie more than one pixel outside the line of ONE edge?  (the distance to a line is affine:
// the four corner samples decide)
bool tile_clear_of_an_edge(const double sx[3], const double sy[3], int gx, int gy)
{
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        const double ex = sx[j] - sx[i], ey = sy[j] - sy[i], len = std::hypot(ex, ey);
        if (!(len > 0)) continue;
        const double side = (ex * (sy[k] - sy[i]) - ey * (sx[k] - sx[i])) >= 0 ? 1.0 : -1.0;     // the third corner's side is inside
        double inner = -1e300;
        for (int c = 0; c < 4; ++c) {
            const double px = gx + (c & 1) * (mr::TILE_W - 1), py = gy + (c >> 1) * (mr::TILE_H - 1);
            inner = std::fmax(inner, side * (ex * (py - sy[i]) - ey * (px - sx[i])) / len);
        }
        if (inner < -1.0) return true;
    }
    return false;
}

struct Tally { long long pairs = 0, rejected = 0, must = 0, unsafe = 0, missed = 0, triangles = 0, dropped = 0; };

void check_triangle(const double sx[3], const double sy[3], Tally &t, const char *what)
{
    mr::TriRec rec;
    int box[4];
    if (!make_record(sx, sy, rec, box)) { ++t.dropped; return; }
    ++t.triangles;
    bool strict = min_angle(sx, sy) >= 5.0;
    for (int i = 0; i < 3; ++i) strict = strict && std::fabs(sx[i]) <= 8192.0 && std::fabs(sy[i]) <= 8192.0;
    for (int ty = box[2] / mr::TILE_H; ty <= (box[3] - 1) / mr::TILE_H; ++ty)
        for (int tx = box[0] / mr::TILE_W; tx <= (box[1] - 1) / mr::TILE_W; ++tx) {
            const int gx = tx * mr::TILE_W, gy = ty * mr::TILE_H;
            const bool keep = mr::tri_touches_tile(rec, gx, gy);
            ++t.pairs;
            if (!keep) {
                ++t.rejected;
                bool any = false;
                for (int y = gy; y < gy + mr::TILE_H && !any; ++y)
                    for (int x = gx; x < gx + mr::TILE_W; ++x)
                        if (covered(rec, x, y, false) || covered(rec, x, y, true)) { any = true; break; }
                if (any) {
                    if (t.unsafe++ < 10)
                        std::printf("UNSAFE %s: tile (%d, %d) rejected, a sample is covered: (%.17g %.17g) (%.17g %.17g) (%.17g %.17g)\n",
                                    what, tx, ty, sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
                }
            }
            if (strict && tile_clear_of_an_edge(sx, sy, gx, gy)) {
                ++t.must;
                if (keep && t.missed++ < 10)
                    std::printf("MISSED %s: tile (%d, %d) lies clear of an edge and was kept: (%.17g %.17g) (%.17g %.17g) (%.17g %.17g)\n",
                                what, tx, ty, sx[0], sy[0], sx[1], sy[1], sx[2], sy[2]);
            }
        }
}

// c4's floor: the capture's mvp and viewport (tests/golden/c4_torus200k_1080p.npz, host_mvp / host_viewport), the
// floor's corners (+-2, -1, +-2) and faces (1 3 2), (1 4 3) of tests/scenes.py, through xform_vertex's arithmetic
void floor_triangles(double sx[2][3], double sy[2][3])
{
    static const double mvp[16] = {
        0x1.e3efd1ee4a225p-1, -0x1.777acde80baeap-3, -0x1.c127f0e17e3c4p-3, -0x1.bee9056fb9c39p-3,
        0x0.0p+0, 0x1.8ef27ac68c698p+0, -0x1.c127f0e17e3c4p-2, -0x1.bee9056fb9c39p-2,
        -0x1.e3efd1ee4a225p-3, -0x1.777acde80baeap-1, -0x1.c127f0e17e3c4p-1, -0x1.bee9056fb9c39p-1,
        0x0.0p+0, 0x0.0p+0, 0x1.19e4f1e5ab155p+1, 0x1.2548eb9151e86p+1 };
    static const double viewport[16] = {
        0x1.ep+9, 0, 0, 0,   0, 0x1.0ep+9, 0, 0,   0, 0, 0x1.3e66666666666p+3, 0,   0x1.ep+9, 0x1.0ep+9, 0x1.3e66666666666p+3, 1 };
    static const double corner[4][4] = { { -2, -1, -2, 1 }, { 2, -1, -2, 1 }, { 2, -1, 2, 1 }, { -2, -1, 2, 1 } };
    static const int face[2][3] = { { 0, 2, 1 }, { 0, 3, 2 } };
    for (int f = 0; f < 2; ++f)
        for (int k = 0; k < 3; ++k) {
            const double *v = corner[face[f][k]];
            double clip[4], ndc[4];
            for (int j = 0; j < 4; ++j) clip[j] = chain4(v, mvp, j);
            const double depth = 1.0 / clip[3];
            for (int j = 0; j < 4; ++j) ndc[j] = clip[j] * depth;
            sx[f][k] = chain4(ndc, viewport, 0);
            sy[f][k] = chain4(ndc, viewport, 1);
        }
}

}  // namespace

int main(int argc, char **argv)
{
    const int per_class = argc > 1 ? std::atoi(argv[1]) : 120;
    std::mt19937_64 rng(20240611);
    auto uni = [&](double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); };
    Tally all;
    const char *names[] = { "well-shaped", "sliver", "near-degenerate", "far off screen", "c4 floor" };
    for (int cls = 0; cls < 5; ++cls) {
        Tally t;
        const int n = cls == 4 ? 2 : per_class;
        double fsx[2][3], fsy[2][3];
        floor_triangles(fsx, fsy);
        for (int i = 0; i < n; ++i) {
            double sx[3], sy[3];
            if (cls == 0) {                               // large, any shape the dice give: on and around the screen
                for (int k = 0; k < 3; ++k) { sx[k] = uni(-1500, W + 1500); sy[k] = uni(-1500, H + 1500); }
            } else if (cls == 1 || cls == 2) {            // a long edge across the screen, the third corner a hair off it
                sx[0] = uni(-500, 600); sy[0] = uni(-300, H + 300);
                sx[1] = uni(W - 600, W + 500); sy[1] = uni(-300, H + 300);
                if (i & 1) {                              // (every other one from the bottom of the screen to its top)
                    sx[0] = uni(-300, W + 300); sy[0] = uni(-400, 300);
                    sx[1] = uni(-300, W + 300); sy[1] = uni(H - 300, H + 400);
                }
                const double ex = sx[1] - sx[0], ey = sy[1] - sy[0], len = std::hypot(ex, ey), s = uni(-0.2, 1.2);
                const double width = cls == 1 ? std::pow(10.0, uni(-3, 0.7)) : std::pow(10.0, uni(-13, -4));      // pixels
                const double sign = (i & 2) ? 1.0 : -1.0;
                sx[2] = sx[0] + s * ex - sign * width * ey / len; sy[2] = sy[0] + s * ey + sign * width * ex / len;
                if (cls == 2 && i % 5 == 0)               // and the tiny kind: all three corners within a millionth of a pixel
                    for (int k = 1; k < 3; ++k) { sx[k] = sx[0] + uni(-1e-6, 1e-6); sy[k] = sy[0] + uni(-1e-6, 1e-6); }
                const int r = i % 3;                      // any corner first
                std::swap(sx[0], sx[r]); std::swap(sy[0], sy[r]);
            } else if (cls == 3) {                        // corners far off the screen, negative and beyond 8 192
                const double far = std::pow(10.0, uni(3.9, 6.5));
                for (int k = 0; k < 3; ++k) { sx[k] = uni(-far, far); sy[k] = uni(-far, far); }
                if (i & 1) { sx[0] = uni(0, W); sy[0] = uni(0, H); }
                if (i % 4 == 3) { sx[1] = uni(-8192, 8192); sy[1] = uni(-8192, 8192); }
            } else {
                for (int k = 0; k < 3; ++k) { sx[k] = fsx[i][k]; sy[k] = fsy[i][k]; }
            }
            check_triangle(sx, sy, t, names[cls]);
        }
        std::printf("%-16s %6lld triangles (%lld dropped by the set-up), %8lld pairs, %8lld rejected, %8lld had to be, %lld unsafe, %lld missed\n",
                    names[cls], t.triangles, t.dropped, t.pairs, t.rejected, t.must, t.unsafe, t.missed);
        all.pairs += t.pairs; all.rejected += t.rejected; all.must += t.must; all.unsafe += t.unsafe; all.missed += t.missed;
    }
    const bool enough = argc > 1 || all.pairs >= 1000000;
    std::printf("total %lld pairs, %lld rejected, %lld had to be rejected\n", all.pairs, all.rejected, all.must);
    if (all.unsafe || all.missed || !enough || all.rejected == 0 || all.must == 0) {
        std::printf("host_tri_reject_check: FAILED (%lld unsafe, %lld missed%s)\n", all.unsafe, all.missed, enough ? "" : ", fewer than a million pairs");
        return 1;
    }
    std::printf("host_tri_reject_check: ok\n");
    return 0;
}
