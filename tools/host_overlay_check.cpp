// host_overlay_check.cpp -- the host's count of a segment's distinct overlay targets (csrc/host_overlay.h:
// count_distinct_targets, mark_overlay_segments) under the sanitizers, on the CPU: plain C++, no HIP runtime.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I py-numpy-renderer_amd/csrc tools/host_overlay_check.cpp -o /tmp/host_overlay_check && /tmp/host_overlay_check
//
// Exit status 0 and "host_overlay_check: ok" when every count is the expected one and the sanitizers saw nothing.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "host_overlay.h"

namespace {

constexpr int32_t LDS_POINTS = 4096, MAX_TARGETS = 12288, FLAG = 1 << 30;      // kernels_overlay.h

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

// (5, n) targets of the points (row, col), neighbours clipped to the frame
std::vector<int32_t> targets_of(const std::vector<int> &rows, const std::vector<int> &cols, int height, int width)
{
    const size_t n = rows.size();
    std::vector<int32_t> t(5 * n);
    auto clamp = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
    for (size_t i = 0; i < n; ++i) {
        const int r = rows[i], c = cols[i];
        t[0 * n + i] = r * width + c;
        t[1 * n + i] = clamp(r - 1, height - 1) * width + c;
        t[2 * n + i] = r * width + clamp(c - 1, width - 1);
        t[3 * n + i] = clamp(r + 1, height - 1) * width + c;
        t[4 * n + i] = r * width + clamp(c + 1, width - 1);
    }
    return t;
}

int32_t distinct_by_set(const std::vector<int32_t> &t, size_t n, int32_t first, int32_t count)
{
    std::set<int32_t> seen;
    for (int k = 0; k < 5; ++k)
        for (int32_t i = 0; i < count; ++i) seen.insert(t[k * n + (size_t)first + (size_t)i]);
    return (int32_t)seen.size();
}

}  // namespace

int main()
{
    mr_host::OverlayCountWork ws;

    // the plus lattice (row + 2 * col) % 5 == 0 of the interior of a 120 x 160 frame: 3729 points, 18 645 targets
    const int H = 120, W = 160;
    std::vector<int> rows, cols;
    for (int r = 1; r < H - 1; ++r)
        for (int c = 1; c < W - 1; ++c)
            if ((r + 2 * c) % 5 == 0) { rows.push_back(r); cols.push_back(c); }
    const size_t n = rows.size();
    CHECK(n == 3729);
    const std::vector<int32_t> lattice = targets_of(rows, cols, H, W);
    CHECK(distinct_by_set(lattice, n, 0, (int32_t)n) == 18645);
    // counted exactly below the limit, and one past it at most
    CHECK(mr_host::count_distinct_targets(lattice.data(), n, 5, 0, (int32_t)n, 1 << 20, ws) == 18645);
    CHECK(mr_host::count_distinct_targets(lattice.data(), n, 5, 0, (int32_t)n, MAX_TARGETS, ws) == MAX_TARGETS + 1);
    CHECK(mr_host::count_distinct_targets(lattice.data(), n, 5, 0, 2457, MAX_TARGETS, ws) == 12285);
    CHECK(mr_host::count_distinct_targets(lattice.data(), n, 5, 100, 2458, MAX_TARGETS, ws) == MAX_TARGETS + 1);
    CHECK(mr_host::count_distinct_targets(lattice.data(), n, 5, (int32_t)n - 7, 7, MAX_TARGETS, ws) == 35);
    CHECK(mr_host::count_distinct_targets(lattice.data(), n, 5, 0, 1, 0, ws) == 1);
    // segments: 2457 points (at the limit), 1 point, the remaining 1271; then the same list as ONE segment
    {
        std::vector<int32_t> seg = { 0, 2457, 2457, 1, 2458, (int32_t)n - 2458 };
        CHECK(mr_host::mark_overlay_segments(lattice.data(), n, seg.data(), 3, LDS_POINTS, MAX_TARGETS, FLAG, ws) == 0);
        CHECK(seg[1] == 2457 && seg[3] == 1 && seg[5] == (int32_t)n - 2458);
        std::vector<int32_t> one = { 0, (int32_t)n };
        CHECK(mr_host::mark_overlay_segments(lattice.data(), n, one.data(), 1, LDS_POINTS, MAX_TARGETS, FLAG, ws) == 1);
        CHECK(one[1] == ((int32_t)n | FLAG) && one[0] == 0);
        std::vector<int32_t> two = { 0, 2458, 2458, (int32_t)n - 2458 };
        CHECK(mr_host::mark_overlay_segments(lattice.data(), n, two.data(), 2, LDS_POINTS, MAX_TARGETS, FLAG, ws) == 1);
        CHECK(two[1] == (2458 | FLAG) && two[3] == (int32_t)n - 2458);
    }

    // all duplicates: 32768, 4096 and 2458 points on one corner pixel (its own row and column neighbour): three targets
    {
        const size_t m = 32768 + 4096 + 2458;
        std::vector<int> r(m, 0), c(m, 0);
        const std::vector<int32_t> dup = targets_of(r, c, H, W);
        CHECK(mr_host::count_distinct_targets(dup.data(), m, 5, 0, 32768, MAX_TARGETS, ws) == 3);
        CHECK(mr_host::count_distinct_targets(dup.data(), m, 5, 0, (int32_t)m, 1, ws) == 2);
        std::vector<int32_t> seg = { 0, 32768, 32768, 4096, 32768 + 4096, 2458 };
        CHECK(mr_host::mark_overlay_segments(dup.data(), m, seg.data(), 3, LDS_POINTS, MAX_TARGETS, FLAG, ws) == 0);
        CHECK(seg[1] == 32768 && seg[3] == 4096 && seg[5] == 2458);
    }

    // the largest pixel index of a 32767 x 32767 frame hashes like any other
    {
        const int32_t big = 32767 * 32767 - 1;
        std::vector<int32_t> t(5 * 3000);
        for (size_t i = 0; i < t.size(); ++i) t[i] = big - (int32_t)(i % 13000);
        CHECK(mr_host::count_distinct_targets(t.data(), 3000, 5, 0, 3000, MAX_TARGETS, ws) == MAX_TARGETS + 1);
        CHECK(mr_host::count_distinct_targets(t.data(), 3000, 5, 0, 2000, MAX_TARGETS, ws) == 9000);     // (the fifth row wraps into the first)
    }

    // an empty list, and an empty segment
    {
        CHECK(mr_host::mark_overlay_segments(nullptr, 0, nullptr, 0, LDS_POINTS, MAX_TARGETS, FLAG, ws) == 0);
        CHECK(mr_host::count_distinct_targets(nullptr, 0, 5, 0, 0, MAX_TARGETS, ws) == 0);
        CHECK(mr_host::count_distinct_targets(lattice.data(), n, 5, 10, 0, MAX_TARGETS, ws) == 0);
    }

    if (failures) { std::printf("host_overlay_check: %d check(s) failed\n", failures); return 1; }
    std::printf("host_overlay_check: ok\n");
    return 0;
}
