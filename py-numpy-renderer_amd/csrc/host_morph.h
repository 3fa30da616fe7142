// host_morph.h -- morph targets (blend shapes) on the host: the check of the caller's tables, the builder of the
// per-vertex contribution lists the device walks, and the walk itself (mr_host_morph_chain).  Plain C++, no HIP: it
// compiles alone (tools/host_morph_check.cpp), and the library's upload path and its host helper share this one builder.
//
// The caller's tables are CSR by target: target k lists the vertices index[first[k] .. first[k + 1]) and displaces
// vertex index[j] by delta[3 j .. 3 j + 2].  The kernel needs the transpose -- per vertex, the targets that list it, in
// ascending target order, because the contract is a chain of fma steps in that order -- and needs it in a shape a
// wavefront can read: the lists are stored sliced.  A slice is 64 consecutive vertices of the model (one wavefront) and
// as long as its longest list; entry e of lane l sits at first_entry(slice) + e * 64 + l in four planes, the target
// (int32, -1 marks padding: skipped, never multiplied by a weight of 0) and the three components of the delta (double).
// Every wave-instruction of the walk is then one contiguous 256- or 512-byte access, the trip count is uniform over the
// wavefront, and a long list stalls its own slice only.  No slice is longer than the number of targets, so the storage
// is bounded by the dense size.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mr_morph {

constexpr int SLICE = 64;

struct Lists {
    int32_t n = 0;                           // vertices (or normals) of the model
    std::vector<int32_t> slice_first;        // n_slices + 1: the first entry of every slice, a multiple of SLICE
    std::vector<int32_t> target;             // per entry: the target, -1 for padding
    std::vector<double> dx, dy, dz;          // per entry: the delta (0 in padding)
    int32_t slices() const { return (int32_t)slice_first.size() - 1; }
    int32_t entries() const { return slice_first.empty() ? 0 : slice_first.back(); }
    void clear() { n = 0; slice_first.clear(); target.clear(); dx.clear(); dy.clear(); dz.clear(); }
};

// What the kernels trust: offsets that start at 0 and never fall, every index inside [0, n) and named once per target
// at most, every delta finite.  nullptr, or what is wrong.
inline const char *check_tables(int32_t n, int32_t n_targets, const int32_t *first, const int32_t *index, const double *delta)
{
    if (n <= 0 || n_targets <= 0 || !first) return "a morph needs at least one target";
    if (first[0] != 0) return "morph offsets must start at 0";
    for (int32_t k = 0; k < n_targets; ++k)
        if (first[k + 1] < first[k]) return "morph offsets must not fall";
    const int32_t total = first[n_targets];
    if (total > 0 && (!index || !delta)) return "a morph needs indices and deltas";
    std::vector<int32_t> seen((size_t)n, -1);                // the last target that named the vertex
    for (int32_t k = 0; k < n_targets; ++k)
        for (int32_t j = first[k]; j < first[k + 1]; ++j) {
            const int32_t v = index[j];
            if (v < 0 || v >= n) return "morph index out of range";
            if (seen[v] == k) return "a morph target names an index twice";
            seen[v] = k;
            for (int c = 0; c < 3; ++c)
                if (!std::isfinite(delta[(size_t)j * 3 + c])) return "morph deltas must be finite";
        }
    return nullptr;
}

// The lists of one checked table, by counting sort: count the targets of every vertex, size every slice by its longest
// list, then deal the targets out in ascending order, so that every list is in ascending target order.  False when the
// padded lists do not fit 32-bit offsets.
inline bool build_lists(int32_t n, int32_t n_targets, const int32_t *first, const int32_t *index, const double *delta, Lists &out)
{
    out.clear();
    out.n = n;
    const int32_t n_slices = (n + SLICE - 1) / SLICE;
    std::vector<int32_t> fill((size_t)n, 0);
    for (int32_t j = 0; j < first[n_targets]; ++j) fill[index[j]] += 1;
    out.slice_first.assign((size_t)n_slices + 1, 0);
    int64_t total = 0;
    for (int32_t s = 0; s < n_slices; ++s) {
        int32_t longest = 0;
        for (int32_t v = s * SLICE; v < n && v < (s + 1) * SLICE; ++v) longest = fill[v] > longest ? fill[v] : longest;
        total += (int64_t)longest * SLICE;
        if (total > INT32_MAX) { out.clear(); return false; }
        out.slice_first[(size_t)s + 1] = (int32_t)total;
    }
    out.target.assign((size_t)total, -1);
    out.dx.assign((size_t)total, 0.0); out.dy.assign((size_t)total, 0.0); out.dz.assign((size_t)total, 0.0);
    std::fill(fill.begin(), fill.end(), 0);
    for (int32_t k = 0; k < n_targets; ++k)
        for (int32_t j = first[k]; j < first[k + 1]; ++j) {
            const int32_t v = index[j];
            const size_t at = (size_t)out.slice_first[v / SLICE] + (size_t)fill[v]++ * SLICE + (size_t)(v % SLICE);
            out.target[at] = k;
            out.dx[at] = delta[(size_t)j * 3]; out.dy[at] = delta[(size_t)j * 3 + 1]; out.dz[at] = delta[(size_t)j * 3 + 2];
        }
    return true;
}

// The walk, in the kernel's order: vertex i starts from base[i] (width 4: x y z w, w passes through; width 3: a widened
// normal) and takes one fma step per entry of its list, padding skipped.  out may be base.
inline void walk_lists(const Lists &lists, const double *base, int32_t width, const double *w, double *out)
{
    for (int32_t i = 0; i < lists.n; ++i) {
        const int32_t s = i / SLICE, lane = i % SLICE;
        double x = base[(size_t)i * width], y = base[(size_t)i * width + 1], z = base[(size_t)i * width + 2];
        for (int32_t p = lists.slice_first[s]; p < lists.slice_first[(size_t)s + 1]; p += SLICE) {
            const int32_t t = lists.target[(size_t)p + lane];
            if (t < 0) continue;
            x = std::fma(w[t], lists.dx[(size_t)p + lane], x);
            y = std::fma(w[t], lists.dy[(size_t)p + lane], y);
            z = std::fma(w[t], lists.dz[(size_t)p + lane], z);
        }
        out[(size_t)i * width] = x; out[(size_t)i * width + 1] = y; out[(size_t)i * width + 2] = z;
        if (width == 4) out[(size_t)i * 4 + 3] = base[(size_t)i * 4 + 3];
    }
}

}  // namespace mr_morph
