// host_autonormals.h -- vertex normals rebuilt from the deformed mesh (Model.auto_normals) on the host: the check of a
// face table, the builder of the per-normal face lists the device walks, and the walk itself (mr_host_auto_normals).
// Plain C++, no HIP: it compiles alone (tools/host_autonormals_check.cpp), and the library's upload path and its host
// helper share this one builder.
//
// A face row is the library's: 12 int32, corner k at [4 k .. 4 k + 3] = vertex, uv, normal, material.  L(q), the list of
// normal q, holds every face that has at least one corner whose normal column is q, once, in ascending face order: the
// contract is a sum of area-weighted face normals in that order.  The lists are stored sliced, as the morph lists are
// (host_morph.h): a slice is 64 consecutive normals of the model (one wavefront) and as long as its longest list; entry
// e of lane l sits at first_entry(slice) + e * 64 + l, one int32 per entry (the face; -1 marks padding, skipped).  A
// load of the walk is then one contiguous 256-byte access, the trip count is uniform over the wavefront, and a hub
// normal (the centre of a fan) stalls its own slice only.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mr_autonormals {

constexpr int SLICE = 64;

struct Lists {
    int32_t n = 0;                           // normals of the model
    std::vector<int32_t> slice_first;        // n_slices + 1: the first entry of every slice, a multiple of SLICE
    std::vector<int32_t> face;               // per entry: the face (as the caller's rows count them), -1 for padding
    int32_t slices() const { return (int32_t)slice_first.size() - 1; }
    int32_t entries() const { return slice_first.empty() ? 0 : slice_first.back(); }
    void clear() { n = 0; slice_first.clear(); face.clear(); }
};

// What the walk trusts: every vertex column inside [0, n_verts), every normal column inside [0, n_normals).  nullptr, or
// what is wrong.
inline const char *check_faces(const int32_t *faces12, int32_t n_faces, int32_t n_verts, int32_t n_normals)
{
    if (n_faces < 0 || n_verts <= 0 || n_normals <= 0 || (n_faces > 0 && !faces12)) return "auto normals need vertices, normals and faces";
    for (int64_t i = 0; i < (int64_t)n_faces * 3; ++i) {
        const int32_t *c = faces12 + i * 4;
        if (c[0] < 0 || c[0] >= n_verts) return "vertex index out of range";
        if (c[2] < 0 || c[2] >= n_normals) return "normal index out of range";
    }
    return nullptr;
}

// the corners of face row c that name a normal no earlier corner of the row names: a face enters a list once
inline int distinct_normals(const int32_t *c, int32_t normal_off, int32_t q[3])
{
    int n = 0;
    for (int k = 0; k < 3; ++k) {
        const int32_t v = c[k * 4 + 2] - normal_off;
        bool seen = false;
        for (int j = 0; j < n; ++j) seen = seen || q[j] == v;
        if (!seen) q[n++] = v;
    }
    return n;
}

// The lists of the faces [f0, f1) of a checked table, by counting sort: count the faces of every normal, size every
// slice by its longest list, then deal the faces out in ascending order, so that every list is in ascending face order.
// The normal columns of these rows lie in [normal_off, normal_off + n_normals); the lists name the faces by their row.
// False when the padded lists do not fit 32-bit offsets.
inline bool build_lists(int32_t n_normals, int32_t normal_off, const int32_t *faces12, int32_t f0, int32_t f1, Lists &out)
{
    out.clear();
    out.n = n_normals;
    const int32_t n_slices = (n_normals + SLICE - 1) / SLICE;
    std::vector<int32_t> fill((size_t)n_normals, 0);
    int32_t q[3];
    for (int32_t f = f0; f < f1; ++f) {
        const int n = distinct_normals(faces12 + (size_t)f * 12, normal_off, q);
        for (int k = 0; k < n; ++k) fill[q[k]] += 1;
    }
    out.slice_first.assign((size_t)n_slices + 1, 0);
    int64_t total = 0;
    for (int32_t s = 0; s < n_slices; ++s) {
        int32_t longest = 0;
        for (int32_t v = s * SLICE; v < n_normals && v < (s + 1) * SLICE; ++v) longest = fill[v] > longest ? fill[v] : longest;
        total += (int64_t)longest * SLICE;
        if (total > INT32_MAX) { out.clear(); return false; }
        out.slice_first[(size_t)s + 1] = (int32_t)total;
    }
    out.face.assign((size_t)total, -1);
    std::fill(fill.begin(), fill.end(), 0);
    for (int32_t f = f0; f < f1; ++f) {
        const int n = distinct_normals(faces12 + (size_t)f * 12, normal_off, q);
        for (int k = 0; k < n; ++k) {
            const int32_t v = q[k];
            out.face[(size_t)out.slice_first[v / SLICE] + (size_t)fill[v]++ * SLICE + (size_t)(v % SLICE)] = f;
        }
    }
    return true;
}

// The walk, in the kernel's order: normal q sums the cross products (b - a) x (c - a) of the faces of its list --
// a, b, c the vertices of corners 0, 1, 2, rows of 4 doubles; every operation rounded on its own, the first product
// taken as it is, not added to a zero -- and is float32(acc / |acc|); the authored normal stays for an empty list, a
// sum of length 0 and a sum or a length that is not finite.  normals_in and out are (n, 3) float32 and may be one
// array.  Returns how many normals kept their authored value.
inline int32_t walk_lists(const Lists &lists, const double *verts, const int32_t *faces12, const float *normals_in, float *out)
{
    int32_t kept = 0;
    for (int32_t i = 0; i < lists.n; ++i) {
        const int32_t s = i / SLICE, lane = i % SLICE;
        double acc[3] = { 0, 0, 0 };
        bool any = false;
        for (int32_t p = lists.slice_first[s]; p < lists.slice_first[(size_t)s + 1]; p += SLICE) {
            const int32_t f = lists.face[(size_t)p + lane];
            if (f < 0) continue;
            const int32_t *c = faces12 + (size_t)f * 12;
            const double *a = verts + (size_t)c[0] * 4, *b = verts + (size_t)c[4] * 4, *d = verts + (size_t)c[8] * 4;
            const double e0[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, e1[3] = { d[0] - a[0], d[1] - a[1], d[2] - a[2] };
            const double p0 = e0[1] * e1[2], p1 = e0[2] * e1[1], p2 = e0[2] * e1[0], p3 = e0[0] * e1[2], p4 = e0[0] * e1[1], p5 = e0[1] * e1[0];
            const double cr[3] = { p0 - p1, p2 - p3, p4 - p5 };
            for (int j = 0; j < 3; ++j) acc[j] = any ? acc[j] + cr[j] : cr[j];
            any = true;
        }
        const double s0 = acc[0] * acc[0], s1 = acc[1] * acc[1], s2 = acc[2] * acc[2];
        const double l = std::sqrt((s0 + s1) + s2);
        const bool keep = !any || l == 0 || !std::isfinite(acc[0]) || !std::isfinite(acc[1]) || !std::isfinite(acc[2]) || !std::isfinite(l);
        for (int j = 0; j < 3; ++j) out[(size_t)i * 3 + j] = keep ? normals_in[(size_t)i * 3 + j] : (float)(acc[j] / l);
        kept += keep ? 1 : 0;
    }
    return kept;
}

}  // namespace mr_autonormals
