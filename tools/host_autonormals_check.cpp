// host_autonormals_check.cpp -- the builder of the sliced per-normal face lists and their walk
// (csrc/host_autonormals.h: check_faces, build_lists, walk_lists) against a naive per-normal loop, under the
// sanitizers, on the CPU: plain C++, no HIP runtime.
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I py-numpy-renderer_amd/csrc tools/host_autonormals_check.cpp -o /tmp/host_autonormals_check && /tmp/host_autonormals_check
//
// Exit status 0 and "host_autonormals_check: ok" when every list and every normal is the expected one and the
// sanitizers saw nothing.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "host_autonormals.h"

namespace {

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Mesh {
    int32_t n_verts = 0, n_normals = 0, normal_off = 0;      // (normal_off: the rows' normal columns as a scene holds them, made global)
    std::vector<double> verts;
    std::vector<int32_t> rows;                               // 12 per face
    std::vector<float> normals;
    int32_t faces() const { return (int32_t)(rows.size() / 12); }
    void face(int32_t a, int32_t b, int32_t c, int32_t qa, int32_t qb, int32_t qc)
    {
        const int32_t row[12] = { a, 7, qa + normal_off, 3, b, 8, qb + normal_off, 3, c, 9, qc + normal_off, 3 };    // (uv and material columns: never read)
        rows.insert(rows.end(), row, row + 12);
    }
};

Mesh cloud(int32_t n_verts, int32_t n_normals, std::mt19937_64 &rng)
{
    Mesh m;
    m.n_verts = n_verts; m.n_normals = n_normals;
    std::uniform_real_distribution<double> d(-1.0, 1.0);
    m.verts.resize((size_t)n_verts * 4);
    for (double &x : m.verts) x = d(rng);
    m.normals.resize((size_t)n_normals * 3);
    for (float &x : m.normals) x = (float)d(rng);
    return m;
}

// the contract, normal by normal: every face in ascending order, asked whether a corner names the normal
int32_t naive(const Mesh &m, std::vector<float> &out)
{
    int32_t kept = 0;
    out = m.normals;
    for (int32_t q = 0; q < m.n_normals; ++q) {
        double acc[3] = { 0, 0, 0 };
        bool any = false;
        for (int32_t f = 0; f < m.faces(); ++f) {
            const int32_t *c = &m.rows[(size_t)f * 12];
            if (c[2] - m.normal_off != q && c[6] - m.normal_off != q && c[10] - m.normal_off != q) continue;
            const double *a = &m.verts[(size_t)c[0] * 4], *b = &m.verts[(size_t)c[4] * 4], *d = &m.verts[(size_t)c[8] * 4];
            const double e0[3] = { b[0] - a[0], b[1] - a[1], b[2] - a[2] }, e1[3] = { d[0] - a[0], d[1] - a[1], d[2] - a[2] };
            const double cr[3] = { e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0] };
            for (int j = 0; j < 3; ++j) acc[j] = any ? acc[j] + cr[j] : cr[j];
            any = true;
        }
        const double l = std::sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]);
        if (!any || l == 0 || !std::isfinite(acc[0]) || !std::isfinite(acc[1]) || !std::isfinite(acc[2]) || !std::isfinite(l)) { ++kept; continue; }
        for (int j = 0; j < 3; ++j) out[(size_t)q * 3 + j] = (float)(acc[j] / l);
    }
    return kept;
}

void check(const Mesh &m, const char *what)
{
    CHECK(m.normal_off != 0 || mr_autonormals::check_faces(m.rows.data(), m.faces(), m.n_verts, m.n_normals) == nullptr);
    mr_autonormals::Lists lists;
    CHECK(mr_autonormals::build_lists(m.n_normals, m.normal_off, m.rows.data(), 0, m.faces(), lists));
    const int32_t n_slices = (m.n_normals + mr_autonormals::SLICE - 1) / mr_autonormals::SLICE;
    CHECK(lists.n == m.n_normals && lists.slices() == n_slices && lists.slice_first[0] == 0);
    CHECK((size_t)lists.entries() == lists.face.size());
    // every slice as long as its longest list; every list ascending, without a face twice, closed by padding; every
    // (face, distinct normal) pair of the table once
    std::vector<int32_t> named((size_t)m.n_normals, 0);
    size_t pairs = 0;
    for (int32_t f = 0; f < m.faces(); ++f) {
        int32_t q[3];
        const int n = mr_autonormals::distinct_normals(&m.rows[(size_t)f * 12], m.normal_off, q);
        CHECK(n >= 1 && n <= 3);
        for (int k = 0; k < n; ++k) named[q[k]] += 1;
        pairs += (size_t)n;
    }
    size_t real = 0;
    for (int32_t s = 0; s < n_slices; ++s) {
        const int32_t span = lists.slice_first[s + 1] - lists.slice_first[s], len = span / mr_autonormals::SLICE;
        CHECK(span >= 0 && span % mr_autonormals::SLICE == 0);
        int32_t longest = 0;
        for (int lane = 0; lane < mr_autonormals::SLICE; ++lane) {
            const int32_t q = s * mr_autonormals::SLICE + lane;
            int32_t last = -1, count = 0;
            bool closed = false;
            for (int32_t e = 0; e < len; ++e) {
                const int32_t f = lists.face[(size_t)lists.slice_first[s] + (size_t)e * mr_autonormals::SLICE + lane];
                if (f < 0) { CHECK(f == -1); closed = true; continue; }
                CHECK(!closed && f > last && f < m.faces() && q < m.n_normals);
                if (f < m.faces() && q < m.n_normals) {
                    const int32_t *c = &m.rows[(size_t)f * 12];
                    CHECK(c[2] - m.normal_off == q || c[6] - m.normal_off == q || c[10] - m.normal_off == q);
                }
                last = f;
                ++count;
            }
            CHECK(count == (q < m.n_normals ? named[q] : 0));
            longest = count > longest ? count : longest;
            real += (size_t)count;
        }
        CHECK(longest == len);
    }
    CHECK(real == pairs);
    std::vector<float> want, got((size_t)m.n_normals * 3, -7.f);
    const int32_t kept = naive(m, want);
    CHECK(mr_autonormals::walk_lists(lists, m.verts.data(), m.rows.data(), m.normals.data(), got.data()) == kept);
    CHECK(std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0);
    std::vector<float> in_place = m.normals;
    CHECK(mr_autonormals::walk_lists(lists, m.verts.data(), m.rows.data(), in_place.data(), in_place.data()) == kept);
    CHECK(std::memcmp(in_place.data(), want.data(), got.size() * sizeof(float)) == 0);
    std::printf("  %-10s normals %5d faces %5d entries %7d (%zu listed, %d kept)\n", what, m.n_normals, m.faces(), lists.entries(), real, kept);
}

}  // namespace

int main()
{
    std::mt19937_64 rng(4321);
    // the slice seams: a strip whose face i names the normals i, i + 1 and a hub in the middle of the model -- so 0, 63,
    // 64 and the last normal are named by one or two faces and the hub by all of them --, a face that names one normal
    // with two corners, a triangle with both windings (a sum of exactly zero), and one normal nothing names
    for (int32_t n : { 1, 63, 64, 65, 130, 1000 }) {
        Mesh m = cloud(n + 8, n, rng);
        const int32_t hub = n / 2, spare = n > 8 ? n - 2 : -1, cancel = n > 8 ? n - 5 : -1;
        for (int32_t i = 0; i + 1 < n; ++i) {
            if (i == spare || i + 1 == spare || i == cancel || i + 1 == cancel) continue;
            m.face(i, i + 1, n + 7, i, i + 1, hub);
        }
        m.face(n, n + 1, n + 2, 0, 0, n - 1);
        if (cancel >= 0) {
            m.face(n + 3, n + 4, n + 5, cancel, cancel, cancel);
            m.face(n + 3, n + 5, n + 4, cancel, cancel, cancel);
        }
        check(m, "seams");
        if (n == 1) { Mesh none = cloud(3, 1, rng); check(none, "no faces"); }
    }
    // seeded random meshes: scrambled face order, hubs, unreferenced normals, normal columns offset as in a scene
    for (int round = 0; round < 24; ++round) {
        const int32_t n_normals = 1 + (int32_t)(rng() % 700), n_verts = 3 + (int32_t)(rng() % 500);
        Mesh m = cloud(n_verts, n_normals, rng);
        m.normal_off = round % 3 == 0 ? 0 : (int32_t)(rng() % 5000);
        const int32_t n_faces = (int32_t)(rng() % 2500), hubs = 1 + (int32_t)(rng() % 3);
        const int32_t reach = 1 + (int32_t)(rng() % (uint64_t)n_normals);          // normals past `reach` are named by nothing
        std::vector<int32_t> hub((size_t)hubs);
        for (int32_t &h : hub) h = (int32_t)(rng() % (uint64_t)reach);
        for (int32_t f = 0; f < n_faces; ++f) {
            int32_t q[3], v[3];
            for (int k = 0; k < 3; ++k) {
                v[k] = (int32_t)(rng() % (uint64_t)n_verts);
                q[k] = rng() % 4 == 0 ? hub[rng() % (uint64_t)hubs] : (int32_t)(rng() % (uint64_t)reach);
            }
            if (rng() % 7 == 0) q[1] = q[0];
            m.face(v[0], v[1], v[2], q[0], q[1], q[2]);
        }
        check(m, "random");
    }
    // what check_faces refuses
    {
        const int32_t good[12] = { 0, 0, 1, 0, 1, 0, 0, 0, 2, 0, 1, 0 };
        int32_t bad[12];
        CHECK(mr_autonormals::check_faces(good, 1, 3, 2) == nullptr);
        CHECK(mr_autonormals::check_faces(good, 1, 2, 2) != nullptr);
        CHECK(mr_autonormals::check_faces(good, 1, 3, 1) != nullptr);
        std::memcpy(bad, good, sizeof bad); bad[4] = -1;
        CHECK(mr_autonormals::check_faces(bad, 1, 3, 2) != nullptr);
        std::memcpy(bad, good, sizeof bad); bad[10] = -1;
        CHECK(mr_autonormals::check_faces(bad, 1, 3, 2) != nullptr);
        CHECK(mr_autonormals::check_faces(nullptr, 1, 3, 2) != nullptr);
        CHECK(mr_autonormals::check_faces(nullptr, 0, 3, 2) == nullptr);
        CHECK(mr_autonormals::check_faces(good, -1, 3, 2) != nullptr);
        CHECK(mr_autonormals::check_faces(good, 1, 0, 2) != nullptr);
        CHECK(mr_autonormals::check_faces(good, 1, 3, 0) != nullptr);
    }
    if (failures) { std::printf("host_autonormals_check: %d FAILED\n", failures); return 1; }
    std::printf("host_autonormals_check: ok\n");
    return 0;
}
