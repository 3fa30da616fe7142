// host_morph_check.cpp -- the builder of the sliced per-vertex morph lists and their walk (csrc/host_morph.h:
// check_tables, build_lists, walk_lists) against a naive per-vertex loop, under the sanitizers, on the CPU: plain C++,
// no HIP runtime.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I py-numpy-renderer_amd/csrc tools/host_morph_check.cpp -o /tmp/host_morph_check && /tmp/host_morph_check
//
// Exit status 0 and "host_morph_check: ok" when every list and every chain is the expected one and the sanitizers saw
// nothing.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "host_morph.h"

namespace {

int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Tables {
    int32_t n = 0;
    std::vector<int32_t> first{ 0 }, index;
    std::vector<double> delta;
    int32_t targets() const { return (int32_t)first.size() - 1; }
    void add(const std::vector<int32_t> &listed, std::mt19937_64 &rng)
    {
        std::uniform_real_distribution<double> d(-0.1, 0.1);
        for (int32_t v : listed) {
            index.push_back(v);
            for (int c = 0; c < 3; ++c) delta.push_back(d(rng));
        }
        first.push_back((int32_t)index.size());
    }
};

// the contract, vertex by vertex: every target in ascending order, searched for the vertex
void naive(const Tables &t, const std::vector<double> &base, int width, const std::vector<double> &w, std::vector<double> &out)
{
    out = base;
    for (int32_t i = 0; i < t.n; ++i)
        for (int32_t k = 0; k < t.targets(); ++k)
            for (int32_t j = t.first[k]; j < t.first[k + 1]; ++j)
                if (t.index[j] == i)
                    for (int c = 0; c < 3; ++c)
                        out[(size_t)i * width + c] = std::fma(w[k], t.delta[(size_t)j * 3 + c], out[(size_t)i * width + c]);
}

void check(const Tables &t, std::mt19937_64 &rng, const char *what)
{
    CHECK(mr_morph::check_tables(t.n, t.targets(), t.first.data(), t.index.data(), t.delta.data()) == nullptr);
    mr_morph::Lists lists;
    CHECK(mr_morph::build_lists(t.n, t.targets(), t.first.data(), t.index.data(), t.delta.data(), lists));
    const int32_t n_slices = (t.n + mr_morph::SLICE - 1) / mr_morph::SLICE;
    CHECK(lists.n == t.n && lists.slices() == n_slices && lists.slice_first[0] == 0);
    CHECK((size_t)lists.entries() == lists.target.size() && lists.dx.size() == lists.target.size());
    CHECK(lists.dy.size() == lists.target.size() && lists.dz.size() == lists.target.size());
    // every slice as long as its longest list, every list ascending and closed by padding, every entry of the tables once
    std::vector<int32_t> listed((size_t)t.n, 0);
    for (int32_t j = 0; j < t.first[t.targets()]; ++j) listed[t.index[j]] += 1;
    size_t real = 0;
    for (int32_t s = 0; s < n_slices; ++s) {
        const int32_t len = (lists.slice_first[s + 1] - lists.slice_first[s]) / mr_morph::SLICE;
        CHECK((lists.slice_first[s + 1] - lists.slice_first[s]) % mr_morph::SLICE == 0 && len <= t.targets());
        int32_t longest = 0;
        for (int lane = 0; lane < mr_morph::SLICE; ++lane) {
            const int32_t v = s * mr_morph::SLICE + lane;
            int32_t last = -1, count = 0;
            bool closed = false;
            for (int32_t e = 0; e < len; ++e) {
                const int32_t k = lists.target[(size_t)lists.slice_first[s] + (size_t)e * mr_morph::SLICE + lane];
                if (k < 0) { closed = true; continue; }
                CHECK(!closed && k > last && k < t.targets() && v < t.n);
                last = k;
                ++count;
            }
            CHECK(count == (v < t.n ? listed[v] : 0));
            longest = count > longest ? count : longest;
            real += (size_t)count;
        }
        CHECK(longest == len);
    }
    CHECK(real == t.index.size());
    std::uniform_real_distribution<double> d(-2.0, 2.0);
    std::vector<double> w((size_t)t.targets());
    for (double &x : w) x = d(rng);
    if (!w.empty()) w[0] = 0.0;                                    // (a weight of 0 takes its step all the same)
    for (int width : { 4, 3 }) {
        std::vector<double> base((size_t)t.n * width), want, got((size_t)t.n * width, -1.0);
        for (double &x : base) x = d(rng);
        naive(t, base, width, w, want);
        mr_morph::walk_lists(lists, base.data(), width, w.data(), got.data());
        CHECK(std::memcmp(got.data(), want.data(), got.size() * sizeof(double)) == 0);
        mr_morph::walk_lists(lists, base.data(), width, w.data(), base.data());       // in place
        CHECK(std::memcmp(base.data(), want.data(), base.size() * sizeof(double)) == 0);
    }
    std::printf("  %-28s n %5d targets %3d entries %7d (%zu listed)\n", what, t.n, t.targets(), lists.entries(), real);
}

}  // namespace

int main()
{
    std::mt19937_64 rng(12345);
    // the slice seams: 0, 63, 64, 255, 256 and the last vertex; a lone vertex in an otherwise empty slice; a hub every
    // target with entries lists, between two empty slices; a target without entries; n no multiple of 64
    for (int32_t n : { 1, 63, 64, 65, 130, 1000 }) {
        Tables t;
        t.n = n;
        const int32_t hub = n > 517 ? 517 : n / 2;
        const std::vector<std::vector<int32_t>> sets = { { 0, 63, 64, 255, 256, n - 1, hub }, {}, { 401, hub }, { 63, 64, hub }, { n - 1, 0, hub } };
        for (const auto &wanted : sets) {
            std::vector<int32_t> kept;
            for (int32_t v : wanted)
                if (v >= 0 && v < n && std::find(kept.begin(), kept.end(), v) == kept.end()) kept.push_back(v);
            t.add(kept, rng);
        }
        check(t, rng, "slices");
    }
    // seeded random tables: a few targets to a few hundred, sparse to dense, listed in scrambled order
    for (int round = 0; round < 24; ++round) {
        Tables t;
        t.n = 1 + (int32_t)(rng() % 700);
        const int32_t n_targets = 1 + (int32_t)(rng() % (round % 4 == 3 ? 300 : 12));
        const double density = (double)(rng() % 1000) / 1000.0 * (round % 2 ? 1.0 : 0.05);
        for (int32_t k = 0; k < n_targets; ++k) {
            std::vector<int32_t> listed;
            for (int32_t v = 0; v < t.n; ++v)
                if ((double)(rng() % 100000) / 100000.0 < density) listed.push_back(v);
            std::shuffle(listed.begin(), listed.end(), rng);
            t.add(listed, rng);
        }
        check(t, rng, "random");
    }
    // what check_tables refuses
    {
        const int32_t first[3] = { 0, 2, 3 }, index[3] = { 1, 0, 1 }, twice[3] = { 1, 1, 0 }, far[3] = { 1, 4, 0 }, neg[3] = { -1, 0, 1 };
        const int32_t falls[3] = { 0, 2, 1 }, late[3] = { 1, 2, 3 };
        double delta[9] = { 0 }, nan[9] = { 0 };
        nan[8] = NAN;
        CHECK(mr_morph::check_tables(4, 2, first, index, delta) == nullptr);
        CHECK(mr_morph::check_tables(4, 2, first, twice, delta) != nullptr);
        CHECK(mr_morph::check_tables(4, 2, first, far, delta) != nullptr);
        CHECK(mr_morph::check_tables(4, 2, first, neg, delta) != nullptr);
        CHECK(mr_morph::check_tables(4, 2, first, index, nan) != nullptr);
        CHECK(mr_morph::check_tables(4, 2, falls, index, delta) != nullptr);
        CHECK(mr_morph::check_tables(4, 2, late, index, delta) != nullptr);
        CHECK(mr_morph::check_tables(4, 0, first, index, delta) != nullptr);
        CHECK(mr_morph::check_tables(4, 2, nullptr, index, delta) != nullptr);
        CHECK(mr_morph::check_tables(4, 2, first, nullptr, delta) != nullptr);
        CHECK(mr_morph::check_tables(0, 2, first, index, delta) != nullptr);
    }
    if (failures) { std::printf("host_morph_check: %d FAILED\n", failures); return 1; }
    std::printf("host_morph_check: ok\n");
    return 0;
}
