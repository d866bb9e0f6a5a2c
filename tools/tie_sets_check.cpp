// tie_sets_check.cpp — the flat tie sets of the sahlin driver (isonclust2_amd/csrc/ioc_tie_sets.h) against the container they
// replaced, a std::vector<uint32_t> per slot, driven on the CPU:
//
//  * a collection indexed by query (reset(n), set, equals, begin / end): random sequences of replacements — by a smaller set (in
//    place), by a larger one (moved to the end of the arena), by an empty one, of the last slot, of sets of 0, 1, 16 and 40 keys —
//    leave every slot equal to the model's vector, the untouched slots included;
//  * a round's list (reset(), push): slots in the order pushed, empty sets among them, begin / end of each;
//  * equals against sets that differ in length, in the first and in the last key.
//
// Host code only (the header includes no HIP header); meant for the sanitizers:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iisonclust2_amd/csrc \
//       -o /tmp/tie_sets_check tools/tie_sets_check.cpp && /tmp/tie_sets_check
//
// Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <random>
#include <vector>

#include "ioc_tie_sets.h"

namespace {

long g_checks = 0;
bool g_ok = true;
#define EXPECT(cond)                                          \
    do {                                                      \
        ++g_checks;                                           \
        if (!(cond)) {                                        \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
            g_ok = false;                                     \
        }                                                     \
    } while (0)

using Model = std::vector<std::vector<uint32_t>>;

void same(const TieSets& t, const Model& m)
{
    EXPECT(t.slots() == m.size());
    for (size_t s = 0; s < m.size() && s < t.slots(); ++s) {
        EXPECT(t.size(s) == m[s].size());
        EXPECT(t.end(s) - t.begin(s) == long(m[s].size()));
        EXPECT(std::vector<uint32_t>(t.begin(s), t.end(s)) == m[s]);
        EXPECT(t.equals(s, m[s].data(), uint32_t(m[s].size())));
    }
}

std::vector<uint32_t> draw(std::mt19937& rng, uint32_t n)
{
    std::vector<uint32_t> v(n);
    for (auto& x : v) x = uint32_t(rng());
    return v;
}

void by_query()
{
    std::mt19937 rng(71);
    const uint32_t sizes[] = {0, 1, 2, 15, 16, 17, 40};
    for (size_t n : {size_t(1), size_t(2), size_t(37), size_t(1600)}) {
        TieSets t;
        t.reset(n);
        Model m(n);
        same(t, m);
        for (int step = 0; step < 4000; ++step) {
            const size_t s = step % 7 == 0 ? n - 1 : rng() % n;
            const std::vector<uint32_t> v = draw(rng, sizes[rng() % 7]);
            t.set(s, v.data(), uint32_t(v.size()));
            m[s] = v;
            if (step % 500 == 0) same(t, m);
        }
        same(t, m);
        t.reset(n);  // (the next call's queries: every set empty again, the arena too)
        EXPECT(t.keys.empty());
        same(t, Model(n));
    }
}

void by_round()
{
    std::mt19937 rng(73);
    TieSets t;
    t.reset();
    Model m;
    same(t, m);
    for (int step = 0; step < 3000; ++step) {
        const std::vector<uint32_t> v = draw(rng, step % 5 == 0 ? 0u : uint32_t(rng() % 41));
        EXPECT(t.push(v.data(), uint32_t(v.size())) == m.size());
        m.push_back(v);
    }
    same(t, m);
    // a set of one collection into another (run_pipeline: the round's set becomes the query's)
    TieSets q;
    q.reset(m.size());
    for (size_t s = 0; s < m.size(); ++s) q.set(s, t.begin(s), t.size(s));
    same(q, m);
}

void equality()
{
    TieSets t;
    t.reset(3);
    const uint32_t a[] = {3, 5, 9, 11}, b[] = {4, 5, 9, 11}, d[] = {3, 5, 9, 12};
    t.set(1, a, 4);
    EXPECT(t.equals(1, a, 4));
    EXPECT(!t.equals(1, a, 3));
    EXPECT(!t.equals(1, b, 4));
    EXPECT(!t.equals(1, d, 4));
    EXPECT(t.equals(0, a, 0) && t.equals(2, nullptr, 0));
    EXPECT(!t.equals(0, a, 1));
}

}  // namespace

int main()
{
    by_query();
    by_round();
    equality();
    printf("%s: %ld checks\n", g_ok ? "ok" : "FAILED", g_checks);
    return g_ok ? 0 : 1;
}
