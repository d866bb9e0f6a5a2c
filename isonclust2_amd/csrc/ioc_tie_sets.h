// ioc_tie_sets.h — the tie sets of the sahlin driver (run_pipeline, ioc_host.cpp) in flat arrays.
//
// After every resolve the driver holds, per query that reaches the alignment fallback, the candidates tied at its top Size: the
// set its verdict was derived from (kept across rounds), the set of the current round, and the candidates of that set whose
// alignment passed.  They used to be one std::vector per query and round — some 1 600 allocations per round, twice a step.
// Here a collection of sets is one arena of keys and an (offset, count) per slot.
//
// Host code only (no HIP header): tools/tie_sets_check.cpp drives it under the sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

struct TieSets {
    std::vector<uint32_t> keys;  // the arena
    std::vector<size_t> off;     // per slot: where its keys start ...
    std::vector<uint32_t> cnt;   // ... and how many there are

    size_t slots() const { return cnt.size(); }
    // `n_slots` empty sets (a collection indexed by query), or none (a round's list, filled with push)
    void reset(size_t n_slots = 0)
    {
        keys.clear();
        off.assign(n_slots, 0);
        cnt.assign(n_slots, 0);
    }
    const uint32_t* begin(size_t slot) const { return keys.data() + off[slot]; }
    const uint32_t* end(size_t slot) const { return keys.data() + off[slot] + cnt[slot]; }
    uint32_t size(size_t slot) const { return cnt[slot]; }
    bool equals(size_t slot, const uint32_t* k, uint32_t n) const
    {
        if (cnt[slot] != n) return false;
        const uint32_t* mine = begin(slot);
        for (uint32_t x = 0; x < n; ++x)
            if (mine[x] != k[x]) return false;
        return true;
    }
    // a new slot at the end, holding k[0 .. n); returns its index.  k must not point into this arena (it may move).
    size_t push(const uint32_t* k, uint32_t n)
    {
        off.push_back(keys.size());
        cnt.push_back(n);
        keys.insert(keys.end(), k, k + n);
        return cnt.size() - 1;
    }
    // slot's set becomes k[0 .. n): in place when it is no larger than the set it replaces, at the end of the arena otherwise (the
    // old keys stay behind as dead space: a query's set changes a handful of times per call).  k must not point into this arena.
    void set(size_t slot, const uint32_t* k, uint32_t n)
    {
        if (n > cnt[slot]) {
            off[slot] = keys.size();
            keys.insert(keys.end(), k, k + n);
        } else {
            for (uint32_t x = 0; x < n; ++x) keys[off[slot] + x] = k[x];
        }
        cnt[slot] = n;
    }
};
