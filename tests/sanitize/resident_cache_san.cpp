// tests/sanitize/resident_cache_san.cpp — csrc/resident_cache.h (the bookkeeping of the batch's keyframe store and of a node member's resident clouds)
// under AddressSanitizer + UndefinedBehaviorSanitizer, driven next to a deliberately naive model: a vector scanned linearly.  A few thousand
// pseudo-random operations per seed over at most 64 keys — insert, resize, touch, hold, release, next_era, make_room, erase, forget-all, set_cap —
// and after every one of them: the same keys, bytes and stamps as the model, every surviving entry at the address it was inserted at, and for
// make_room the rules themselves, checked from a snapshot and not from the model's loop: nothing in use went, the victims are the evictable entries of
// smallest tick, and it stopped exactly when the need fitted or nothing evictable was left.
// Exit code 0, "0 failed checks" and no sanitizer report = pass (tests/test_hardening_cpu.py builds and runs it).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "resident_cache.h"

using namespace mrgfe;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); ++fails; } } while (0)

struct Fake {
    size_t b = 0;
    int*   owned = new int(7);  // (a leak or a double free of an entry shows under the sanitizer)
    Fake() = default;
    Fake(const Fake&) = delete;
    Fake& operator=(const Fake&) = delete;
    ~Fake() { delete owned; }
    size_t bytes() const { return b; }
};
using Cache = ResidentCache<uint64_t, Fake>;
typedef unsigned __int128 wide;  // bytes + need without wrap-around

struct ModelEntry {
    uint64_t key, era, tick;
    size_t   bytes;
    bool     held;
    const Cache::Entry* at;
};
struct Model {
    std::vector<ModelEntry> v;
    uint64_t era = 1, tick = 0;
    size_t   cap = ~size_t(0);
    ModelEntry* find(uint64_t key) { for (auto& e : v) if (e.key == key) return &e; return nullptr; }
    bool   in_use(const ModelEntry& e) const { return e.era == era || e.held; }
    size_t bytes() const { size_t t = 0; for (auto& e : v) t += e.bytes; return t; }
    void   erase(uint64_t key) { v.erase(std::remove_if(v.begin(), v.end(), [&](const ModelEntry& e) { return e.key == key; }), v.end()); }
    void   make_room(size_t need)
    {
        for (;;) {
            if (wide(bytes()) + need <= cap) return;
            int victim = -1;
            for (size_t i = 0; i < v.size(); ++i)
                if (!in_use(v[i]) && (victim < 0 || v[i].tick < v[size_t(victim)].tick)) victim = int(i);
            if (victim < 0) return;
            v.erase(v.begin() + victim);
        }
    }
};

static void same(const Cache& c, Model& m)
{
    size_t n = 0;
    for (auto& kv : c) {
        ++n;
        const ModelEntry* e = m.find(kv.first);
        CHECK(e != nullptr);
        if (!e) continue;
        CHECK(&kv.second == e->at);  // pointer stability: where it was inserted
        CHECK(kv.second.data.bytes() == e->bytes && kv.second.era == e->era && kv.second.tick == e->tick && kv.second.held == e->held);
        CHECK(c.in_use(kv.second) == m.in_use(*e) && c.named(kv.second) == (e->era == m.era));
        CHECK(c.find(kv.first) == &kv.second);
    }
    CHECK(n == m.v.size());
    CHECK(c.bytes() == m.bytes());
    CHECK(c.cap() == m.cap);
}

// make_room against the rules, from a snapshot `before` of the model
static void check_make_room(const Cache& c, const Model& before, size_t need)
{
    std::vector<ModelEntry> evictable;
    size_t kept_bytes = 0;
    for (auto& e : before.v) {
        if (before.in_use(e)) { CHECK(c.find(e.key) == e.at); kept_bytes += e.bytes; }  // nothing in use is erased
        else evictable.push_back(e);
    }
    std::sort(evictable.begin(), evictable.end(), [](const ModelEntry& a, const ModelEntry& b) { return a.tick < b.tick; });
    size_t gone = 0;
    while (gone < evictable.size() && !c.find(evictable[gone].key)) ++gone;
    for (size_t i = gone; i < evictable.size(); ++i) CHECK(c.find(evictable[i].key) == evictable[i].at);  // the victims are the `gone` smallest ticks
    wide after = kept_bytes;
    for (size_t i = gone; i < evictable.size(); ++i) after += evictable[i].bytes;
    CHECK(after == c.bytes());
    CHECK(after + need <= before.cap || gone == evictable.size());               // it went on as long as it had to and could ...
    if (gone) CHECK(after + evictable[gone - 1].bytes + need > before.cap);      // ... and no further
}

static void run(unsigned seed, int n_ops, int n_keys)
{
    std::mt19937 rng(seed);
    auto pick = [&](unsigned n) { return unsigned(rng() % n); };
    const size_t sizes[] = {0, 0, 1, 16, 100, 4096, 20000 * 16, 20000 * 64, size_t(3) << 20};
    const size_t caps[] = {0, 1, 4096, size_t(1) << 20, size_t(8) << 20, size_t(64) << 20, ~size_t(0)};
    Cache c;
    Model m;
    CHECK(c.cap() == ~size_t(0));
    c.make_room(123);  // (an empty cache)
    same(c, m);
    c.set_cap(m.cap = size_t(1) << 20);
    for (int op = 0; op < n_ops; ++op) {
        const uint64_t key = 1 + pick(unsigned(n_keys));
        const unsigned what = pick(100);
        Cache::Entry* e = c.find(key);
        ModelEntry*   me = m.find(key);
        CHECK((e != nullptr) == (me != nullptr));
        if (what < 30) {  // insert; an entry that is there is found, and grows or shrinks (covariances arrive after the cloud)
            Cache::Entry* got = c.find_or_insert(key);
            CHECK(got != nullptr && (!e || got == e));
            if (!got) continue;
            if (!me) {
                CHECK(got->era == 0 && !got->held && !c.in_use(*got));
                m.v.push_back(ModelEntry{key, 0, ++m.tick, 0, false, got});
                me = &m.v.back();
            }
            got->data.b = me->bytes = sizes[pick(sizeof(sizes) / sizeof(sizes[0]))];
        } else if (what < 50) {
            if (e) { c.touch(*e); me->era = m.era; me->tick = ++m.tick; }
        } else if (what < 58) {
            if (e) e->held = me->held = true;
        } else if (what < 64) {
            if (e) e->held = me->held = false;
        } else if (what < 72) {
            c.next_era();
            ++m.era;
        } else if (what < 90) {
            const size_t pool[] = {0, 1, 20000 * 16, m.cap, m.cap / 2, m.cap + 1, ~size_t(0), sizes[pick(9)]};  // (larger than the cap, and wrapping, included)
            const size_t need = pool[pick(8)];
            const Model  before = m;
            c.make_room(need);
            m.make_room(need);
            check_make_room(c, before, need);
        } else if (what < 95) {
            c.erase(key);
            m.erase(key);
            CHECK(c.find(key) == nullptr);
        } else if (what < 96) {
            c.clear();
            m.v.clear();
        } else if (what < 98) {
            c.clear_held();
            for (auto& x : m.v) x.held = false;
        } else {
            c.set_cap(m.cap = caps[pick(sizeof(caps) / sizeof(caps[0]))]);
        }
        same(c, m);
    }
}

// the rules once more on a case small enough to read: cap 100, three entries of 40 bytes
static void by_hand()
{
    Cache c;
    c.set_cap(100);
    Cache::Entry *a = c.find_or_insert(1), *b = c.find_or_insert(2);
    a->data.b = b->data.b = 40;
    c.touch(*b);
    c.touch(*a);  // a is the more recently used
    c.next_era();
    c.make_room(40);  // 80 + 40 > 100: b goes, a stays
    CHECK(c.find(1) == a && !c.find(2) && c.bytes() == 40);
    Cache::Entry* d = c.find_or_insert(3);
    d->data.b = 40;
    c.touch(*d);
    c.touch(*a);
    c.make_room(1000);  // more than the cap, and both are named by this era: the working set stays
    CHECK(c.find(1) == a && c.find(3) == d && c.bytes() == 80);
    a->held = true;
    c.next_era();
    c.set_cap(0);
    c.make_room(0);  // cap 0: what is not in use goes, the held entry stays
    CHECK(c.find(1) == a && !c.find(3));
    c.clear_held();
    c.make_room(0);
    CHECK(!c.find(1) && c.bytes() == 0);
    Cache::Entry* z = c.find_or_insert(4);  // zero bytes fit under cap 0: not evicted
    c.make_room(0);
    CHECK(c.find(4) == z);
}

static void cap_from_env()
{
    unsetenv("MRGFE_KEYFRAME_STORE_MB");
    CHECK(Cache::cap_from_env(size_t(16) << 30) == size_t(16) << 30);
    const struct { const char* text; size_t want; } cases[] = {{"1", size_t(1) << 20}, {"16384", size_t(16) << 30}, {"2.9", size_t(2) << 20}, {"0.5", 0}, {"0", 0}, {"-5", 0}, {"junk", 0}};
    for (auto& k : cases) {
        setenv("MRGFE_KEYFRAME_STORE_MB", k.text, 1);
        CHECK(Cache::cap_from_env(77) == k.want);
    }
    unsetenv("MRGFE_KEYFRAME_STORE_MB");
}

int main()
{
    by_hand();
    cap_from_env();
    for (unsigned seed : {1u, 2u, 3u}) run(seed, 3000, 64);
    run(4u, 3000, 5);  // few keys: long lives, many replacements of the same entry
    std::printf("%d failed checks\n", fails);
    return fails ? 1 : 0;
}
