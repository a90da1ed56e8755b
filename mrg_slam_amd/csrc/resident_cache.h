// csrc/resident_cache.h — ResidentCache: payloads kept resident under a key and a byte budget, least recently used out first.  The ONE bookkeeping
// behind the batch's keyframe store (batch.cpp) and a node member's keyed targets and map-store replicas (node.cpp); each owner has a cache, and so a
// budget, of its own.  Plain C++17 on purpose: no HIP, nothing of common.h, so tests/sanitize/resident_cache_san.cpp drives it on the host.
//   * An entry is IN USE when the current work named it (touch() since the last next_era()) or it is `held`; an entry in use is never evicted, and the
//     owner does not replace or erase one either.
//   * make_room(need) evicts entries not in use, smallest tick first, only until bytes() + need <= cap() — or nothing evictable is left: the working
//     set of one call may exceed the cap.  Ticks are unique (insertion stamps one, touch() a newer one), so the victim never depends on container order.
//   * Every entry is a map node, allocated on its own: an Entry* / Payload* stays good until THAT entry is erased, whatever else is inserted or evicted.
// No locking inside.  The caller holds the owning context's lock (a node member: its thread, or the node's api lock) and has the context's device
// bound wherever an entry can be freed — erase(), clear(), make_room() — since a payload frees its device memory in its destructor.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <new>

namespace mrgfe {

template <class Key, class Payload>  // Key: operator<;  Payload: default-constructible, size_t bytes() const
class ResidentCache {
   public:
    // era: that of the last touch() (0: never named); tick: insertion or the last touch(), whichever is later — the LRU order
    struct Entry { Payload data; uint64_t era = 0, tick = 0; bool held = false; };
    using Map = std::map<Key, Entry>;
    Entry* find(const Key& key) { auto it = map_.find(key); return it == map_.end() ? nullptr : &it->second; }
    const Entry* find(const Key& key) const { auto it = map_.find(key); return it == map_.end() ? nullptr : &it->second; }
    Entry* find_or_insert(const Key& key)  // default-constructed, and named by nobody, when it was not there; null: out of host memory
    {
        try {
            auto at = map_.try_emplace(key);
            if (at.second) at.first->second.tick = ++tick_;
            return &at.first->second;
        } catch (const std::bad_alloc&) { return nullptr; }
    }
    void touch(Entry& e) { e.era = era_; e.tick = ++tick_; }
    void next_era() { ++era_; }  // nothing is named by the current work any more; `held` stays
    bool named(const Entry& e) const { return e.era == era_; }
    bool in_use(const Entry& e) const { return named(e) || e.held; }
    void make_room(size_t need)
    {
        size_t total = bytes();
        while (need > cap_ || total > cap_ - need) {
            auto victim = map_.end();
            for (auto it = map_.begin(); it != map_.end(); ++it)
                if (!in_use(it->second) && (victim == map_.end() || it->second.tick < victim->second.tick)) victim = it;
            if (victim == map_.end()) return;  // everything left is in use
            total -= victim->second.data.bytes();
            map_.erase(victim);
        }
    }
    void erase(const Key& key) { map_.erase(key); }
    void clear() { map_.clear(); }
    void clear_held() { for (auto& kv : map_) kv.second.held = false; }
    size_t bytes() const { size_t total = 0; for (auto& kv : map_) total += kv.second.data.bytes(); return total; }
    size_t cap() const { return cap_; }
    void   set_cap(size_t bytes) { cap_ = bytes; }
    typename Map::iterator begin() { return map_.begin(); }  // (key, entry) pairs in key order: `for (auto& kv : cache)`
    typename Map::iterator end() { return map_.end(); }
    typename Map::const_iterator begin() const { return map_.begin(); }
    typename Map::const_iterator end() const { return map_.end(); }

    // the budget in bytes: MRGFE_KEYFRAME_STORE_MB (MiB, negative counts as 0) when set, else `dflt` — read here and nowhere else
    static size_t cap_from_env(size_t dflt) { const char* e = std::getenv("MRGFE_KEYFRAME_STORE_MB"); return e ? static_cast<size_t>(std::max(0.0, std::atof(e))) << 20 : dflt; }

   private:
    Map      map_;
    uint64_t era_ = 1, tick_ = 0;
    size_t   cap_ = ~size_t(0);
};

}  // namespace mrgfe
