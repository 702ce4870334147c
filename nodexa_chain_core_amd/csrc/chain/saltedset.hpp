// A bounded set of 32-byte keys that evicts the oldest first: what the signature cache
// (sigcache.hpp) and the script-execution cache (scriptcache.hpp) keep their entries in. The keys are
// salted SHA-256 values made by the owner, so their first bytes serve as the table hash. Not
// synchronised: the owner holds its lock around every call.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <string>
#include <unordered_map>
#include <utility>

namespace nodexa {

class SaltedSet {
public:
    explicit SaltedSet(size_t max_entries) : max_entries_(max_entries) {}
    size_t size() const { return set_.size(); }
    size_t max_entries() const { return max_entries_; }
    uint64_t evictions() const { return evictions_; }
    bool contains(const std::string& k) const { return set_.count(k) > 0; }
    // true if the entry was there; its slot in `order_` is skipped at eviction
    bool erase(const std::string& k) { return set_.erase(k) > 0; }
    void clear() {
        set_.clear();
        order_.clear();
    }
    void set_max_entries(size_t n) {
        max_entries_ = n;
        while (set_.size() > max_entries_ && !order_.empty()) pop_oldest();
    }
    // true if the entry is new (a bound of 0 keeps nothing)
    bool insert(std::string k) {
        if (max_entries_ == 0) return false;
        const uint64_t g_new = ++gen_;
        if (!set_.emplace(k, g_new).second) return false;
        order_.emplace_back(std::move(k), g_new);
        while (set_.size() > max_entries_ && !order_.empty()) pop_oldest();
        if (order_.size() > 2 * max_entries_ + 1024) {  // drop the slots of erased entries
            std::deque<std::pair<std::string, uint64_t>> live;
            for (auto& x : order_) {
                auto it = set_.find(x.first);
                if (it != set_.end() && it->second == x.second) live.push_back(x);
            }
            order_.swap(live);
        }
        return true;
    }

private:
    struct KeyHash {
        size_t operator()(const std::string& k) const {
            size_t h;
            std::memcpy(&h, k.data(), sizeof(h));  // the key is already a salted SHA-256
            return h;
        }
    };
    // drop the oldest slot; evicts its entry only if the slot is the entry's current one
    void pop_oldest() {
        auto& f = order_.front();
        auto it = set_.find(f.first);
        if (it != set_.end() && it->second == f.second) {
            set_.erase(it);
            ++evictions_;
        }
        order_.pop_front();
    }
    // live entries with the insertion generation of their slot in `order_`: an entry erased and
    // stored again later owns only its newest slot, so eviction of the stale slot (a generation
    // that no longer matches) leaves the re-inserted entry alone
    std::unordered_map<std::string, uint64_t, KeyHash> set_;
    std::deque<std::pair<std::string, uint64_t>> order_;  // insertion order, for eviction of the oldest
    uint64_t gen_ = 0;
    size_t max_entries_;
    uint64_t evictions_ = 0;
};

}  // namespace nodexa
