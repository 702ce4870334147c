// Script-execution cache: see scriptcache.hpp.
#include "scriptcache.hpp"

#include <cstring>
#include <mutex>
#include <random>
#include <string>
#include <utility>

#include "../crypto/sha256.hpp"
#include "saltedset.hpp"

namespace nodexa {

namespace {

constexpr size_t kDefaultMaxBytes = size_t(16) << 20;  // half of DEFAULT_MAX_SIG_CACHE_SIZE (32 MiB)
constexpr size_t kSaltBytes = 19;                      // 19 + 32 + 4 = 55: one SHA-256 compression

}  // namespace

struct ScriptCache::Impl {
    mutable std::mutex mu;
    SaltedSet set{kDefaultMaxBytes / 32};  // bounded, oldest first (saltedset.hpp)
    u8 salt[kSaltBytes];
    uint64_t hits = 0, misses = 0, inserts = 0, erases = 0;

    Impl() {
        std::random_device rd;
        for (auto& b : salt) b = u8(rd());
    }
    std::string key(const Uint256& wtxid, u32 flags) const {
        u8 m[kSaltBytes + 32 + 4];
        std::memcpy(m, salt, kSaltBytes);
        std::memcpy(m + kSaltBytes, wtxid.data, 32);
        for (int i = 0; i < 4; ++i) m[kSaltBytes + 32 + i] = u8(flags >> (8 * i));
        u8 out[32];
        sha256(m, sizeof(m), out);
        return std::string(reinterpret_cast<const char*>(out), 32);
    }
};

ScriptCache::ScriptCache() : impl_(new Impl) {}

ScriptCache& ScriptCache::instance() {
    static ScriptCache cache;
    return cache;
}

void ScriptCache::set_max_bytes(size_t bytes) {
    std::lock_guard<std::mutex> g(impl_->mu);
    impl_->set.set_max_entries(bytes / 32);
}

bool ScriptCache::contains(const Uint256& wtxid, u32 flags) {
    const std::string k = impl_->key(wtxid, flags);
    std::lock_guard<std::mutex> g(impl_->mu);
    const bool hit = impl_->set.contains(k);
    hit ? ++impl_->hits : ++impl_->misses;
    return hit;
}

void ScriptCache::insert(const Uint256& wtxid, u32 flags) {
    std::string k = impl_->key(wtxid, flags);
    std::lock_guard<std::mutex> g(impl_->mu);
    if (impl_->set.insert(std::move(k))) ++impl_->inserts;
}

bool ScriptCache::erase(const Uint256& wtxid, u32 flags) {
    const std::string k = impl_->key(wtxid, flags);
    std::lock_guard<std::mutex> g(impl_->mu);
    const bool was = impl_->set.erase(k);
    if (was) ++impl_->erases;
    return was;
}

void ScriptCache::clear() {
    std::lock_guard<std::mutex> g(impl_->mu);
    impl_->set.clear();
}

ScriptCache::Stats ScriptCache::stats() const {
    std::lock_guard<std::mutex> g(impl_->mu);
    Stats s;
    s.entries = impl_->set.size();
    s.max_entries = impl_->set.max_entries();
    s.hits = impl_->hits;
    s.misses = impl_->misses;
    s.inserts = impl_->inserts;
    s.erases = impl_->erases;
    s.evictions = impl_->set.evictions();
    return s;
}

}  // namespace nodexa
