// Signature cache: see sigcache.hpp.
#include "sigcache.hpp"

#include <cstring>
#include <mutex>
#include <random>
#include <shared_mutex>
#include <string>
#include <utility>

#include "../crypto/sha256.hpp"
#include "saltedset.hpp"

namespace nodexa {

namespace {

constexpr size_t kDefaultMaxBytes = size_t(32) << 20;  // DEFAULT_MAX_SIG_CACHE_SIZE (32 MiB)

}  // namespace

struct SigCache::Impl {
    mutable std::shared_mutex mu;
    SaltedSet set{kDefaultMaxBytes / 32};  // bounded, oldest first (saltedset.hpp)
    u8 salt[32];
    uint64_t hits = 0, misses = 0, inserts = 0;

    Impl() {
        std::random_device rd;
        for (auto& b : salt) b = u8(rd());
    }
    std::string key(const u8 msg[32], const Bytes& pubkey, const Bytes& sig) const {
        Bytes m;
        m.reserve(32 + 32 + pubkey.size() + sig.size());
        m.insert(m.end(), salt, salt + 32);
        m.insert(m.end(), msg, msg + 32);
        m.insert(m.end(), pubkey.begin(), pubkey.end());
        m.insert(m.end(), sig.begin(), sig.end());
        u8 out[32];
        sha256(m.data(), m.size(), out);
        return std::string(reinterpret_cast<const char*>(out), 32);
    }
};

SigCache::SigCache() : impl_(new Impl) {}

SigCache& SigCache::instance() {
    static SigCache cache;
    return cache;
}

void SigCache::set_max_bytes(size_t bytes) {
    std::unique_lock<std::shared_mutex> g(impl_->mu);
    impl_->set.set_max_entries(bytes / 32);
}

bool SigCache::get(const u8 msg[32], const Bytes& pubkey, const Bytes& sig, bool erase) {
    const std::string k = impl_->key(msg, pubkey, sig);
    if (erase) {
        std::unique_lock<std::shared_mutex> g(impl_->mu);
        const bool hit = impl_->set.erase(k);
        hit ? ++impl_->hits : ++impl_->misses;
        return hit;
    }
    std::shared_lock<std::shared_mutex> g(impl_->mu);
    const bool hit = impl_->set.contains(k);
    // counters are statistics only: benign races between readers
    hit ? __atomic_add_fetch(&impl_->hits, 1, __ATOMIC_RELAXED) : __atomic_add_fetch(&impl_->misses, 1, __ATOMIC_RELAXED);
    return hit;
}

void SigCache::put(const u8 msg[32], const Bytes& pubkey, const Bytes& sig) {
    std::string k = impl_->key(msg, pubkey, sig);
    std::unique_lock<std::shared_mutex> g(impl_->mu);
    if (impl_->set.insert(std::move(k))) ++impl_->inserts;
}

void SigCache::clear() {
    std::unique_lock<std::shared_mutex> g(impl_->mu);
    impl_->set.clear();
}

SigCache::Stats SigCache::stats() const {
    std::shared_lock<std::shared_mutex> g(impl_->mu);
    Stats s;
    s.entries = impl_->set.size();
    s.max_entries = impl_->set.max_entries();
    s.hits = impl_->hits;
    s.misses = impl_->misses;
    s.inserts = impl_->inserts;
    s.evictions = impl_->set.evictions();
    return s;
}

}  // namespace nodexa
