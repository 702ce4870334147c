// Script-execution cache: scriptExecutionCache (src/validation.cpp:9231-9335, InitScriptExecutionCache
// at src/init.cpp:1346) — a transaction whose every input script passed under a set of flags when it
// entered the mempool is remembered as a whole, so connecting the block that confirms it runs no
// script of it at all: no interpreter pass on the host, no signature, hash or CHECKMULTISIG group in
// the GPU batch. It sits one level above the signature cache (sigcache.hpp), whose key holds the
// message and so cannot serve signatures whose message only exists on the device.
//
// Entries are SHA256(salt[0:19] || wtxid || flags as LE32): 55 bytes, one compression, as the
// reference builds them. The key is the witness hash, so the same txid with another witness is
// another transaction; the flags are part of it, so an entry made under one set of rules says
// nothing under another. The salt is per process and random. The table is bounded (half of
// -maxsigcachesize, bytes of 32-byte entries) and evicts the oldest entries first. Mempool
// acceptance inserts, connect_block only looks up, and the caller erases the entries a block hit
// once that block is final (chain/state.py _connect_final).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../util/common.hpp"
#include "uint256.hpp"

namespace nodexa {

class ScriptCache {
public:
    static ScriptCache& instance();
    void set_max_bytes(size_t bytes);
    bool contains(const Uint256& wtxid, u32 flags);
    void insert(const Uint256& wtxid, u32 flags);
    bool erase(const Uint256& wtxid, u32 flags);  // true if the entry was there
    void clear();
    struct Stats {
        size_t entries = 0, max_entries = 0;
        uint64_t hits = 0, misses = 0, inserts = 0, erases = 0, evictions = 0;
    };
    Stats stats() const;

private:
    ScriptCache();
    struct Impl;
    Impl* impl_;
};

}  // namespace nodexa
