// The consensus arithmetic every KawPow kernel shares, written once: FNV, the two ProgPoW op
// switches, the item-index modulo, the keccak-f800 absorbs with their pad words, the KISS99 mix
// seeding, the digest fold, the 64-word program encoding, and what the two search kernels do
// with a finished hash (share append, stale-work check). Reference behaviour: progpow.cpp
// (src/crypto/ethash/lib/ethash/progpow.cpp:158-355); the CPU golden model is csrc/pow/kawpow.cpp.
//
// The round bodies are NOT here: they differ in how the 32-word mix is held (LDS in
// kawpow_verify.hip and kl_verify, VGPRs behind switches in kawpow_anyperiod.hip, VGPRs behind
// the handler table in kawpow_verify_waves, literal registers in kawpow_search.hip), and a fill
// or a round that reaches the mix through a callback or an out-array puts it into scratch.
#pragma once
#include "kernel_params.h"
#include "keccak_device.hpp"

#define KP_FNV_PRIME 0x01000193u
#define KP_FNV_OFFSET 0x811c9dc5u
NX_DEV uint32_t kp_fnv1(uint32_t u, uint32_t v) { return (u * KP_FNV_PRIME) ^ v; }
NX_DEV uint32_t kp_fnv1a(uint32_t h, uint32_t d) { return (h ^ d) * KP_FNV_PRIME; }
NX_DEV uint32_t kp_clz(uint32_t x) { return x ? (uint32_t)__builtin_clz(x) : 32u; }

// x mod f.d, Barrett: q' = floor(x * floor(2^32/d) / 2^32) is q or q-1, so r' < 2d and one
// unsigned min(r', r'-d) finishes it (r'-d wraps high when r' < d). 5 ops.
NX_DEV uint32_t kp_mod(uint32_t x, const FastMod32& f) {
    const uint32_t r = x - __umulhi(x, f.mb) * f.d;
    return min(r, r - f.d);
}
// x mod f.d, the older round-up multiply-shift form (kernel_params.h: FastMod32)
NX_DEV uint32_t kp_mod_shift(uint32_t x, const FastMod32& f) {
    const uint32_t t = __umulhi(x, f.m);
    const uint32_t q = (t + ((x - t) >> 1)) >> (f.s - 1);
    return x - q * f.d;
}

NX_DEV uint32_t kp_merge(uint32_t a, uint32_t b, uint32_t kind, uint32_t rot) {
    switch (kind) {
        case 0: return a * 33u + b;
        case 1: return (a ^ b) * 33u;
        case 2: return __builtin_rotateleft32(a, rot) ^ b;
        default: return __builtin_rotateright32(a, rot) ^ b;
    }
}

NX_DEV uint32_t kp_math(uint32_t a, uint32_t b, uint32_t kind) {
    switch (kind) {
        case 0: return a + b;
        case 1: return a * b;
        case 2: return __umulhi(a, b);
        case 3: return min(a, b);
        case 4: return __builtin_rotateleft32(a, b);
        case 5: return __builtin_rotateright32(a, b);
        case 6: return a & b;
        case 7: return a | b;
        case 8: return a ^ b;
        case 9: return kp_clz(a) + kp_clz(b);
        default: return (uint32_t)(__builtin_popcount(a) + __builtin_popcount(b));
    }
}

// Program encoding, KV_PROG_WORDS (64) u32 per period, 51 of them used
// (csrc/pow/kawpow.cpp make_kawpow_program; KV_PROG_WORDS lives in kernel_params.h):
//   [0..10]  cache op i : src | dst << 8 | merge_kind << 16 | rot << 24
//   [11..28] math op i  : src1 | src2 << 8 | math_kind << 16 | dst << 24
//   [29..46] math merge : merge_kind | rot << 8
//   [47..50] dag merge  : dst | merge_kind << 8 | rot << 16
// Math op i runs after cache op i (i < 11); its result is merged by math merge i.
#define KP_PROG_CACHE 0
#define KP_PROG_MATH 11
#define KP_PROG_MMERGE 29
#define KP_PROG_DAG 47
#define KP_PROG_OPS 51
NX_DEV uint32_t kp_cache_src(uint32_t op) { return op & 31; }
NX_DEV uint32_t kp_cache_dst(uint32_t op) { return (op >> 8) & 31; }
NX_DEV uint32_t kp_cache_kind(uint32_t op) { return (op >> 16) & 3; }
NX_DEV uint32_t kp_cache_rot(uint32_t op) { return op >> 24; }
NX_DEV uint32_t kp_math_src1(uint32_t op) { return op & 31; }
NX_DEV uint32_t kp_math_src2(uint32_t op) { return (op >> 8) & 31; }
NX_DEV uint32_t kp_math_kind(uint32_t op) { return (op >> 16) & 15; }
NX_DEV uint32_t kp_math_dst(uint32_t op) { return op >> 24; }
NX_DEV uint32_t kp_mmerge_kind(uint32_t mg) { return mg & 3; }
NX_DEV uint32_t kp_mmerge_rot(uint32_t mg) { return mg >> 8; }
NX_DEV uint32_t kp_dag_dst(uint32_t op) { return op & 31; }
NX_DEV uint32_t kp_dag_kind(uint32_t op) { return (op >> 8) & 3; }
NX_DEV uint32_t kp_dag_rot(uint32_t op) { return op >> 16; }

// "rAVENCOINKAWPOW" padding words (one byte per u32): all 15 after the seed absorb's header and
// nonce, the first 9 after the final absorb's seed state and mix digest.
#define KP_PAD0 0x72u
#define KP_PAD1 0x41u
#define KP_PAD2 0x56u
#define KP_PAD3 0x45u
#define KP_PAD4 0x4Eu
#define KP_PAD5 0x43u
#define KP_PAD6 0x4Fu
#define KP_PAD7 0x49u
#define KP_PAD8 0x4Eu
#define KP_PAD9 0x4Bu
#define KP_PAD10 0x41u
#define KP_PAD11 0x57u
#define KP_PAD12 0x50u
#define KP_PAD13 0x4Fu
#define KP_PAD14 0x57u

NX_DEV void kp_seed(const uint32_t header[8], uint64_t nonce, uint32_t st2[8]) {
    uint32_t s[25];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = header[i];
    s[8] = (uint32_t)nonce;
    s[9] = (uint32_t)(nonce >> 32);
    s[10] = KP_PAD0; s[11] = KP_PAD1; s[12] = KP_PAD2; s[13] = KP_PAD3; s[14] = KP_PAD4;
    s[15] = KP_PAD5; s[16] = KP_PAD6; s[17] = KP_PAD7; s[18] = KP_PAD8; s[19] = KP_PAD9;
    s[20] = KP_PAD10; s[21] = KP_PAD11; s[22] = KP_PAD12; s[23] = KP_PAD13; s[24] = KP_PAD14;
    keccak_f800(s);
#pragma unroll
    for (int i = 0; i < 8; ++i) st2[i] = s[i];
}

NX_DEV void kp_final(const uint32_t st2[8], const uint32_t digest[8], uint32_t out[8]) {
    uint32_t s[25];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = st2[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[8 + i] = digest[i];
    s[16] = KP_PAD0; s[17] = KP_PAD1; s[18] = KP_PAD2; s[19] = KP_PAD3; s[20] = KP_PAD4;
    s[21] = KP_PAD5; s[22] = KP_PAD6; s[23] = KP_PAD7; s[24] = KP_PAD8;
    keccak_f800(s);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = s[i];
}

struct KpKiss {
    uint32_t z, w, jsr, jcong;
    NX_DEV uint32_t next() {
        z = 36969u * (z & 0xffffu) + (z >> 16);
        w = 18000u * (w & 0xffffu) + (w >> 16);
        jcong = 69069u * jcong + 1234567u;
        jsr ^= (jsr << 17);
        jsr ^= (jsr >> 13);
        jsr ^= (jsr << 5);
        return (((z << 16) + w) ^ jcong) + jsr;
    }
};

// The generator that fills a lane's mix: seeded from the hash's seed-state words 0 and 1 and the
// lane. Mix word r is the r-th next(); the 32-word fill loop and its store stay with the caller.
NX_DEV KpKiss kp_mix_rng(uint32_t s0, uint32_t s1, uint32_t lane) {
    const uint32_t z = kp_fnv1a(KP_FNV_OFFSET, s0);
    const uint32_t w = kp_fnv1a(z, s1);
    const uint32_t jsr = kp_fnv1a(w, lane);
    return KpKiss{z, w, jsr, kp_fnv1a(jsr, lane)};
}

// digest[k] = fold(lane_hash[k], lane_hash[k + 8]) over the group's 16 lane hashes; every lane of
// the group runs the (convergent) shuffles and gets the word.
NX_DEV uint32_t kp_digest_fold(uint32_t lo, uint32_t hi) { return kp_fnv1a(kp_fnv1a(KP_FNV_OFFSET, lo), hi); }
NX_DEV uint32_t kp_digest_word(uint32_t lane_hash, int k) {
    return kp_digest_fold(__shfl(lane_hash, k, 16), __shfl(lane_hash, k + 8, 16));
}

// Result row `row` of a batch kernel: mix[8] then final[8]. (kawpow_hash_batch and kawpow_hash_any
// write the same row with a loop of their own; profiles/r16_kawpow_header says why.)
NX_DEV void kp_store_hash(uint32_t* out, uint32_t row,const uint32_t digest[8], const uint32_t fin[8]) {
    uint32_t* o = out + (size_t)row * 16;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        o[k] = digest[k];
        o[8 + k] = fin[k];
    }
}

// The share rule of both search kernels: a nonce is a share if the upper 64 bits of its final hash
// (big-endian) are <= target. `count` keeps counting past the ring; shares beyond it are dropped.
NX_DEV void kp_append_share(KawpowResults* results, uint64_t target, uint64_t nonce, const uint32_t digest[8],
                            const uint32_t fin[8]) {
    const uint64_t head = ((uint64_t)__builtin_bswap32(fin[0]) << 32) | __builtin_bswap32(fin[1]);
    if (head <= target) {
        const uint32_t slot = atomicAdd(&results->count, 1u);
        if (slot < NODEXA_KAWPOW_MAX_SHARES) {
            KawpowShare* s = &results->shares[slot];
            s->nonce = nonce;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                s->mix[k] = digest[k];
                s->final_[k] = fin[k];
            }
        }
    }
}

// Stale-work check, run by thread 0 of a search workgroup before the barrier that publishes
// *stale: one uncached read of the host-mapped generation word per workgroup (overlapped with the
// L1 fill), so a template change stops queued work within one workgroup's lifetime. A stale
// workgroup counts itself in `skipped` and searches nothing.
NX_DEV void kp_check_stale(uint32_t* stale, const uint32_t* gen_word, uint32_t generation, KawpowResults* results) {
    uint32_t s = 0;
    if (gen_word) s = __hip_atomic_load(gen_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != generation;
    *stale = s;
    if (s) atomicAdd(&results->skipped, 1u);
}
