// Batch SHA-256d on gfx950 ("CPU + HIP device SHA256d for batch header hashing").
//
// sha256d_batch: one lane per fixed-length message (block headers: 80-byte KawPow inputs,
// 1459-byte Equihash-extended headers), digest = SHA256(SHA256(msg)) in the byte order of
// the reference's CHash256 / SerializeHash (src/hash.h:49,274).
// sha256d_merkle_level: one level of ComputeMerkleRoot (src/consensus/merkle.cpp): out[i] =
// SHA256d(in[2i] || in[2i+1]), the last node paired with itself on odd levels.
// Both are integer-ALU kernels (64 rounds of 32-bit rotates/adds per 64-byte block) with
// the message schedule in a 16-word register ring; SHA-256 has no MFMA shape.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kawpow_device.hpp"
#include "sha256_device.hpp"

// SHA-256 of len bytes at m (any alignment), padding generated on the fly. A block that lies
// inside the message with a dword to spare is read as 17 aligned dwords and realigned in registers
// (v_alignbyte + byte swap): 17 loads instead of 64 byte loads per block, which matters for the
// 1487-byte Equihash headers (23 such blocks each) of the resident verify's side stream. The tail
// blocks (message end, padding, length) keep the byte path, so no load reaches past the message.
__device__ void sha256_bytes(const uint8_t* m, uint32_t len, uint32_t s[8]) {
    sha256_init(s);
    const uint32_t nblocks = (len + 9 + 63) / 64;
    const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(m) & 3);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(m - mis);
    // the next in-message block's dwords are loaded before this block is compressed, so the load
    // latency hides behind the 64 rounds (one lane hashes its message's blocks one after another)
    uint32_t nxt[17];
    if (64 + 4 <= len) {
#pragma unroll
        for (int k = 0; k < 17; ++k) nxt[k] = a[k];
    }
    for (uint32_t b = 0; b < nblocks; ++b) {
        uint32_t w[16];
        if ((b + 1) * 64 + 4 <= len) {
            uint32_t d[17];
#pragma unroll
            for (int k = 0; k < 17; ++k) d[k] = nxt[k];
            if ((b + 2) * 64 + 4 <= len) {
#pragma unroll
                for (int k = 0; k < 17; ++k) nxt[k] = a[(b + 1) * 16 + k];
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = __builtin_bswap32(__builtin_amdgcn_alignbyte(d[j + 1], d[j], mis));
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                uint32_t word = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t idx = b * 64 + uint32_t(j) * 4 + uint32_t(k);
                    const uint32_t byte = idx < len ? m[idx] : (idx == len ? 0x80u : 0u);
                    word = (word << 8) | byte;
                }
                w[j] = word;
            }
        }
        if (b == nblocks - 1) {
            w[14] = len >> 29;
            w[15] = len << 3;
        }
        sha256_compress(s, w);
    }
}

extern "C" __global__ __launch_bounds__(256) void sha256d_batch(Sha256dParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    uint32_t s1[8], s2[8];
    sha256_bytes(p.in + size_t(i) * p.stride, p.len, s1);
    sha256_of_digest(s1, s2);
    store_digest(p.out + size_t(i) * 32, s2);
}

extern "C" __global__ __launch_bounds__(256) void sha256d_merkle_level(Sha256dParams p) {
    // p.n = output nodes, p.len = input nodes (32 bytes each)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t l = 2 * i, r = (2 * i + 1 < p.len) ? 2 * i + 1 : 2 * i;
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint8_t* a = p.in + size_t(l) * 32 + 4 * j;
        const uint8_t* b = p.in + size_t(r) * 32 + 4 * j;
        w[j] = (uint32_t(a[0]) << 24) | (uint32_t(a[1]) << 16) | (uint32_t(a[2]) << 8) | a[3];
        w[8 + j] = (uint32_t(b[0]) << 24) | (uint32_t(b[1]) << 16) | (uint32_t(b[2]) << 8) | b[3];
    }
    uint32_t s1[8], s2[8];
    sha256_init(s1);
    sha256_compress(s1, w);
    uint32_t pad[16] = {0x80000000u, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 512};
    sha256_compress(s1, pad);
    sha256_of_digest(s1, s2);
    store_digest(p.out + size_t(i) * 32, s2);
}

// ---------------------------------------------------------------- K4: mix-only header check
// progpow::hash_no_verify (src/crypto/ethash/lib/ethash/progpow.cpp:498-550) for a batch of KawPow
// headers, fused with the SHA256d header hash it needs (K6): header hash = SHA256d of the 80-byte
// CKAWPOWInput (src/primitives/block.h:213-233), byte-reversed into ProgPoW order (GetHex ->
// to_hash256, src/hash.cpp:269-270); seed = keccak-f800(header hash, nonce64, "rAVENCOINKAWPOW");
// final = keccak-f800(seed[0..7], claimed mix, "RAVENCOIN"). The host then sends only the headers
// whose final meets their nBits boundary to the full (DAG) check — the reference's CheckBlockHeader
// does that cheap check first for the same reason (src/validation.cpp:11638-11665).
__device__ __forceinline__ uint32_t mo_le32(const uint8_t* p) {
    return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}

__device__ __forceinline__ void mo_store_le(uint8_t* o, uint32_t w) {
    o[0] = uint8_t(w); o[1] = uint8_t(w >> 8); o[2] = uint8_t(w >> 16); o[3] = uint8_t(w >> 24);
}

extern "C" __global__ __launch_bounds__(256) void kawpow_mixonly_batch(MixOnlyParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const uint8_t* h = p.headers + size_t(i) * p.stride;
    uint8_t* o = p.out + size_t(i) * 128;
    uint32_t s1[8], s2[8];
    sha256_bytes(h, 80, s1);
    sha256_of_digest(s1, s2);
    // ProgPoW word k of the byte-reversed digest is SHA state word 7-k (its big-endian bytes reversed)
    uint32_t hh[8], st2[8], mix[8], st[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) hh[k] = s2[7 - k];
    kp_seed(hh, (uint64_t(mo_le32(h + 84)) << 32) | mo_le32(h + 80), st2);  // nonce64
#pragma unroll
    for (int k = 0; k < 8; ++k) mix[k] = __builtin_bswap32(mo_le32(h + 88 + 28 - 4 * k));  // reversed mix_hash
    kp_final(st2, mix, st);
    // nBits -> 256-bit target, big-endian bytes (arith_uint256::SetCompact; zero when negative or
    // overflowing, so nothing meets it)
    const uint32_t bits = mo_le32(h + 72);
    const uint32_t ex = bits >> 24;
    uint32_t mant = bits & 0x007fffffu;
    const bool neg = mant != 0 && (bits & 0x00800000u) != 0;
    const bool ovf = mant != 0 && (ex > 34 || (mant > 0xff && ex > 33) || (mant > 0xffff && ex > 32));
    uint8_t b[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) b[k] = 0;
    if (!neg && !ovf) {
        if (ex <= 3) {
            mant >>= 8 * (3 - ex);
            b[31] = uint8_t(mant); b[30] = uint8_t(mant >> 8); b[29] = uint8_t(mant >> 16);
        } else {
            const uint32_t s = ex - 3;  // little-endian byte position of the mantissa's low byte
            for (uint32_t q = 0; q < 3; ++q)
                if (s + q < 32) b[31 - (s + q)] = uint8_t(mant >> (8 * q));
        }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        mo_store_le(o + 4 * k, hh[k]);
        mo_store_le(o + 32 + 4 * k, st[k]);
        mo_store_le(o + 96 + 4 * k, mix[k]);
    }
#pragma unroll
    for (int k = 0; k < 32; ++k) o[64 + k] = b[k];
}
