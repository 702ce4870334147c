// KawPow nonce search for gfx950 with the period's program as data: one static code object
// mines any ProgPoW period (kawpow_search_any), so the miner has something to launch while
// the per-period specialised kernel (kawpow_search.hip, compiled by ops/jit.py) does not
// exist yet: cold start, blocks that come faster than a compile, height jumps, rigs without
// the compiler. kawpow_hash_any is the batch-hash twin (explicit (header, nonce) jobs).
//
// Reference behaviour: progpow::search / hash (src/crypto/ethash/lib/ethash/progpow.cpp:
// 298-355, 553-579); the CPU golden model is csrc/pow/kawpow.cpp, and every op below is the
// arithmetic of kl_verify<true> (kawpow_verify_light.hip), bit for bit.
//
// CDNA4 mapping
//   * the search contract is kawpow_search's: one nonce per thread, a 16-thread group is
//     one hash, the group walks its 16 nonces (one keccak-f800 seed per nonce, not 16), the
//     same KawpowResults ring, the same per-workgroup stale-work check.
//   * ONE program serves the whole launch, so it is uniform over every wave: its 51 op
//     words are read once into SGPRs, the op and merge kinds are scalar branches, and the
//     32-word mix stays in VGPRs, addressed by uniform register moves (the form of
//     kawpow_verify_waves, without its handler-slot table: plain C++ switches, so this
//     module needs no jump-slot stamp and loads where the LLVM tools that check one are
//     missing). LDS holds only the 16 KiB L1.
//   * a workgroup is 256 threads whatever the launch granule: it covers `granule` nonces
//     (the KP_BLOCK of the specialised variant for the same DAG, 768 tuned) in
//     ceil(granule / 256) passes, so a window is cut the same way for both kernels and
//     `skipped` counts the same units.
//   * DAG item addresses are 64-bit ((size_t)index * 16 + slice over uint4): DAGs of 4 GiB
//     and more need no other variant.
#include "kernel_params.h"
#include "keccak_device.hpp"

#define KA_BLOCK 256
// 6 waves per SIMD (80 VGPRs, no spill): 44.8 MH/s at epoch 384 against 41.6 at the 4 waves the
// compiler picks unbounded (101 VGPRs); 7 and 8 waves spill the mix to scratch for +1 %
// (profiles/r7_kawpow_anyperiod). The kernel is bound by the scalar dispatch, not by occupancy.
#define KA_MIN_WAVES 6

NX_DEV uint32_t ka_fnv1a(uint32_t h, uint32_t d) { return (h ^ d) * 0x01000193u; }
NX_DEV uint32_t ka_mod(uint32_t x, const FastMod32& f) {
    const uint32_t r = x - __umulhi(x, f.mb) * f.d;  // Barrett estimate, one correction (kernel_params.h)
    return min(r, r - f.d);
}
NX_DEV uint32_t ka_clz(uint32_t x) { return x ? (uint32_t)__builtin_clz(x) : 32u; }

NX_DEV uint32_t ka_merge(uint32_t a, uint32_t b, uint32_t kind, uint32_t rot) {
    switch (kind) {
        case 0: return a * 33u + b;
        case 1: return (a ^ b) * 33u;
        case 2: return __builtin_rotateleft32(a, rot) ^ b;
        default: return __builtin_rotateright32(a, rot) ^ b;
    }
}

NX_DEV uint32_t ka_math(uint32_t a, uint32_t b, uint32_t kind) {
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
        case 9: return ka_clz(a) + ka_clz(b);
        default: return (uint32_t)(__builtin_popcount(a) + __builtin_popcount(b));
    }
}

typedef uint32_t ka_mix_t __attribute__((ext_vector_type(32)));
NX_DEV uint32_t ka_get(const ka_mix_t& m, uint32_t i) { return m[i & 31]; }
NX_DEV void ka_set(ka_mix_t& m, uint32_t i, uint32_t v) { m[i & 31] = v; }

// The absorb pads are "rAVENCOINKAWPOW", one byte per u32.
NX_DEV void ka_seed(const uint32_t header[8], uint64_t nonce, uint32_t st2[8]) {
    uint32_t s[25];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = header[i];
    s[8] = (uint32_t)nonce;
    s[9] = (uint32_t)(nonce >> 32);
    const uint32_t pad[15] = {0x72, 0x41, 0x56, 0x45, 0x4E, 0x43, 0x4F, 0x49, 0x4E, 0x4B, 0x41, 0x57, 0x50, 0x4F, 0x57};
#pragma unroll
    for (int i = 0; i < 15; ++i) s[10 + i] = pad[i];
    keccak_f800(s);
#pragma unroll
    for (int i = 0; i < 8; ++i) st2[i] = s[i];
}

NX_DEV void ka_final(const uint32_t st2[8], const uint32_t digest[8], uint32_t out[8]) {
    uint32_t s[25];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = st2[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[8 + i] = digest[i];
    const uint32_t pad[9] = {0x72, 0x41, 0x56, 0x45, 0x4E, 0x43, 0x4F, 0x49, 0x4E};
#pragma unroll
    for (int i = 0; i < 9; ++i) s[16 + i] = pad[i];
    keccak_f800(s);
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = s[i];
}

// The period's 51 op words in SGPRs (the program is uniform over the launch).
struct KaProgram {
    uint32_t w[51];
};
NX_DEV void ka_load_program(KaProgram& pg, const uint32_t* program) {
#pragma unroll
    for (int i = 0; i < 51; ++i) pg.w[i] = __builtin_amdgcn_readfirstlane(program[i]);
}

// The group's 16 hashes, one after the other: hash h's seed words live in lane h (`st0`, `st1`);
// its 8 digest words end in `own` of that lane.
NX_DEV void ka_group_hashes(const uint4* __restrict__ dag, const FastMod32& items, const uint32_t* l1,
                            KaProgram& pg, uint32_t st0, uint32_t st1, uint32_t lane, uint32_t (&own)[8]) {
#pragma unroll 1
    for (uint32_t h = 0; h < 16; ++h) {
        ka_mix_t mix;
        {
            const uint32_t z0 = ka_fnv1a(0x811c9dc5u, __shfl(st0, (int)h, 16));
            const uint32_t w0 = ka_fnv1a(z0, __shfl(st1, (int)h, 16));
            const uint32_t jsr0 = ka_fnv1a(w0, lane);
            uint32_t kz = z0, kw = w0, kj = jsr0, kc = ka_fnv1a(jsr0, lane);
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                kz = 36969u * (kz & 0xffffu) + (kz >> 16);
                kw = 18000u * (kw & 0xffffu) + (kw >> 16);
                kc = 69069u * kc + 1234567u;
                kj ^= (kj << 17);
                kj ^= (kj >> 13);
                kj ^= (kj << 5);
                mix[r] = (((kz << 16) + kw) ^ kc) + kj;
            }
        }
#pragma unroll 1
        for (uint32_t r = 0; r < 64; ++r) {
            const uint32_t index = ka_mod(__shfl(mix[0], (int)(r & 15), 16), items);
            // lane l merges words ((l^r)%16)*4..+3 of the 2048-bit item: load exactly that slice
            const uint4 d = dag[(size_t)index * 16 + ((lane ^ r) & 15)];
            // opaque per round: the op fields are decoded where they are used (SALU, next to the
            // op) instead of being hoisted out of the loop into loop-invariant SGPRs that spill
#pragma unroll
            for (int i = 0; i < 51; ++i) asm volatile("" : "+s"(pg.w[i]));
#pragma unroll
            for (int i = 0; i < 18; ++i) {
                if (i < 11) {
                    const uint32_t op = pg.w[i];
                    const uint32_t dst = (op >> 8) & 31;
                    ka_set(mix, dst, ka_merge(ka_get(mix, dst), l1[ka_get(mix, op) & 4095u], (op >> 16) & 3, op >> 24));
                }
                const uint32_t op = pg.w[11 + i];
                const uint32_t mg = pg.w[29 + i];
                const uint32_t dst = op >> 24;
                const uint32_t v = ka_math(ka_get(mix, op), ka_get(mix, op >> 8), (op >> 16) & 15);
                ka_set(mix, dst, ka_merge(ka_get(mix, dst), v, mg & 3, mg >> 8));
            }
            const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t op = pg.w[47 + i];
                ka_set(mix, op, ka_merge(ka_get(mix, op), dw[i], (op >> 8) & 3, op >> 16));
            }
        }
        uint32_t lh = 0x811c9dc5u;
#pragma unroll
        for (int r = 0; r < 32; ++r) lh = ka_fnv1a(lh, mix[r]);
        const bool mine = lane == h;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            // digest[k] = fnv1a(fnv1a(basis, lane_hash[k]), lane_hash[k + 8]); every lane runs the
            // (convergent) shuffles, only the owner of hash h keeps the words
            const uint32_t a = __shfl(lh, k, 16);
            const uint32_t b = __shfl(lh, k + 8, 16);
            const uint32_t word = ka_fnv1a(ka_fnv1a(0x811c9dc5u, a), b);
            own[k] = mine ? word : own[k];
        }
    }
}

extern "C" __global__ __launch_bounds__(KA_BLOCK, KA_MIN_WAVES) void kawpow_search_any(KawpowAnySearchParams p) {
    __shared__ uint32_t l1[4096];
    __shared__ uint32_t stale_word;
    if (blockDim.x != KA_BLOCK) return;  // launched with the wrong block: no shares rather than bad ones
    if (threadIdx.x == 0) {
        // one uncached read of the host-mapped generation word per workgroup, overlapped with the
        // L1 fill below: a template change stops queued work within one workgroup's lifetime
        uint32_t s = 0;
        if (p.gen_word) s = __hip_atomic_load(p.gen_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != p.generation;
        stale_word = s;
        if (s) atomicAdd(&p.results->skipped, 1u);
    }
    for (int i = threadIdx.x; i < 4096; i += KA_BLOCK) l1[i] = p.l1[i];
    __syncthreads();
    if (stale_word) return;  // uniform over the workgroup

    KaProgram pg;
    ka_load_program(pg, p.program);
    const uint32_t lane = threadIdx.x & 15;
    const uint4* dag = (const uint4*)p.dag;
    // no barrier below: a wave whose threads all lie past the granule skips its pass
#pragma unroll 1
    for (uint32_t t = threadIdx.x; t < p.granule; t += KA_BLOCK) {  // granule % 64 == 0: wave-uniform
        const uint64_t nonce = p.start_nonce + (uint64_t)blockIdx.x * p.granule + t;
        uint32_t st2[8], digest[8] = {0, 0, 0, 0, 0, 0, 0, 0}, fin[8];
        ka_seed(p.header, nonce, st2);
        ka_group_hashes(dag, p.items, l1, pg, st2[0], st2[1], lane, digest);
        ka_final(st2, digest, fin);
        const uint64_t head = ((uint64_t)__builtin_bswap32(fin[0]) << 32) | __builtin_bswap32(fin[1]);
        if (head <= p.target) {
            const uint32_t slot = atomicAdd(&p.results->count, 1u);
            if (slot < NODEXA_KAWPOW_MAX_SHARES) {
                KawpowShare* s = &p.results->shares[slot];
                s->nonce = nonce;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    s->mix[k] = digest[k];
                    s->final_[k] = fin[k];
                }
            }
        }
    }
}

// Batch hash (no target) of (header, nonce) jobs that all belong to the period of `program`.
// One job per thread, grouped as in the search; out per job: mix[8] then final[8].
extern "C" __global__ __launch_bounds__(KA_BLOCK, KA_MIN_WAVES) void kawpow_hash_any(KawpowAnyHashParams p) {
    __shared__ uint32_t l1[4096];
    if (blockDim.x != KA_BLOCK) return;
    for (int i = threadIdx.x; i < 4096; i += KA_BLOCK) l1[i] = p.l1[i];
    __syncthreads();
    KaProgram pg;
    ka_load_program(pg, p.program);
    const uint32_t lane = threadIdx.x & 15;
    const uint32_t job = blockIdx.x * KA_BLOCK + threadIdx.x;
    const bool valid = job < p.num_jobs;
    const KawpowVerifyJob j = p.jobs[valid ? job : 0];
    uint32_t st2[8], digest[8] = {0, 0, 0, 0, 0, 0, 0, 0}, fin[8];
    ka_seed(j.header, j.nonce, st2);
    ka_group_hashes((const uint4*)p.dag, p.items, l1, pg, st2[0], st2[1], lane, digest);
    ka_final(st2, digest, fin);
    if (valid) {
        uint32_t* o = p.out + (size_t)job * 16;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            o[k] = digest[k];
            o[8 + k] = fin[k];
        }
    }
}
