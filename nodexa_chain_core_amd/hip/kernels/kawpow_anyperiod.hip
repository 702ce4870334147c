// KawPow nonce search for gfx950 with the period's program as data: one static code object
// mines any ProgPoW period (kawpow_search_any), so the miner has something to launch while
// the per-period specialised kernel (kawpow_search.hip, compiled by ops/jit.py) does not
// exist yet: cold start, blocks that come faster than a compile, height jumps, rigs without
// the compiler. kawpow_hash_any is the batch-hash twin (explicit (header, nonce) jobs).
//
// Reference behaviour: progpow::search / hash (src/crypto/ethash/lib/ethash/progpow.cpp:
// 298-355, 553-579); the CPU golden model is csrc/pow/kawpow.cpp. The arithmetic, the program
// encoding, the share rule and the stale-work check are kawpow_device.hpp's, shared with every
// other KawPow kernel.
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
#include "kawpow_device.hpp"

#define KA_BLOCK 256
// 6 waves per SIMD (80 VGPRs, no spill): 44.8 MH/s at epoch 384 against 41.6 at the 4 waves the
// compiler picks unbounded (101 VGPRs); 7 and 8 waves spill the mix to scratch for +1 %
// (profiles/r7_kawpow_anyperiod). The kernel is bound by the scalar dispatch, not by occupancy.
#define KA_MIN_WAVES 6

typedef uint32_t ka_mix_t __attribute__((ext_vector_type(32)));
NX_DEV uint32_t ka_get(const ka_mix_t& m, uint32_t i) { return m[i & 31]; }
NX_DEV void ka_set(ka_mix_t& m, uint32_t i, uint32_t v) { m[i & 31] = v; }

// The period's 51 op words in SGPRs (the program is uniform over the launch).
struct KaProgram {
    uint32_t w[KP_PROG_OPS];
};
NX_DEV void ka_load_program(KaProgram& pg, const uint32_t* program) {
#pragma unroll
    for (int i = 0; i < KP_PROG_OPS; ++i) pg.w[i] = __builtin_amdgcn_readfirstlane(program[i]);
}

// The group's 16 hashes, one after the other: hash h's seed words live in lane h (`st0`, `st1`);
// its 8 digest words end in `own` of that lane.
NX_DEV void ka_group_hashes(const uint4* __restrict__ dag, const FastMod32& items, const uint32_t* l1,
                            KaProgram& pg, uint32_t st0, uint32_t st1, uint32_t lane, uint32_t (&own)[8]) {
#pragma unroll 1
    for (uint32_t h = 0; h < 16; ++h) {
        ka_mix_t mix;
        {
            KpKiss rng = kp_mix_rng(__shfl(st0, (int)h, 16), __shfl(st1, (int)h, 16), lane);
#pragma unroll
            for (int r = 0; r < 32; ++r) mix[r] = rng.next();
        }
#pragma unroll 1
        for (uint32_t r = 0; r < 64; ++r) {
            const uint32_t index = kp_mod(__shfl(mix[0], (int)(r & 15), 16), items);
            // lane l merges words ((l^r)%16)*4..+3 of the 2048-bit item: load exactly that slice
            const uint4 d = dag[(size_t)index * 16 + ((lane ^ r) & 15)];
            // opaque per round: the op fields are decoded where they are used (SALU, next to the
            // op) instead of being hoisted out of the loop into loop-invariant SGPRs that spill
#pragma unroll
            for (int i = 0; i < KP_PROG_OPS; ++i) asm volatile("" : "+s"(pg.w[i]));
#pragma unroll
            for (int i = 0; i < 18; ++i) {
                if (i < 11) {
                    const uint32_t op = pg.w[KP_PROG_CACHE + i];
                    const uint32_t dst = kp_cache_dst(op);
                    ka_set(mix, dst, kp_merge(ka_get(mix, dst), l1[ka_get(mix, kp_cache_src(op)) & 4095u], kp_cache_kind(op),
                                              kp_cache_rot(op)));
                }
                const uint32_t op = pg.w[KP_PROG_MATH + i];
                const uint32_t mg = pg.w[KP_PROG_MMERGE + i];
                const uint32_t dst = kp_math_dst(op);
                const uint32_t v = kp_math(ka_get(mix, kp_math_src1(op)), ka_get(mix, kp_math_src2(op)), kp_math_kind(op));
                ka_set(mix, dst, kp_merge(ka_get(mix, dst), v, kp_mmerge_kind(mg), kp_mmerge_rot(mg)));
            }
            const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t op = pg.w[KP_PROG_DAG + i];
                const uint32_t dst = kp_dag_dst(op);
                ka_set(mix, dst, kp_merge(ka_get(mix, dst), dw[i], kp_dag_kind(op), kp_dag_rot(op)));
            }
        }
        uint32_t lh = KP_FNV_OFFSET;
#pragma unroll
        for (int r = 0; r < 32; ++r) lh = kp_fnv1a(lh, mix[r]);
        const bool mine = lane == h;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            // every lane gets the word, only the owner of hash h keeps it
            const uint32_t word = kp_digest_word(lh, k);
            own[k] = mine ? word : own[k];
        }
    }
}

extern "C" __global__ __launch_bounds__(KA_BLOCK, KA_MIN_WAVES) void kawpow_search_any(KawpowAnySearchParams p) {
    __shared__ uint32_t l1[4096];
    __shared__ uint32_t stale_word;
    if (blockDim.x != KA_BLOCK) return;  // launched with the wrong block: no shares rather than bad ones
    if (threadIdx.x == 0) kp_check_stale(&stale_word, p.gen_word, p.generation, p.results);
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
        kp_seed(p.header, nonce, st2);
        ka_group_hashes(dag, p.items, l1, pg, st2[0], st2[1], lane, digest);
        kp_final(st2, digest, fin);
        kp_append_share(p.results, p.target, nonce, digest, fin);
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
    kp_seed(j.header, j.nonce, st2);
    ka_group_hashes((const uint4*)p.dag, p.items, l1, pg, st2[0], st2[1], lane, digest);
    kp_final(st2, digest, fin);
    if (valid) {
        // kp_store_hash's row, kept inline as in kawpow_hash_batch: through the call this kernel's
        // median time left the spread of the kernel before it (profiles/r16_kawpow_header)
        uint32_t* o = p.out + (size_t)job * 16;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            o[k] = digest[k];
            o[8 + k] = fin[k];
        }
    }
}
