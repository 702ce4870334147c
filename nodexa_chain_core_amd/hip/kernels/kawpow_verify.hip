// KawPow batch verification kernel for gfx950 — one launch covers every
// ProgPoW period in the batch (BASELINE config 5).
//
// The search kernel bakes one period's program into the code; a batch of
// headers from a chain segment spans many periods (3 blocks each), so here the
// program is data: the host materialises each distinct period's op list
// (csrc/pow/kawpow.cpp make_kawpow_program) and sorts jobs so that every
// wave64 (4 hashes x 16 lanes, 64 jobs walked by the wave) shares one period.
// The op fields are then wave-uniform (readfirstlane), so the 32-word mix (in
// LDS, [wave][group][reg][lane]) is addressed with uniform offsets instead of a
// divergent waterfall. Each group walks 16 jobs of its slab, so this layout
// suits periods with many jobs; a header batch (3 headers per period) uses
// kawpow_verify_waves (kawpow_verify_light.hip) instead.
#include "kawpow_device.hpp"

// The mix lives in LDS: [wave][group(4)][reg(32)][lane(16)] so a uniform-register
// access by the 64 threads of a wave touches 64 consecutive words (conflict-free).
#define KV_MIX(r) mixs[(wslot * 32 + (r)) * 64 + tl]

extern "C" __global__ __launch_bounds__(256) void kawpow_verify_batch(KawpowVerifyParams p) {
    __shared__ uint32_t l1[4096];
    __shared__ uint32_t mixs[4 * 32 * 64];  // 4 waves x 32 regs x 64 threads
    {
        const uint4* src = (const uint4*)p.dag;
        uint4* dst = (uint4*)l1;
        for (int i = threadIdx.x; i < 1024; i += 256) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t tl = threadIdx.x & 63;  // thread within wave
    const uint32_t wslot = threadIdx.x >> 6;
    const uint32_t lane = threadIdx.x & 15;
    const uint32_t job = blockIdx.x * 256 + threadIdx.x;
    const uint32_t slab = __builtin_amdgcn_readfirstlane(job >> 6);
    // num_jobs is a multiple of 64, so this exit is wave-uniform; waves past the
    // last slab must not index job_program (it has num_jobs / 64 entries).
    if (slab >= (p.num_jobs >> 6)) return;
    const uint32_t* prog = p.programs + (size_t)p.job_program[slab] * KV_PROG_WORDS;
    const bool valid = job < p.num_jobs;
    const KawpowVerifyJob j = p.jobs[valid ? job : 0];
    uint32_t st2[8];
    kp_seed(j.header, j.nonce, st2);
    uint32_t digest[8];
    for (uint32_t h = 0; h < 16; ++h) {
        KpKiss rng = kp_mix_rng(__shfl(st2[0], (int)h, 16), __shfl(st2[1], (int)h, 16), lane);
        for (int r = 0; r < 32; ++r) KV_MIX(r) = rng.next();
        for (uint32_t r = 0; r < 64; ++r) {
            const uint32_t src = __shfl(KV_MIX(0), (int)(r & 15), 16);
            const uint32_t index = kp_mod_shift(src, p.items);
            const uint4 d = ((const uint4*)p.dag)[(size_t)index * 16 + ((lane ^ r) & 15)];
            for (int i = 0; i < 18; ++i) {
                if (i < 11) {
                    const uint32_t op = __builtin_amdgcn_readfirstlane(prog[KP_PROG_CACHE + i]);
                    const uint32_t a = KV_MIX(kp_cache_src(op));
                    uint32_t& dst = KV_MIX(kp_cache_dst(op));
                    dst = kp_merge(dst, l1[a & 4095u], kp_cache_kind(op), kp_cache_rot(op));
                }
                const uint32_t op = __builtin_amdgcn_readfirstlane(prog[KP_PROG_MATH + i]);
                const uint32_t mg = __builtin_amdgcn_readfirstlane(prog[KP_PROG_MMERGE + i]);
                const uint32_t v = kp_math(KV_MIX(kp_math_src1(op)), KV_MIX(kp_math_src2(op)), kp_math_kind(op));
                uint32_t& dst = KV_MIX(kp_math_dst(op));
                dst = kp_merge(dst, v, kp_mmerge_kind(mg), kp_mmerge_rot(mg));
            }
            const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
            for (int i = 0; i < 4; ++i) {
                const uint32_t op = __builtin_amdgcn_readfirstlane(prog[KP_PROG_DAG + i]);
                uint32_t& dst = KV_MIX(kp_dag_dst(op));
                dst = kp_merge(dst, dw[i], kp_dag_kind(op), kp_dag_rot(op));
            }
        }
        uint32_t lh = KP_FNV_OFFSET;
        for (int r = 0; r < 32; ++r) lh = kp_fnv1a(lh, KV_MIX(r));
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t v = kp_digest_word(lh, k);
            if (h == lane) digest[k] = v;
        }
    }
    uint32_t fin[8];
    kp_final(st2, digest, fin);
    if (valid) kp_store_hash(p.out, job, digest, fin);
}
