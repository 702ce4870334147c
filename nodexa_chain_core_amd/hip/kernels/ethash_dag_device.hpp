// One Ethash 512-bit dataset item per aligned lane quad: the computation shared by the DAG build
// (ethash_dag.hip) and the DAG audit (ethash_dag_check.hip). See ethash_dag.hip for the mapping.
#pragma once
#include "kernel_params.h"
#include "keccak_device.hpp"

NX_DEV uint32_t fnv1(uint32_t u, uint32_t v) { return (u * 0x01000193u) ^ v; }

NX_DEV uint32_t dag_mod(uint32_t x, const FastMod32& f) {
    const uint32_t r = x - __umulhi(x, f.mb) * f.d;  // Barrett estimate, one correction (kernel_params.h)
    return min(r, r - f.d);
}

// lane C of each aligned quad, to the whole quad
template <int C>
NX_DEV uint32_t dag_quad_bcast(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, C * 0x55, 0xf, 0xf, false);
}

// Bytes 16s..16s+15 of item `index`, for lane s of the quad. All four lanes of the quad must be
// active and share `index` (the quad broadcasts read their registers). `index` and `s` come by
// reference: hipcc then compiles ethash_dag_build to the code it had with this body written in the
// kernel (78 VGPRs; by value it takes 79 and allocates registers differently).
NX_DEV uint4 dag_item_quad(const void* light_cache, const FastMod32& lmod, const uint64_t& index,
                           const uint32_t& s) {
    const uint4* __restrict__ light = (const uint4*)light_cache;
    const uint32_t seed = (uint32_t)index;  // index < 2^32 for every supported epoch

    uint32_t m[4];
    {
        const uint32_t li = dag_mod(seed, lmod);
        uint64_t in[8], out[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 v = light[(size_t)li * 4 + k];
            in[2 * k] = ((uint64_t)v.y << 32) | v.x;
            in[2 * k + 1] = ((uint64_t)v.w << 32) | v.z;
        }
        in[0] ^= seed;
        keccak512_64(in, out);
        const uint64_t lo = (s & 2) ? ((s & 1) ? out[6] : out[4]) : ((s & 1) ? out[2] : out[0]);
        const uint64_t hi = (s & 2) ? ((s & 1) ? out[7] : out[5]) : ((s & 1) ? out[3] : out[1]);
        m[0] = (uint32_t)lo;
        m[1] = (uint32_t)(lo >> 32);
        m[2] = (uint32_t)hi;
        m[3] = (uint32_t)(hi >> 32);
    }

#pragma unroll 1
    for (uint32_t j = 0; j < 512; j += 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t own = m[k & 3];
            uint32_t mk;
            switch (k >> 2) {
                case 0: mk = dag_quad_bcast<0>(own); break;
                case 1: mk = dag_quad_bcast<1>(own); break;
                case 2: mk = dag_quad_bcast<2>(own); break;
                default: mk = dag_quad_bcast<3>(own); break;
            }
            const uint32_t parent = dag_mod(fnv1(seed ^ (j + (uint32_t)k), mk), lmod);
            const uint4 v = light[(size_t)parent * 4 + s];
            m[0] = fnv1(m[0], v.x);
            m[1] = fnv1(m[1], v.y);
            m[2] = fnv1(m[2], v.z);
            m[3] = fnv1(m[3], v.w);
        }
    }

    // final keccak512 over the whole 16-word mix, gathered from the quad
    uint32_t all[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        all[k] = dag_quad_bcast<0>(m[k]);
        all[4 + k] = dag_quad_bcast<1>(m[k]);
        all[8 + k] = dag_quad_bcast<2>(m[k]);
        all[12 + k] = dag_quad_bcast<3>(m[k]);
    }
    uint64_t in[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = ((uint64_t)all[2 * k + 1] << 32) | all[2 * k];
    keccak512_64(in, out);
    const uint64_t lo = (s & 2) ? ((s & 1) ? out[6] : out[4]) : ((s & 1) ? out[2] : out[0]);
    const uint64_t hi = (s & 2) ? ((s & 1) ? out[7] : out[5]) : ((s & 1) ? out[3] : out[1]);
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
