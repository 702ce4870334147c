// Integrity checks of a resident Ethash DAG on gfx950: a position-keyed digest per 1 MiB chunk and an
// audit that recomputes items from the light cache, compares and optionally repairs them.
//
// Digest (the definition is csrc/pow/ethash.cpp dag_digest, the host model): for u32 word w at global
// word index g, x = w ^ g * 0x9E3779B1 and two bijective mixes a(x), b(x) are summed mod 2^32 over the
// chunk's words. The sums commute, so lanes accumulate in any order, the result is deterministic and
// needs no atomics. It is a pure streaming read: one 256-thread workgroup per chunk, consecutive lanes
// on consecutive 16 bytes, DG_UNROLL 16-byte loads in flight per lane (32 KiB per workgroup, and a
// 1 GiB DAG gives every CU four workgroups), ~20 integer operations per 16 bytes.
//
// Audit: one item per aligned lane quad exactly as the build computes it (ethash_dag_device.hpp);
// lane s compares its bytes 16s..16s+15 of the resident item. Mismatches are the rare path and use
// ordinary global atomics.
#include "ethash_dag_device.hpp"

#define DG_BLOCK 256
#define DG_UNROLL 8

NX_DEV void dg_mix(uint32_t w, uint32_t g, uint32_t& A, uint32_t& B) {
    const uint32_t x = w ^ (g * 0x9E3779B1u);
    uint32_t a = x * 0x85EBCA6Bu;
    a ^= a >> 13;
    a *= 0xC2B2AE35u;
    a ^= a >> 16;
    uint32_t b = (x ^ 0xA5A5A5A5u) * 0x27D4EB2Fu;
    b ^= b >> 15;
    b *= 0x165667B1u;
    b ^= b >> 13;
    A += a;
    B += b;
}

typedef uint32_t dg_u32x4 __attribute__((ext_vector_type(4)));

// read once and never again soon: keep the stream out of the way of the search's cached DAG lines
NX_DEV uint4 dg_load(const uint4* p) {
    const dg_u32x4 v = __builtin_nontemporal_load((const dg_u32x4*)p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// q: global index of the 16-byte piece (4 per item), so its first word is g = 4 q
NX_DEV void dg_mix4(const uint4 v, uint64_t q, uint32_t& A, uint32_t& B) {
    const uint32_t g = (uint32_t)q * 4u;
    dg_mix(v.x, g, A, B);
    dg_mix(v.y, g + 1, A, B);
    dg_mix(v.z, g + 2, A, B);
    dg_mix(v.w, g + 3, A, B);
}

extern "C" __global__ __launch_bounds__(DG_BLOCK) void ethash_dag_digest(EthashDagDigestParams p) {
    __shared__ uint32_t part[2 * (DG_BLOCK / 64)];
    const uint64_t end = p.first_item + p.num_items;
    const uint64_t chunk = p.first_item / p.chunk_items + blockIdx.x;
    const uint64_t c_lo = chunk * p.chunk_items, c_hi = c_lo + p.chunk_items;
    const uint64_t lo = c_lo > p.first_item ? c_lo : p.first_item;
    const uint64_t hi = c_hi < end ? c_hi : end;
    const uint4* __restrict__ dag = (const uint4*)p.dag;

    uint32_t A = 0, B = 0;
    const uint64_t q_end = hi * 4;  // lo >= hi (the host launches no such workgroup) reads nothing
    uint64_t q = lo * 4 + threadIdx.x;
    for (; q + (DG_UNROLL - 1) * DG_BLOCK < q_end; q += DG_UNROLL * DG_BLOCK) {
        uint4 v[DG_UNROLL];
#pragma unroll
        for (int u = 0; u < DG_UNROLL; ++u) v[u] = dg_load(&dag[q + u * DG_BLOCK]);
#pragma unroll
        for (int u = 0; u < DG_UNROLL; ++u) dg_mix4(v[u], q + u * DG_BLOCK, A, B);
    }
    for (; q < q_end; q += DG_BLOCK) dg_mix4(dg_load(&dag[q]), q, A, B);

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        A += __shfl_xor(A, off);
        B += __shfl_xor(B, off);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[2 * wave] = A;
        part[2 * wave + 1] = B;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (int w = 0; w < DG_BLOCK / 64; ++w) {
            a += part[2 * w];
            b += part[2 * w + 1];
        }
        p.table[blockIdx.x] = ((uint64_t)b << 32) | a;
    }
}

// 64 items per 256-thread workgroup; the host launches ceil(count / 64) workgroups
extern "C" __global__ __launch_bounds__(256) void ethash_dag_audit(EthashDagAuditParams p, FastMod32 lmod) {
    const uint64_t k = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    if (threadIdx.x == 0) {  // items of this workgroup, counted once
        const uint64_t left = p.count - (uint64_t)blockIdx.x * 64;
        atomicAdd(&p.out[3], left < 64 ? (uint32_t)left : 64u);
    }
    if (k >= p.count) return;  // whole quads: the quad's lanes share `k`
    const uint32_t s = threadIdx.x & 3;
    const uint64_t index = p.first_item + k * p.stride;
    uint4* slot = (uint4*)p.dag + index * 4 + s;
    const uint4 have = *slot;  // issued ahead of the recomputation
    const uint4 want = dag_item_quad(p.light, lmod, index, s);
    const uint32_t diff = ((have.x ^ want.x) | (have.y ^ want.y) | (have.z ^ want.z) | (have.w ^ want.w)) != 0;
    const uint32_t any = dag_quad_bcast<0>(diff) | dag_quad_bcast<1>(diff) | dag_quad_bcast<2>(diff) |
                         dag_quad_bcast<3>(diff);
    if (!any) return;
    if (p.repair && diff) *slot = want;
    if (s == 0) {
        atomicAdd(&p.out[0], 1u);
        atomicMin(&p.out[1], (uint32_t)index);
        if (p.repair) atomicAdd(&p.out[2], 1u);
    }
}
