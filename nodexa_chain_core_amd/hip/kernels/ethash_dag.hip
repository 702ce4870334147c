// Ethash dataset (DAG) generation on gfx950.
//
// Each 512-bit item (src/crypto/ethash/lib/ethash/ethash.cpp:180-207):
//   mix = keccak512(light[i % n] with word0 ^= i)
//   512 x { parent = fnv1(i ^ j, mix[j % 16]) % n ; mix = fnv1(mix, light[parent]) }
//   item = keccak512(mix)
// The light cache (16 MiB at epoch 0 .. 64 MiB at epoch 384) stays resident in the 256 MiB
// Infinity Cache, and the build is bound by its rate for random 64-byte reads.
//
// CDNA4 mapping: one item per aligned lane quad. Lane s of the quad owns mix words 4s..4s+3 and
// reads its 16 bytes of every parent, so a wave-wide parent load is one 16-byte load per lane
// touching 16 lines, each read whole by its quad (a thread-per-item layout needs four 16-byte
// loads per lane touching 64 lines each for the same bytes). The parent index word mix[j % 16]
// lives in quad lane (j % 16) / 4 and reaches the other three by a DPP quad_perm broadcast (j % 16
// is a literal after unrolling by 16). Each lane runs the two keccak512s itself: VALU the build
// has to spare. tools/dag_build_probe.hip (profiles/r6m_rehearsal): 3.80 TB/s of parent reads at
// epoch 384 against 3.46 for thread-per-item, i.e. the measured ceiling for independent random
// 64-byte reads of a 64 MiB buffer (3.68 TB/s); 4 GiB in 0.578 s instead of 0.636.
#include "ethash_dag_device.hpp"  // the per-item computation, shared with the audit kernel

// 64 items per 256-thread workgroup; the host launches ceil(num_items / 64) workgroups
extern "C" __global__ __launch_bounds__(256) void ethash_dag_build(EthashDagParams p, FastMod32 lmod) {
    const uint64_t local = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
    if (local >= p.num_items) return;  // whole quads: the quad's lanes share `local`
    const uint32_t s = threadIdx.x & 3;
    const uint64_t index = p.first_item + local;
    // absolute item index: shards build in place
    ((uint4*)p.dag)[index * 4 + s] = dag_item_quad(p.light, lmod, index, s);
}
