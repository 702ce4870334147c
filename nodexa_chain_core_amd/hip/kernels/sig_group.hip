// CHECKMULTISIG pairings of a signature batch on gfx950.
//
// With -gpumultisig a CHECKMULTISIG leaves every (signature, key) pair its walk can reach in the
// batch, m * w entries for m signatures and n keys (w = n - m + 1), and one SigGroup record
// (kernel_params.h). sig_group_resolve follows secp_verify_batch on the same stream, before
// sig_window_verdicts: it runs the interpreter's walk over the group's verdicts and rewrites all
// of them to the outcome, so that everything downstream sees "every entry valid" exactly when the
// opcode succeeds, whichever keys signed.
//
// One lane per group: the walk is at most 20 dependent dword reads and the rewrite at most
// SIG_GROUP_MAX_PAIRS dword stores, and a window holds thousands of groups. No LDS, no atomics.
// The host has checked the table (csrc/chain/sighash.cpp sig_group_check): every group lies inside
// the verdicts, 1 <= m <= n <= 20, m * w <= SIG_GROUP_MAX_PAIRS, groups disjoint, so no two lanes
// touch the same entry. sig_group_resolve_model there is the definition.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_params.h"

extern "C" __global__ __launch_bounds__(256) void sig_group_resolve(SigGroupParams p) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= p.ng) return;
    const uint4 rec = reinterpret_cast<const uint4*>(p.groups)[g];
    const uint32_t m = rec.y, n = rec.z, w = n - m + 1u;
    uint32_t* v = p.verdicts + rec.x;
    uint32_t a = 0, b = 0, outcome = 1u;
    while (a < m) {
        const uint32_t x = v[a * w + (b - a)];  // 0 <= b - a < w: the stop rule below keeps it
        if (x == 2u) {
            outcome = 2u;
            break;
        }
        if (x == 1u) ++a;
        ++b;
        if (m - a > n - b) {
            outcome = 0u;
            break;
        }
    }
    const uint32_t pairs = m * w;
    for (uint32_t i = 0; i < pairs; ++i) v[i] = outcome;
}
