// Test probe kernel: one thread per record through the op switch of secp256k1_probe.hpp, the
// device build of the limb arithmetic the batch verifier (secp256k1_verify.hip) runs. The host
// runs the same switch (_core.secp32_probe); tests/test_secp_edges.py requires both to give the
// same bytes and those to equal Python integers. Launched with the generic Kernel.launch:
// grid (ceil(n / 64), 1, 1), block (64, 1, 1), parameters SecpProbeParams.
#include "secp256k1_probe.hpp"

extern "C" __global__ __launch_bounds__(64) void secp_probe(SecpProbeParams p) {
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    if (idx >= p.n) return;
    secp32::probe_record(p.op, p.in + (size_t)idx * SECP_PROBE_IN_WORDS, p.out + (size_t)idx * SECP_PROBE_OUT_WORDS);
}
