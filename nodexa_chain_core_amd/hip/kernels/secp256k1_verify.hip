// Batch ECDSA verification on gfx950 (new; the reference verifies every signature serially on
// the CPU: CPubKey::Verify, src/pubkey.cpp:169, called from the script-check worker pool
// CCheckQueue, src/checkqueue.h:33-160, src/validation.cpp:9949). One thread per signature;
// arithmetic in secp256k1_device.hpp (host-testable, see csrc/crypto/secp256k1_model32.cpp).
//
// Per signature: public-key decompression (one sqrt chain), s^-1 mod n, u2*Q by a 2-bit window
// over affine {Q, 2Q, 3Q} (one batch inversion), u1*G by 64 mixed additions from a 64 KiB comb
// table that every thread reads (it stays in L1/L2), and the x(R) == r check in Jacobian
// coordinates. Work is the same for every lane (no data-dependent branches but the rare
// degenerate-addition flag), so waves do not diverge.
#include "kernel_params.h"
#include "secp256k1_device.hpp"

using namespace secp32;

extern "C" __global__ __launch_bounds__(256) void secp_verify_batch(SecpVerifyParams p) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= p.n) return;
    p.out[idx] = verify_job32(p.jobs[idx], (const A*)p.gtab);  // secp256k1_device.hpp, shared with the host model
}
