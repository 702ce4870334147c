// Packing a block's deferred legacy signature hashes for the GPU (hip/kernels/sighash.hip) and
// the host model of that kernel.
//
// connect_block with defer_sighash leaves the message of every sighash_all_form signature
// (interpreter.hpp) uncomputed. pack_sighash lays the block out as one byte arena: the template of
// each transaction that has such a signature once, then per signature its emitted script code and
// its hash type; a SighashJob names the four ranges whose concatenation is the preimage. The arena
// is linear in the block size, where hashing on the host re-serialises the transaction per input.
#pragma once
#include <vector>

#include "../../hip/kernels/kernel_params.h"
#include "coins.hpp"

namespace nodexa {

struct SighashPack {
    Bytes arena;
    std::vector<SighashJob> jobs;          // block order (the order of ConnectResult::sigs)
    // One record per entry of ConnectResult::sigs. A signature whose hash is a job above has
    // kind = SECP_KIND_INVALID and z = 0 until the kernel writes both: a record the kernel never
    // reached verifies as 0 and goes to the host re-check (a known constant z would be forgeable).
    std::vector<SecpVerifyJob> secp_jobs;
    size_t device_jobs = 0, host_jobs = 0;
};

SighashPack pack_sighash(const ConnectResult& res);

// Throws std::invalid_argument on a segment outside [0, arena_len) or an out_index >= n_out.
void sighash_check_jobs(size_t arena_len, const SighashJob* jobs, size_t n, size_t n_out);

// The definition of sighash_gather_batch: digest k = SHA256d of job k's four segments in order,
// 32 raw bytes each, in job order.
Bytes sighash_gather_model(const Bytes& arena, const SighashJob* jobs, size_t n);

}  // namespace nodexa
