// Per-block verdicts of a signature window on gfx950.
//
// With -gpusigwindow the signatures of a run of consecutive blocks are verified by one
// secp_verify_batch launch. sig_window_verdicts follows it on the same stream and turns the
// verifier's out[] into one 16-byte SigWindowRecord per block (kernel_params.h), so that the host
// downloads and scans 16 bytes per block instead of 4 per signature; it fetches a block's slice of
// out[] only when the record shows something other than valid.
//
// One wave64 per block: the lanes stride over the block's signatures (none, or tens of
// thousands), each keeping three counts and the lowest index that is not valid, then a butterfly
// of cross-lane exchanges folds the 64 partial results (sums, and a minimum for the index). No
// atomics, no LDS allocation; every lane ends with the same totals, whatever the order, and lane 0
// writes the record with one 16-byte store. csrc/chain/sighash.cpp sig_window_verdicts_model is
// the definition.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_params.h"

extern "C" __global__ __launch_bounds__(256) void sig_window_verdicts(SigWindowParams p) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);  // uniform over the wave
    if (b >= p.nb) return;
    const uint32_t begin = p.sig_begin[b], end = p.sig_begin[b + 1];
    uint32_t valid = 0, invalid = 0, ask = 0, first = SIG_WINDOW_NONE;
    for (uint32_t i = begin + lane; i < end; i += 64u) {
        const uint32_t v = p.verdicts[i];
        valid += v == 1u;
        ask += v == 2u;
        invalid += v != 1u && v != 2u;
        if (v != 1u) first = min(first, i - begin);  // i grows: only the first hit lowers it
        if (end - i <= 64u) break;                   // i + 64 may wrap past 2^32
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        valid += __shfl_xor(valid, m, 64);
        invalid += __shfl_xor(invalid, m, 64);
        ask += __shfl_xor(ask, m, 64);
        first = min(first, uint32_t(__shfl_xor(first, m, 64)));
    }
    if (lane == 0) reinterpret_cast<uint4*>(p.records)[b] = make_uint4(valid, invalid, ask, first);
}
