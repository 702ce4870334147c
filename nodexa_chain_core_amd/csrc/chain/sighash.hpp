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

// ---- every form of both signature versions (hip/kernels/sighash_var.hip)
//
// connect_block with defer_all_forms leaves out every message hash but the legacy constant one.
// pack_sighash_var lays them out over one arena and a segment table, at most
// SIGHASH_VAR_MAX_SEGMENTS ranges per signature. Placed once per transaction, and only when one of
// its signatures needs it: the template T, and Z, the head of T up to the outputs with every
// sequence zeroed (NONE / SINGLE). Placed once per arena: SINGLE's run of blanked outputs
// (ff x 8, 00), of which input i uses the first 9 i bytes. Per signature (| joins the segments;
// e = emitted code, seq = the input's sequence, lt = lock time, ht = hash type, all little-endian):
//   all         T[:off] | e | T[off+1:] | ht
//   none        Z[:off] | e seq | Z[off+5:] | 00 lt ht
//   single      Z[:off] | e seq | Z[off+5:] | cs(i+1) | blank[:9i] | T[output i] | lt ht
//   all|acp     version 01 | T[prevout i] | e seq | T[outputs, lt] | ht
//   none|acp    version 01 | T[prevout i] | e seq 00 lt ht
//   single|acp  version 01 | T[prevout i] | e seq cs(i+1) | blank[:9i] | T[output i] | lt ht
//   witness v0  the whole BIP143 preimage (e + 156 bytes; the three midstate hashes are the
//               transaction's PrecomputedTx, SINGLE's output hash is computed here) as one segment
// so a legacy signature adds at most len(e) + 22 bytes to the arena and the arena stays linear in
// the block size.
struct SighashVarPack {
    Bytes arena;
    std::vector<SighashSeg> segs;
    std::vector<SighashVarJob> jobs;       // block order
    std::vector<SecpVerifyJob> secp_jobs;  // as SighashPack's: device-hashed records INVALID with z = 0
    size_t device_jobs = 0, host_jobs = 0;
    size_t device_v0 = 0, device_partial = 0;  // of device_jobs: witness v0, legacy other than the ALL form
};
SighashVarPack pack_sighash_var(const ConnectResult& res);

// Throws std::invalid_argument on a segment outside [0, arena_len) (32-bit wrap included), a job
// whose first_seg + n_seg passes the table, n_seg > SIGHASH_VAR_MAX_SEGMENTS, a message of 2^29
// bytes or more, or an out_index >= n_out.
void sighash_var_check(size_t arena_len, const SighashSeg* segs, size_t n_segs, const SighashVarJob* jobs, size_t n,
                       size_t n_out);

// The definition of sighash_gather_var: digest k = SHA256d of job k's segments in order, 32 raw
// bytes each, in job order.
Bytes sighash_var_model(const Bytes& arena, const SighashSeg* segs, size_t n_segs, const SighashVarJob* jobs, size_t n);

// ---- a window of consecutive blocks as one batch (-gpusigwindow; hip/kernels/sig_window.hip)
//
// pack_sig_window runs every result through the packer of its mode and concatenates the outputs:
// arena offsets move by the block's arena base, first_seg by its segment base, out_index by its
// signature base, so the tables are what sighash_gather_batch / sighash_gather_var and
// secp_verify_batch take for a single block. Block b owns signatures [sig_begin[b], sig_begin[b+1]).
enum class SigWindowMode { HOST_HASH = 0, LEGACY_ALL = 1, ALL_FORMS = 2 };
// HOST_HASH: connected with defer_sigs alone; LEGACY_ALL: with defer_sighash; ALL_FORMS: with
// defer_all_forms. A result without signatures takes part in a window of any mode.
SigWindowMode sig_window_mode(const ConnectResult& res);
// Offsets are 32-bit: a window whose arena plus SIGHASH_ARENA_SLACK would reach 2^31 bytes is refused.
constexpr u64 SIG_WINDOW_ARENA_LIMIT = (u64(1) << 31) - SIGHASH_ARENA_SLACK;
struct SigWindowPack {
    SigWindowMode mode = SigWindowMode::HOST_HASH;  // of the results that have signatures
    Bytes arena;
    std::vector<SighashSeg> segs;          // ALL_FORMS
    std::vector<SighashJob> jobs;          // LEGACY_ALL
    std::vector<SighashVarJob> var_jobs;   // ALL_FORMS
    std::vector<SecpVerifyJob> secp_jobs;
    std::vector<u32> sig_begin;            // results.size() + 1
    size_t device_jobs = 0, host_jobs = 0;
};
// Throws std::invalid_argument on results of different modes, std::length_error on an arena that
// reaches `arena_limit` bytes (lower than the real limit only in tests).
SigWindowPack pack_sig_window(const std::vector<const ConnectResult*>& results,
                              u64 arena_limit = SIG_WINDOW_ARENA_LIMIT);

// The definition of sig_window_verdicts: one SigWindowRecord per block over the verifier's
// verdicts. Throws std::invalid_argument on a prefix table that decreases or passes n.
std::vector<SigWindowRecord> sig_window_verdicts_model(const u32* verdicts, size_t n, const u32* sig_begin, size_t nb);

// ---- CHECKMULTISIG groups (-gpumultisig; hip/kernels/sig_group.hip)
//
// connect_block with defer_multisig records every candidate pair of a CHECKMULTISIG as entries of
// ConnectResult::sigs and one SigGroupRec (interpreter.hpp). The packers above treat those entries
// like any other; consecutive entries of one group that sign with the same hash type name the same
// arena ranges (and segments), so the arena grows per group, not per pair.
//
// The group table of one result, and of a window (each `first` moved by its block's signature
// base, the prefix pack_sig_window reports as sig_begin).
std::vector<SigGroup> sig_group_table(const ConnectResult& res);
std::vector<SigGroup> sig_window_groups(const std::vector<const ConnectResult*>& results);
// Throws std::invalid_argument on a group with n_sigs = 0, n_sigs > n_keys, n_keys > 20, more than
// SIG_GROUP_MAX_PAIRS pairs or entries past n_verdicts, and on groups that overlap or descend.
void sig_group_check(size_t n_verdicts, const SigGroup* groups, size_t ng);
// The definition of sig_group_resolve, in place. Per group, m = n_sigs, n = n_keys, w = n - m + 1:
//   a = b = 0
//   while a < m:  v = verdicts[first + a * w + (b - a)]
//                 v == 2: ASK, stop;  v == 1: a += 1;  b += 1;  m - a > n - b: FAIL, stop
//   else OK
// which is CHECKMULTISIG's own loop (a verdict other than 1 or 2 is a failed check); the entries
// the walk never reads do not matter. All m * w entries become 1 (OK), 0 (FAIL) or 2 (ASK: the
// host decides); entries outside groups are untouched. Checks the table first.
void sig_group_resolve_model(u32* verdicts, size_t n_verdicts, const SigGroup* groups, size_t ng);

}  // namespace nodexa
