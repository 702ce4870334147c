// Signature hashes of every form on gfx950: legacy ALL / NONE / SINGLE with and
// without ANYONECANPAY, and witness v0 (BIP143).
//
// sighash_gather_var: one lane per signature, as sighash_gather_batch (sighash.hip), but the message
// is the concatenation of 0 to SIGHASH_VAR_MAX_SEGMENTS byte ranges of the shared arena, named
// through a segment table (kernel_params.h SighashSeg / SighashVarJob; csrc/chain/sighash.cpp lays
// the forms out). Any segment may be empty; a job without bytes hashes the empty string. The digest
// is SHA256d in the byte order of CHash256 and goes out as raw bytes and / or into the z limbs of
// the SecpVerifyJob that secp_verify_batch reads next on the same stream.
//
// The rules are the sibling's: a 64-byte block inside one segment is read as 17 aligned dwords and
// realigned in registers, a word inside one segment as 2, and only a word that straddles a segment
// boundary or the message end is assembled byte by byte. SIGHASH_ARENA_SLACK readable bytes follow
// the arena; no byte outside a job's segments reaches the hash.
//
// The read position and the one descriptor held ahead live in named registers; the descriptor
// after it is fetched from the table when a segment is entered, so nothing is indexed at run time.
// Lanes of a wave differ in segment count and lengths (jobs come in block order, forms mixed):
// every lane walks its own stream, and a lane whose message is over simply leaves the block loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_params.h"
#include "sha256_device.hpp"

namespace {

// Read position in the gathered message: `rem` bytes left in the current segment from arena offset
// `pos`; `ahead` segments not entered yet, the first of them being (no, nl) and the one after it
// *next. Kept normalised: rem > 0 unless the message is over (then ahead == 0 too).
struct SvStream {
    uint32_t pos, rem, ahead;
    uint32_t no, nl;
    const SighashSeg* next;
};

__device__ __forceinline__ void sv_normalise(SvStream& st) {
    while (st.rem == 0 && st.ahead != 0) {
        st.pos = st.no;
        st.rem = st.nl;
        if (--st.ahead != 0) {
            const SighashSeg s = *st.next++;
            st.no = s.off;
            st.nl = s.len;
        }
    }
}

// The aligned dword pair around arena byte `pos`, shifted so that the byte comes first.
__device__ __forceinline__ uint32_t sv_load_be32(const uint8_t* arena, uint32_t pos) {
    const uint8_t* p = arena + pos;
    const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(p - mis);
    return __builtin_bswap32(__builtin_amdgcn_alignbyte(a[1], a[0], mis));
}

// Next message word (big-endian). `pad` is the padding byte still owed: 0x80 until it is emitted.
__device__ __forceinline__ uint32_t sv_word(const uint8_t* arena, SvStream& st, uint32_t& pad) {
    if (st.rem >= 4) {
        const uint32_t w = sv_load_be32(arena, st.pos);
        st.pos += 4;
        st.rem -= 4;
        sv_normalise(st);
        return w;
    }
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t byte;
        if (st.rem != 0) {
            byte = arena[st.pos];
            ++st.pos;
            --st.rem;
            sv_normalise(st);
        } else {
            byte = pad;
            pad = 0;
        }
        w = (w << 8) | byte;
    }
    return w;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void sighash_gather_var(SighashVarParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const SighashVarJob job = p.jobs[i];
    const uint8_t* arena = p.arena;
    // first_seg + n_seg <= n_segs, n_seg <= SIGHASH_VAR_MAX_SEGMENTS and the message length < 2^29:
    // checked on the host (sighash_var_check)
    const SighashSeg* tab = p.segs + job.first_seg;
    uint32_t len = 0;
    for (uint32_t s = 0; s < job.n_seg; ++s) len += tab[s].len;
    SvStream st;
    st.pos = 0;
    st.rem = 0;
    st.ahead = job.n_seg;
    st.no = 0;
    st.nl = 0;
    st.next = tab;
    if (st.ahead != 0) {
        const SighashSeg s = *st.next++;
        st.no = s.off;
        st.nl = s.len;
    }
    sv_normalise(st);
    const uint32_t nblocks = (len + 9 + 63) / 64;
    uint32_t pad = 0x80u;
    uint32_t s1[8];
    sha256_init(s1);
    for (uint32_t b = 0; b < nblocks; ++b) {
        uint32_t w[16];
        if (st.rem >= 64) {
            const uint8_t* q = arena + st.pos;
            const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(q) & 3);
            const uint32_t* a = reinterpret_cast<const uint32_t*>(q - mis);
            uint32_t d[17];
#pragma unroll
            for (int k = 0; k < 17; ++k) d[k] = a[k];
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = __builtin_bswap32(__builtin_amdgcn_alignbyte(d[j + 1], d[j], mis));
            st.pos += 64;
            st.rem -= 64;
            sv_normalise(st);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = sv_word(arena, st, pad);
        }
        if (b == nblocks - 1) {
            w[14] = len >> 29;
            w[15] = len << 3;
        }
        sha256_compress(s1, w);
    }
    uint32_t s2[8];
    sha256_of_digest(s1, s2);
    if (p.digests) store_digest(p.digests + size_t(job.out_index) * 32, s2);
    if (p.secp_jobs) {
        // pack_verify_job's z: the digest as a 256-bit big-endian integer in little-endian limbs
        SecpVerifyJob* sj = p.secp_jobs + job.out_index;
#pragma unroll
        for (int k = 0; k < 8; ++k) sj->z[k] = s2[7 - k];
        sj->kind = job.kind;
    }
}
