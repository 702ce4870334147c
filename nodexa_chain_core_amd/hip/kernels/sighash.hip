// Legacy signature hashes on gfx950 (block validation's message hashes).
//
// sighash_gather_batch: one lane per signature. The message is the concatenation of four byte
// ranges of one shared arena (kernel_params.h SighashJob; csrc/chain/sighash.cpp builds them):
//   T[0:off_i] | compact size + script code | T[off_i+1:] | hash type (LE int32)
// where T is the transaction's legacy serialisation with every input script empty, stored once
// per transaction. The digest is SHA256d in the byte order of CHash256 (SignatureHash,
// src/script/interpreter.cpp), and goes out as raw bytes and / or straight into the z limbs of
// the SecpVerifyJob that secp_verify_batch reads next on the same stream.
//
// The host re-serialises and hashes the whole transaction once per input (quadratic in the input
// count); here the arena is linear in the block size and the lanes of a wave that hash the inputs
// of one transaction (jobs come in block order) read the same template lines.
//
// A 64-byte block that lies inside one segment is read as 17 aligned dwords and realigned in
// registers (v_alignbyte + byte swap), a word inside one segment as 2; only a word that straddles
// a segment boundary or the message end is assembled byte by byte. The host keeps
// SIGHASH_ARENA_SLACK readable bytes after the arena, so an aligned dword pair that holds an arena
// byte is always readable; no byte outside a job's segments reaches the hash.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernel_params.h"
#include "sha256_device.hpp"

namespace {

// Read position in the gathered message: segment `seg` (SIGHASH_SEGMENTS = past the end), `rem`
// bytes left in it from arena offset `pos`. Kept normalised: rem > 0 unless the message is over.
struct SgStream {
    uint32_t pos, rem, seg;
    uint32_t o1, l1, o2, l2, o3, l3;  // the segments still ahead, shifted down as they are entered
};

__device__ __forceinline__ void sg_normalise(SgStream& st) {
#pragma unroll
    for (int k = 0; k < SIGHASH_SEGMENTS; ++k) {
        if (st.rem == 0 && st.seg < SIGHASH_SEGMENTS) {
            ++st.seg;
            st.pos = st.o1; st.rem = st.l1;
            st.o1 = st.o2; st.l1 = st.l2;
            st.o2 = st.o3; st.l2 = st.l3;
            st.l3 = 0;
        }
    }
}

// The aligned dword pair around arena byte `pos`, shifted so that the byte comes first.
__device__ __forceinline__ uint32_t sg_load_be32(const uint8_t* arena, uint32_t pos) {
    const uint8_t* p = arena + pos;
    const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(p) & 3);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(p - mis);
    return __builtin_bswap32(__builtin_amdgcn_alignbyte(a[1], a[0], mis));
}

// Next message word (big-endian). `pad` is the padding byte still owed: 0x80 until it is emitted.
__device__ __forceinline__ uint32_t sg_word(const uint8_t* arena, SgStream& st, uint32_t& pad) {
    if (st.rem >= 4) {
        const uint32_t w = sg_load_be32(arena, st.pos);
        st.pos += 4;
        st.rem -= 4;
        sg_normalise(st);
        return w;
    }
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t byte;
        if (st.seg < SIGHASH_SEGMENTS) {
            byte = arena[st.pos];
            ++st.pos;
            --st.rem;
            sg_normalise(st);
        } else {
            byte = pad;
            pad = 0;
        }
        w = (w << 8) | byte;
    }
    return w;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void sighash_gather_batch(SighashParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n) return;
    const SighashJob job = p.jobs[i];
    const uint8_t* arena = p.arena;
    SgStream st;
    st.pos = job.off[0];
    st.rem = job.len[0];
    st.seg = 0;
    st.o1 = job.off[1]; st.l1 = job.len[1];
    st.o2 = job.off[2]; st.l2 = job.len[2];
    st.o3 = job.off[3]; st.l3 = job.len[3];
    sg_normalise(st);
    const uint32_t len = job.len[0] + job.len[1] + job.len[2] + job.len[3];  // < 2^29: checked on the host
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
            sg_normalise(st);
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) w[j] = sg_word(arena, st, pad);
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
