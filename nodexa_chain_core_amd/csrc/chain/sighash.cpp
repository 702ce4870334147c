#include "sighash.hpp"

#include <cstring>
#include <stdexcept>
#include <string>

#include "../crypto/secp256k1_model32.hpp"
#include "../crypto/sha256.hpp"

namespace nodexa {

SighashPack pack_sighash(const ConnectResult& res) {
    SighashPack out;
    out.secp_jobs.resize(res.sigs.size());
    std::vector<int64_t> tmpl_at(res.templates.size(), -1);  // arena offset of each template placed
    static const u8 kZero[32] = {};
    for (size_t k = 0; k < res.sigs.size(); ++k) {
        const PendingSig& p = res.sigs[k];
        SecpVerifyJob& sj = out.secp_jobs[k];
        if (!p.device_hash) {
            secp::pack_verify_job(p.pubkey.data(), p.pubkey.size(), p.sig.data(), p.sig.size(), p.msg.data, sj);
            ++out.host_jobs;
            continue;
        }
        secp::pack_verify_job(p.pubkey.data(), p.pubkey.size(), p.sig.data(), p.sig.size(), kZero, sj);
        const SighashTemplate& t = *res.templates.at(p.tx_index);
        if (tmpl_at[p.tx_index] < 0) {
            tmpl_at[p.tx_index] = int64_t(out.arena.size());
            out.arena.insert(out.arena.end(), t.bytes.begin(), t.bytes.end());
        }
        const size_t base = size_t(tmpl_at[p.tx_index]), off = t.script_off.at(p.n_in);
        const size_t code_at = out.arena.size();
        out.arena.insert(out.arena.end(), p.code.begin(), p.code.end());
        u8 ht[4];
        store_le32(ht, u32(p.hash_type));
        out.arena.insert(out.arena.end(), ht, ht + 4);
        if (out.arena.size() > 0xffffffffULL) throw std::length_error("sighash arena exceeds 4 GiB");
        SighashJob j{};
        j.off[0] = u32(base);
        j.len[0] = u32(off);
        j.off[1] = u32(code_at);
        j.len[1] = u32(p.code.size());
        j.off[2] = u32(base + off + 1);
        j.len[2] = u32(t.bytes.size() - off - 1);
        j.off[3] = u32(code_at + p.code.size());
        j.len[3] = 4;
        j.out_index = u32(k);
        j.kind = sj.kind;  // INVALID stays INVALID: host parsing already failed
        sj.kind = SECP_KIND_INVALID;
        out.jobs.push_back(j);
        ++out.device_jobs;
    }
    return out;
}

void sighash_check_jobs(size_t arena_len, const SighashJob* jobs, size_t n, size_t n_out) {
    for (size_t k = 0; k < n; ++k) {
        u64 total = 0;
        for (int s = 0; s < SIGHASH_SEGMENTS; ++s) {
            if (u64(jobs[k].off[s]) + jobs[k].len[s] > arena_len)
                throw std::invalid_argument("sighash job " + std::to_string(k) + ": segment " + std::to_string(s) +
                                            " lies outside the arena");
            total += jobs[k].len[s];
        }
        if (total >= (1u << 29)) throw std::invalid_argument("sighash job " + std::to_string(k) + ": message too long");
        if (jobs[k].out_index >= n_out)
            throw std::invalid_argument("sighash job " + std::to_string(k) + ": output index out of range");
    }
}

Bytes sighash_gather_model(const Bytes& arena, const SighashJob* jobs, size_t n) {
    sighash_check_jobs(arena.size(), jobs, n, size_t(-1));
    Bytes out(n * 32);
    Bytes msg;
    for (size_t k = 0; k < n; ++k) {
        msg.clear();
        for (int s = 0; s < SIGHASH_SEGMENTS; ++s)
            msg.insert(msg.end(), arena.begin() + jobs[k].off[s], arena.begin() + jobs[k].off[s] + jobs[k].len[s]);
        sha256d(msg.data(), msg.size(), &out[k * 32]);
    }
    return out;
}

}  // namespace nodexa
