#include "sighash.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../crypto/secp256k1_model32.hpp"
#include "../crypto/sha256.hpp"

namespace nodexa {

namespace {

// Whether entry k of res.sigs has the message of entry k - 1, asked for ascending k: both belong to
// one CHECKMULTISIG group (same input, same script code) and sign with the same hash type, and
// both hashes are left to the device. Such entries name the same arena ranges.
class SameMessage {
public:
    explicit SameMessage(const ConnectResult& res) : res_(res) {}
    bool operator()(size_t k) {
        const std::vector<SigGroupRec>& g = res_.sig_groups;
        while (gi_ < g.size() && k >= size_t(g[gi_].first) + pairs(g[gi_])) ++gi_;
        if (gi_ == g.size() || k <= g[gi_].first) return false;
        const PendingSig &p = res_.sigs[k], &q = res_.sigs[k - 1];
        return p.device_hash && q.device_hash && p.hash_type == q.hash_type;
    }

private:
    static size_t pairs(const SigGroupRec& g) { return size_t(g.n_sigs) * (g.n_keys - g.n_sigs + 1); }
    const ConnectResult& res_;
    size_t gi_ = 0;
};

}  // namespace

SighashPack pack_sighash(const ConnectResult& res) {
    // four fixed segments express the legacy ALL form only
    if (res.all_forms) throw std::invalid_argument("pack_sighash: the block was connected with defer_all_forms");
    SighashPack out;
    out.secp_jobs.resize(res.sigs.size());
    std::vector<int64_t> tmpl_at(res.templates.size(), -1);  // arena offset of each template placed
    static const u8 kZero[32] = {};
    SameMessage same_message(res);
    for (size_t k = 0; k < res.sigs.size(); ++k) {
        const PendingSig& p = res.sigs[k];
        SecpVerifyJob& sj = out.secp_jobs[k];
        if (!p.device_hash) {
            secp::pack_verify_job(p.pubkey.data(), p.pubkey.size(), p.sig.data(), p.sig.size(), p.msg.data, sj);
            ++out.host_jobs;
            continue;
        }
        secp::pack_verify_job(p.pubkey.data(), p.pubkey.size(), p.sig.data(), p.sig.size(), kZero, sj);
        if (same_message(k)) {  // another key against the message of the entry before: its ranges
            SighashJob j = out.jobs.back();
            j.out_index = u32(k);
            j.kind = sj.kind;
            sj.kind = SECP_KIND_INVALID;
            out.jobs.push_back(j);
            ++out.device_jobs;
            continue;
        }
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

SighashVarPack pack_sighash_var(const ConnectResult& res) {
    SighashVarPack out;
    out.secp_jobs.resize(res.sigs.size());
    Bytes& A = out.arena;
    static const u8 kZero[32] = {};
    // SINGLE's blanked outputs, once: as long as the furthest legacy SINGLE input needs
    size_t blank_n = 0;
    for (const PendingSig& p : res.sigs)
        if (p.device_hash && p.sigversion == SigVersion::BASE && (p.hash_type & 0x1f) == SIGHASH_SINGLE)
            blank_n = std::max<size_t>(blank_n, p.n_in);
    for (size_t k = 0; k < blank_n; ++k) {
        A.insert(A.end(), 8, 0xff);
        A.push_back(0);
    }
    std::vector<int64_t> t_at(res.forms.size(), -1), z_at(res.forms.size(), -1);
    auto put = [&](const u8* p, size_t n) { A.insert(A.end(), p, p + n); };
    auto put_le32 = [&](u32 v) {
        u8 b[4];
        store_le32(b, v);
        put(b, 4);
    };
    auto put_cs = [&](u64 n) {  // compact size (n < 2^32 here)
        if (n < 253) {
            A.push_back(u8(n));
        } else if (n <= 0xffff) {
            A.push_back(253);
            A.push_back(u8(n));
            A.push_back(u8(n >> 8));
        } else {
            A.push_back(254);
            put_le32(u32(n));
        }
    };
    SameMessage same_message(res);
    for (size_t k = 0; k < res.sigs.size(); ++k) {
        const PendingSig& p = res.sigs[k];
        SecpVerifyJob& sj = out.secp_jobs[k];
        if (!p.device_hash) {
            secp::pack_verify_job(p.pubkey.data(), p.pubkey.size(), p.sig.data(), p.sig.size(), p.msg.data, sj);
            ++out.host_jobs;
            continue;
        }
        if (!res.all_forms)
            throw std::invalid_argument("pack_sighash_var: the block was connected without defer_all_forms");
        secp::pack_verify_job(p.pubkey.data(), p.pubkey.size(), p.sig.data(), p.sig.size(), kZero, sj);
        if (same_message(k)) {  // another key against the message of the entry before: its segments
            SighashVarJob j = out.jobs.back();
            j.out_index = u32(k);
            j.kind = sj.kind;
            sj.kind = SECP_KIND_INVALID;
            out.jobs.push_back(j);
            ++out.device_jobs;
            if (p.sigversion == SigVersion::WITNESS_V0) ++out.device_v0;
            else if (!sighash_all_form(SigVersion::BASE, p.hash_type)) ++out.device_partial;
            continue;
        }
        const SighashTxForms& f = *res.forms.at(p.tx_index);
        const Bytes& T = f.t.bytes;
        const size_t off = f.t.script_off.at(p.n_in);
        const int base = p.hash_type & 0x1f;
        const bool anyone = p.hash_type & SIGHASH_ANYONECANPAY;
        const bool none = base == SIGHASH_NONE, single = base == SIGHASH_SINGLE;
        const u8* lock_time = T.data() + T.size() - 4;
        SighashVarJob j{};
        j.first_seg = u32(out.segs.size());
        auto seg = [&](size_t at, size_t len) { out.segs.push_back(SighashSeg{u32(at), u32(len)}); };
        if (p.sigversion == SigVersion::WITNESS_V0) {
            const size_t at = A.size();
            put(T.data(), 4);
            put(anyone ? kZero : f.pre.prevouts.data, 32);
            put(anyone || none || single ? kZero : f.pre.sequence.data, 32);
            put(T.data() + off - 36, 36);
            put(p.code.data(), p.code.size());
            u8 amt[8];
            store_le32(amt, u32(u64(p.amount)));
            store_le32(amt + 4, u32(u64(p.amount) >> 32));
            put(amt, 8);
            put(T.data() + off + 1, 4);
            if (!none && !single) {
                put(f.pre.outputs.data, 32);
            } else if (single && p.n_in < f.n_out()) {
                u8 ho[32];
                sha256d(T.data() + f.out_off[p.n_in], f.out_off[p.n_in + 1] - f.out_off[p.n_in], ho);
                put(ho, 32);
            } else {
                put(kZero, 32);
            }
            put(lock_time, 4);
            put_le32(u32(p.hash_type));
            seg(at, A.size() - at);
            ++out.device_v0;
        } else {
            if (single && p.n_in >= f.n_out()) throw std::logic_error("pack_sighash_var: a constant-one hash was deferred");
            const bool need_t = !(none && !anyone);  // NONE reads only Z
            if (need_t && t_at[p.tx_index] < 0) {
                t_at[p.tx_index] = int64_t(A.size());
                put(T.data(), T.size());
            }
            if ((none || single) && !anyone && z_at[p.tx_index] < 0) {
                z_at[p.tx_index] = int64_t(A.size());
                put(T.data(), f.outs_off);
                for (u32 o : f.t.script_off) std::memset(A.data() + z_at[p.tx_index] + o + 1, 0, 4);
            }
            const size_t tb = need_t ? size_t(t_at[p.tx_index]) : 0, zb = size_t(std::max<int64_t>(z_at[p.tx_index], 0));
            if (anyone) {
                const size_t head = A.size();
                put(T.data(), 4);
                A.push_back(1);
                seg(head, 5);
                seg(tb + off - 36, 36);
            } else if (none || single) {
                seg(zb, off);
            } else {
                seg(tb, off);
            }
            // the emitted code, and what follows it up to the next shared range
            size_t at = A.size();
            put(p.code.data(), p.code.size());
            if (anyone || none || single) put(T.data() + off + 1, 4);
            if ((none || single) && !anyone) {
                seg(at, A.size() - at);
                seg(zb + off + 5, f.outs_off - off - 5);
                at = A.size();
            }
            if (none) {
                A.push_back(0);
                put(lock_time, 4);
                put_le32(u32(p.hash_type));
                seg(at, A.size() - at);
            } else if (single) {
                put_cs(u64(p.n_in) + 1);
                seg(at, A.size() - at);
                seg(0, 9 * size_t(p.n_in));
                seg(tb + f.out_off[p.n_in], f.out_off[p.n_in + 1] - f.out_off[p.n_in]);
                at = A.size();
                put(lock_time, 4);
                put_le32(u32(p.hash_type));
                seg(at, 8);
            } else {
                seg(at, A.size() - at);
                if (anyone) seg(tb + f.outs_off, T.size() - f.outs_off);
                else seg(tb + off + 1, T.size() - off - 1);
                at = A.size();
                put_le32(u32(p.hash_type));
                seg(at, 4);
            }
            if (!sighash_all_form(SigVersion::BASE, p.hash_type)) ++out.device_partial;
        }
        if (A.size() > 0xffffffffULL) throw std::length_error("sighash arena exceeds 4 GiB");
        j.n_seg = u32(out.segs.size()) - j.first_seg;
        j.out_index = u32(k);
        j.kind = sj.kind;  // INVALID stays INVALID: host parsing already failed
        sj.kind = SECP_KIND_INVALID;
        out.jobs.push_back(j);
        ++out.device_jobs;
    }
    return out;
}

void sighash_var_check(size_t arena_len, const SighashSeg* segs, size_t n_segs, const SighashVarJob* jobs, size_t n,
                       size_t n_out) {
    for (size_t s = 0; s < n_segs; ++s)
        if (u64(segs[s].off) + segs[s].len > arena_len)
            throw std::invalid_argument("sighash segment " + std::to_string(s) + " lies outside the arena");
    for (size_t k = 0; k < n; ++k) {
        const std::string who = "sighash job " + std::to_string(k);
        if (jobs[k].n_seg > SIGHASH_VAR_MAX_SEGMENTS) throw std::invalid_argument(who + ": too many segments");
        if (u64(jobs[k].first_seg) + jobs[k].n_seg > n_segs)
            throw std::invalid_argument(who + ": segments past the end of the table");
        u64 total = 0;
        for (u32 s = 0; s < jobs[k].n_seg; ++s) total += segs[jobs[k].first_seg + s].len;
        if (total >= (1u << 29)) throw std::invalid_argument(who + ": message too long");
        if (jobs[k].out_index >= n_out) throw std::invalid_argument(who + ": output index out of range");
    }
}

Bytes sighash_var_model(const Bytes& arena, const SighashSeg* segs, size_t n_segs, const SighashVarJob* jobs, size_t n) {
    sighash_var_check(arena.size(), segs, n_segs, jobs, n, size_t(-1));
    Bytes out(n * 32);
    Bytes msg;
    for (size_t k = 0; k < n; ++k) {
        msg.clear();
        for (u32 s = 0; s < jobs[k].n_seg; ++s) {
            const SighashSeg& g = segs[jobs[k].first_seg + s];
            msg.insert(msg.end(), arena.begin() + g.off, arena.begin() + g.off + g.len);
        }
        sha256d(msg.data(), msg.size(), &out[k * 32]);
    }
    return out;
}

SigWindowMode sig_window_mode(const ConnectResult& res) {
    if (res.all_forms) return SigWindowMode::ALL_FORMS;
    return res.templates.empty() ? SigWindowMode::HOST_HASH : SigWindowMode::LEGACY_ALL;
}

SigWindowPack pack_sig_window(const std::vector<const ConnectResult*>& results, u64 arena_limit) {
    SigWindowPack out;
    out.sig_begin.reserve(results.size() + 1);
    out.sig_begin.push_back(0);
    bool have_mode = false;
    auto check_arena = [&](const Bytes& a) {  // before a block's arena joins the window's
        if (u64(out.arena.size()) + a.size() >= arena_limit)
            throw std::length_error("signature window: the arena reaches the 32-bit offset limit");
    };
    for (const ConnectResult* r : results) {
        const ConnectResult& res = *r;
        const u32 sig_base = out.sig_begin.back();
        if (u64(sig_base) + res.sigs.size() >= (u64(1) << 31))
            throw std::length_error("signature window: too many signatures");
        out.sig_begin.push_back(sig_base + u32(res.sigs.size()));
        if (res.sigs.empty()) continue;
        const SigWindowMode mode = sig_window_mode(res);
        if (have_mode && mode != out.mode)
            throw std::invalid_argument("signature window: blocks connected with different -gpusighash modes");
        const bool first = !have_mode;  // the first block with signatures
        out.mode = mode;
        have_mode = true;
        const u32 arena_base = u32(out.arena.size());
        if (mode == SigWindowMode::HOST_HASH) {
            for (const PendingSig& p : res.sigs) {
                if (p.device_hash) throw std::invalid_argument("signature window: a deferred hash without its mode");
                SecpVerifyJob sj;
                secp::pack_verify_job(p.pubkey.data(), p.pubkey.size(), p.sig.data(), p.sig.size(), p.msg.data, sj);
                out.secp_jobs.push_back(sj);
            }
            out.host_jobs += res.sigs.size();
        } else if (mode == SigWindowMode::LEGACY_ALL) {
            SighashPack p = pack_sighash(res);
            check_arena(p.arena);
            if (first) {  // every base is 0: the block's tables are the window's so far, moved not copied
                out.arena = std::move(p.arena);
                out.jobs = std::move(p.jobs);
                out.secp_jobs = std::move(p.secp_jobs);
                out.device_jobs = p.device_jobs;
                out.host_jobs = p.host_jobs;
                continue;
            }
            out.arena.insert(out.arena.end(), p.arena.begin(), p.arena.end());
            for (SighashJob j : p.jobs) {
                for (int s = 0; s < SIGHASH_SEGMENTS; ++s) j.off[s] += arena_base;
                j.out_index += sig_base;
                out.jobs.push_back(j);
            }
            out.secp_jobs.insert(out.secp_jobs.end(), p.secp_jobs.begin(), p.secp_jobs.end());
            out.device_jobs += p.device_jobs;
            out.host_jobs += p.host_jobs;
        } else {
            SighashVarPack p = pack_sighash_var(res);
            check_arena(p.arena);
            if (first) {
                out.arena = std::move(p.arena);
                out.segs = std::move(p.segs);
                out.var_jobs = std::move(p.jobs);
                out.secp_jobs = std::move(p.secp_jobs);
                out.device_jobs = p.device_jobs;
                out.host_jobs = p.host_jobs;
                continue;
            }
            out.arena.insert(out.arena.end(), p.arena.begin(), p.arena.end());
            const u64 seg_base = out.segs.size();
            if (seg_base + p.segs.size() > 0xffffffffULL) throw std::length_error("signature window: too many segments");
            for (SighashSeg g : p.segs) {
                g.off += arena_base;
                out.segs.push_back(g);
            }
            for (SighashVarJob j : p.jobs) {
                j.first_seg += u32(seg_base);
                j.out_index += sig_base;
                out.var_jobs.push_back(j);
            }
            out.secp_jobs.insert(out.secp_jobs.end(), p.secp_jobs.begin(), p.secp_jobs.end());
            out.device_jobs += p.device_jobs;
            out.host_jobs += p.host_jobs;
        }
    }
    return out;
}

std::vector<SigWindowRecord> sig_window_verdicts_model(const u32* verdicts, size_t n, const u32* sig_begin, size_t nb) {
    for (size_t b = 0; b < nb; ++b)
        if (sig_begin[b] > sig_begin[b + 1]) throw std::invalid_argument("signature window: prefix offsets decrease");
    if (nb && sig_begin[nb] > n) throw std::invalid_argument("signature window: prefix offsets pass the verdicts");
    std::vector<SigWindowRecord> out(nb);
    for (size_t b = 0; b < nb; ++b) {
        SigWindowRecord r{0, 0, 0, SIG_WINDOW_NONE};
        for (u32 i = sig_begin[b]; i < sig_begin[b + 1]; ++i) {
            const u32 v = verdicts[i];
            if (v == 1) ++r.n_valid;
            else if (v == 2) ++r.n_ask_host;
            else ++r.n_invalid;
            if (v != 1 && r.first_not_valid == SIG_WINDOW_NONE) r.first_not_valid = i - sig_begin[b];
        }
        out[b] = r;
    }
    return out;
}

std::vector<SigGroup> sig_group_table(const ConnectResult& res) {
    std::vector<SigGroup> out;
    out.reserve(res.sig_groups.size());
    for (const SigGroupRec& g : res.sig_groups) out.push_back(SigGroup{g.first, g.n_sigs, g.n_keys, 0});
    return out;
}

std::vector<SigGroup> sig_window_groups(const std::vector<const ConnectResult*>& results) {
    std::vector<SigGroup> out;
    u64 base = 0;
    for (const ConnectResult* r : results) {
        if (base + r->sigs.size() >= (u64(1) << 31)) throw std::length_error("signature window: too many signatures");
        for (const SigGroupRec& g : r->sig_groups) out.push_back(SigGroup{u32(base) + g.first, g.n_sigs, g.n_keys, 0});
        base += r->sigs.size();
    }
    return out;
}

void sig_group_check(size_t n_verdicts, const SigGroup* groups, size_t ng) {
    u64 end = 0;  // of the previous group
    for (size_t k = 0; k < ng; ++k) {
        const SigGroup& g = groups[k];
        const std::string who = "signature group " + std::to_string(k);
        if (g.n_sigs == 0) throw std::invalid_argument(who + ": no signature");
        if (g.n_sigs > g.n_keys) throw std::invalid_argument(who + ": more signatures than keys");
        if (g.n_keys > 20) throw std::invalid_argument(who + ": more than 20 keys");
        const u64 pairs = u64(g.n_sigs) * (g.n_keys - g.n_sigs + 1);
        if (pairs > SIG_GROUP_MAX_PAIRS) throw std::invalid_argument(who + ": too many pairs");
        if (g.first < end) throw std::invalid_argument(who + ": overlaps or precedes the group before it");
        end = u64(g.first) + pairs;
        if (end > n_verdicts) throw std::invalid_argument(who + ": reaches past the verdicts");
    }
}

void sig_group_resolve_model(u32* verdicts, size_t n_verdicts, const SigGroup* groups, size_t ng) {
    sig_group_check(n_verdicts, groups, ng);
    for (size_t k = 0; k < ng; ++k) {
        const u32 m = groups[k].n_sigs, n = groups[k].n_keys, w = n - m + 1;
        u32* v = verdicts + groups[k].first;
        u32 a = 0, b = 0, outcome = 1;
        while (a < m) {
            const u32 x = v[a * w + (b - a)];
            if (x == 2) {
                outcome = 2;
                break;
            }
            if (x == 1) ++a;
            ++b;
            if (m - a > n - b) {
                outcome = 0;
                break;
            }
        }
        for (u32 i = 0; i < m * w; ++i) v[i] = outcome;
    }
}

}  // namespace nodexa
