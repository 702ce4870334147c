// Bindings for secp256k1 (crypto/secp256k1.*) and the script interpreter (chain/interpreter.*).
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <map>
#include <set>
#include <tuple>

#include "../chain/coins.hpp"
#include "../chain/indexes.hpp"
#include "../chain/interpreter.hpp"
#include "../chain/scriptcache.hpp"
#include "../chain/sigcache.hpp"
#include "../chain/sighash.hpp"
#include "../chain/params.hpp"
#include "../crypto/secp256k1.hpp"
#include "../crypto/secp256k1_model32.hpp"
#include "../../hip/kernels/secp256k1_probe.hpp"

namespace py = pybind11;
using namespace nodexa;

PYBIND11_MAKE_OPAQUE(std::vector<PendingSig>)

namespace {

Bytes bytes_of(const py::bytes& b) {
    std::string s = b;
    return Bytes(s.begin(), s.end());
}
py::bytes pyb(const u8* p, size_t n) { return py::bytes(reinterpret_cast<const char*>(p), n); }
py::bytes pyb(const Bytes& b) { return pyb(b.data(), b.size()); }

void need32(const std::string& s, const char* what) {
    if (s.size() != 32) throw std::invalid_argument(std::string(what) + " must be 32 bytes");
}

Transaction tx_of(const py::bytes& raw) {
    const Bytes b = bytes_of(raw);
    Reader r(b);
    Transaction tx = Transaction::deserialize(r, true);
    if (!r.empty()) throw std::invalid_argument("trailing bytes after transaction");
    return tx;
}

std::vector<Bytes> stack_of(const std::vector<py::bytes>& v) {
    std::vector<Bytes> out;
    out.reserve(v.size());
    for (auto& x : v) out.push_back(bytes_of(x));
    return out;
}

}  // namespace

void bind_script(py::module_& m) {
    // ---------------------------------------------------------------- secp256k1
    m.def("secp_pubkey_create", [](const py::bytes& key, bool compressed) -> py::object {
        const std::string k = key;
        need32(k, "key");
        secp::Ge p;
        if (!secp::pubkey_create(reinterpret_cast<const u8*>(k.data()), p)) return py::none();
        u8 out[65];
        return pyb(out, secp::pubkey_serialize(p, compressed, out));
    }, py::arg("key"), py::arg("compressed") = true, "public key of a 32-byte secret (None if invalid)");
    m.def("secp_pubkey_normalize", [](const py::bytes& pub, bool compressed) -> py::object {
        const std::string s = pub;
        secp::Ge p;
        if (!secp::pubkey_parse(reinterpret_cast<const u8*>(s.data()), s.size(), p)) return py::none();
        u8 out[65];
        return pyb(out, secp::pubkey_serialize(p, compressed, out));
    }, py::arg("pubkey"), py::arg("compressed") = true, "parse (02/03/04/06/07) and re-serialize, None if invalid");
    m.def("secp_sign", [](const py::bytes& msg, const py::bytes& key) -> py::object {
        const std::string m32 = msg, k = key;
        need32(m32, "msg");
        need32(k, "key");
        secp::Scalar r, s;
        if (!secp::ecdsa_sign(reinterpret_cast<const u8*>(m32.data()), reinterpret_cast<const u8*>(k.data()), r, s))
            return py::none();
        u8 der[72];
        return pyb(der, secp::sig_serialize_der(r, s, der));
    }, "RFC 6979 low-S DER signature (CKey::Sign with test_case 0)");
    m.def("secp_verify", [](const py::bytes& pub, const py::bytes& sig, const py::bytes& msg) {
        const std::string p = pub, sg = sig, m32 = msg;
        need32(m32, "msg");
        return secp::verify_der(reinterpret_cast<const u8*>(p.data()), p.size(), reinterpret_cast<const u8*>(sg.data()),
                                sg.size(), reinterpret_cast<const u8*>(m32.data()));
    }, "CPubKey::Verify: lax DER, S normalised");
    m.def("secp_sign_compact", [](const py::bytes& msg, const py::bytes& key, bool compressed) -> py::object {
        const std::string m32 = msg, k = key;
        need32(m32, "msg");
        need32(k, "key");
        u8 out[65];
        if (!secp::sign_compact(reinterpret_cast<const u8*>(m32.data()), reinterpret_cast<const u8*>(k.data()),
                                compressed, out))
            return py::none();
        return pyb(out, 65);
    });
    m.def("secp_recover_compact", [](const py::bytes& msg, const py::bytes& sig) -> py::object {
        const std::string m32 = msg, s = sig;
        need32(m32, "msg");
        if (s.size() != 65) return py::none();
        secp::Ge p;
        bool compressed = false;
        if (!secp::recover_compact(reinterpret_cast<const u8*>(m32.data()), reinterpret_cast<const u8*>(s.data()), p,
                                   compressed))
            return py::none();
        u8 out[65];
        return pyb(out, secp::pubkey_serialize(p, compressed, out));
    });
    m.def("secp_seckey_tweak_add", [](const py::bytes& key, const py::bytes& tweak) -> py::object {
        std::string k = key;
        const std::string t = tweak;
        need32(k, "key");
        need32(t, "tweak");
        if (!secp::seckey_tweak_add(reinterpret_cast<u8*>(k.data()), reinterpret_cast<const u8*>(t.data())))
            return py::none();
        return py::bytes(k);
    });
    m.def("secp_pubkey_tweak_add", [](const py::bytes& pub, const py::bytes& tweak) -> py::object {
        const std::string p = pub, t = tweak;
        need32(t, "tweak");
        secp::Ge g;
        if (!secp::pubkey_parse(reinterpret_cast<const u8*>(p.data()), p.size(), g)) return py::none();
        if (!secp::pubkey_tweak_add(g, reinterpret_cast<const u8*>(t.data()))) return py::none();
        u8 out[65];
        return pyb(out, secp::pubkey_serialize(g, p.size() == 33, out));
    });
    m.def("secp_seckey_valid", [](const py::bytes& key) {
        const std::string k = key;
        return k.size() == 32 && secp::seckey_valid(reinterpret_cast<const u8*>(k.data()));
    });
    // DER signature normalisation helpers used by policy and the GPU batch packer
    m.def("secp_der_to_rs", [](const py::bytes& sig) -> py::object {
        const std::string s = sig;
        secp::Scalar r, sv;
        if (!secp::sig_parse_der_lax(reinterpret_cast<const u8*>(s.data()), s.size(), r, sv)) return py::none();
        if (secp::sc_is_high(sv)) sv = secp::sc_neg(sv);
        u8 out[64];
        secp::sc_to_be(r, out);
        secp::sc_to_be(sv, out + 32);
        return pyb(out, 64);
    }, "lax-DER signature -> r || low-S s (32+32 bytes big-endian), None on a structural error");

    // ---------------------------------------------------------------- GPU batch verification
    m.attr("SECP_JOB_BYTES") = sizeof(SecpVerifyJob);
    m.def("secp_pack_jobs", [](const py::list& items) {
        // items: [(pubkey, der_sig_without_hashtype, msg32)] -> SecpVerifyJob array
        std::string out(items.size() * sizeof(SecpVerifyJob), '\0');
        auto* jobs = reinterpret_cast<SecpVerifyJob*>(&out[0]);
        size_t k = 0;
        for (auto it : items) {
            auto t = it.cast<py::tuple>();
            const std::string pub = t[0].cast<py::bytes>(), sig = t[1].cast<py::bytes>(),
                              msg = t[2].cast<py::bytes>();
            need32(msg, "msg");
            secp::pack_verify_job(reinterpret_cast<const u8*>(pub.data()), pub.size(),
                                  reinterpret_cast<const u8*>(sig.data()), sig.size(),
                                  reinterpret_cast<const u8*>(msg.data()), jobs[k++]);
        }
        return py::bytes(out);
    }, "pack (pubkey, DER signature, message) triples as gfx950 verify jobs");
    m.def("secp_gen_table32", [] {
        return py::bytes(reinterpret_cast<const char*>(secp::gen_table32()), 64 * 16 * 16 * 4);
    }, "the device comb table of G (64 KiB)");
    m.def("secp_verify_model32", [](const py::bytes& pub, const py::bytes& sig, const py::bytes& msg) {
        const std::string p = pub, sg = sig, m32 = msg;
        need32(m32, "msg");
        SecpVerifyJob job;
        secp::pack_verify_job(reinterpret_cast<const u8*>(p.data()), p.size(), reinterpret_cast<const u8*>(sg.data()),
                              sg.size(), reinterpret_cast<const u8*>(m32.data()), job);
        return secp::verify_job_model32(job);
    }, "the GPU verifier's 32-bit-limb arithmetic run on the host: 1 valid, 0 invalid, 2 degenerate");
    m.attr("SECP_PROBE_IN_BYTES") = SECP_PROBE_IN_WORDS * 4;
    m.attr("SECP_PROBE_OUT_BYTES") = SECP_PROBE_OUT_WORDS * 4;
    m.def("secp32_probe", [](uint32_t op, const py::bytes& records) {
        const std::string in = records;
        if (op >= SECP_PROBE_NUM_OPS) throw std::invalid_argument("secp32_probe: unknown op");
        if (in.size() % (SECP_PROBE_IN_WORDS * 4)) throw std::invalid_argument("secp32_probe: ragged records");
        const size_t n = in.size() / (SECP_PROBE_IN_WORDS * 4);
        std::vector<uint32_t> w(n * SECP_PROBE_IN_WORDS), out(n * SECP_PROBE_OUT_WORDS);
        std::memcpy(w.data(), in.data(), in.size());
        for (size_t i = 0; i < n; ++i)
            secp32::probe_record(op, w.data() + i * SECP_PROBE_IN_WORDS, out.data() + i * SECP_PROBE_OUT_WORDS);
        return py::bytes(reinterpret_cast<const char*>(out.data()), out.size() * 4);
    }, "one primitive of the GPU verifier's limb arithmetic over packed records, run on the host "
       "(hip/kernels/secp256k1_probe.hpp; the secp_probe kernel runs the same switch on the device)");

    // ---------------------------------------------------------------- interpreter
    m.attr("SCRIPT_VERIFY_P2SH") = u32(SCRIPT_VERIFY_P2SH);
    m.attr("STANDARD_SCRIPT_VERIFY_FLAGS") = kStandardScriptFlags;
    m.attr("MANDATORY_SCRIPT_VERIFY_FLAGS") = kMandatoryScriptFlags;
    m.def("script_flag_bits", [] {
        py::dict d;
        const std::pair<const char*, u32> f[] = {
            {"NONE", SCRIPT_VERIFY_NONE}, {"P2SH", SCRIPT_VERIFY_P2SH}, {"STRICTENC", SCRIPT_VERIFY_STRICTENC},
            {"DERSIG", SCRIPT_VERIFY_DERSIG}, {"LOW_S", SCRIPT_VERIFY_LOW_S}, {"NULLDUMMY", SCRIPT_VERIFY_NULLDUMMY},
            {"SIGPUSHONLY", SCRIPT_VERIFY_SIGPUSHONLY}, {"MINIMALDATA", SCRIPT_VERIFY_MINIMALDATA},
            {"DISCOURAGE_UPGRADABLE_NOPS", SCRIPT_VERIFY_DISCOURAGE_UPGRADABLE_NOPS},
            {"CLEANSTACK", SCRIPT_VERIFY_CLEANSTACK}, {"CHECKLOCKTIMEVERIFY", SCRIPT_VERIFY_CHECKLOCKTIMEVERIFY},
            {"CHECKSEQUENCEVERIFY", SCRIPT_VERIFY_CHECKSEQUENCEVERIFY}, {"WITNESS", SCRIPT_VERIFY_WITNESS},
            {"DISCOURAGE_UPGRADABLE_WITNESS_PROGRAM", SCRIPT_VERIFY_DISCOURAGE_UPGRADABLE_WITNESS_PROGRAM},
            {"MINIMALIF", SCRIPT_VERIFY_MINIMALIF}, {"NULLFAIL", SCRIPT_VERIFY_NULLFAIL},
            {"WITNESS_PUBKEYTYPE", SCRIPT_VERIFY_WITNESS_PUBKEYTYPE}};
        for (auto& [k, v] : f) d[k] = v;
        return d;
    }, "the reference's flag names (src/test/transaction_tests.cpp mapFlagNames)");
    m.def("verify_script", [](const py::bytes& script_sig, const py::bytes& script_pubkey,
                              const std::vector<py::bytes>& witness, u32 flags, const py::bytes& tx_raw, unsigned n_in,
                              int64_t amount, int sigcache) {
        const Transaction tx = tx_of(tx_raw);
        if (n_in >= tx.vin.size()) throw std::invalid_argument("input index out of range");
        const PrecomputedTx cache(tx);
        TxSigChecker checker(&tx, n_in, amount, &cache);
        if (sigcache < 0 || sigcache > 2) throw std::invalid_argument("sigcache: 0 none, 1 store, 2 use");
        checker.sigcache = TxSigChecker::CacheMode(sigcache);
        const std::vector<Bytes> wit = stack_of(witness);
        ScriptError err = ScriptError::UNKNOWN_ERROR;
        py::gil_scoped_release rel;
        const bool ok = verify_script(bytes_of(script_sig), bytes_of(script_pubkey), &wit, flags, checker, &err);
        py::gil_scoped_acquire acq;
        return py::make_tuple(ok, script_error_name(err));
    }, py::arg("script_sig"), py::arg("script_pubkey"), py::arg("witness"), py::arg("flags"), py::arg("tx"),
       py::arg("n_in"), py::arg("amount"), py::arg("sigcache") = 0,
       "VerifyScript of input n_in of the serialized tx -> (ok, error name); sigcache 1 = store verified "
       "signatures (mempool acceptance), 2 = answer from the cache (block validation)");
    m.def("sigcache_set_max_bytes", [](size_t b) { SigCache::instance().set_max_bytes(b); },
          "-maxsigcachesize (bytes of 32-byte entries)");
    m.def("sigcache_clear", [] { SigCache::instance().clear(); });
    m.def("sigcache_stats", [] {
        const SigCache::Stats s = SigCache::instance().stats();
        py::dict d;
        d["entries"] = s.entries;
        d["max_entries"] = s.max_entries;
        d["hits"] = s.hits;
        d["misses"] = s.misses;
        d["inserts"] = s.inserts;
        d["evictions"] = s.evictions;
        return d;
    });
    // ---- the script-execution cache (-scriptcache, chain/scriptcache.hpp)
    auto wtxid_of = [](const py::bytes& wtxid) {
        const std::string w = wtxid;
        if (w.size() != 32) throw std::invalid_argument("wtxid: 32 bytes");
        return Uint256::from_bytes(reinterpret_cast<const u8*>(w.data()));
    };
    m.def("scriptcache_set_max_bytes", [](size_t b) { ScriptCache::instance().set_max_bytes(b); },
          "half of -maxsigcachesize (bytes of 32-byte entries)");
    m.def("scriptcache_clear", [] { ScriptCache::instance().clear(); });
    m.def("scriptcache_stats", [] {
        const ScriptCache::Stats s = ScriptCache::instance().stats();
        py::dict d;
        d["entries"] = s.entries;
        d["max_entries"] = s.max_entries;
        d["hits"] = s.hits;
        d["misses"] = s.misses;
        d["inserts"] = s.inserts;
        d["erases"] = s.erases;
        d["evictions"] = s.evictions;
        return d;
    });
    m.def("scriptcache_contains", [wtxid_of](const py::bytes& wtxid, u32 flags) {
        return ScriptCache::instance().contains(wtxid_of(wtxid), flags);
    }, py::arg("wtxid"), py::arg("flags"), "whether every script of the transaction passed under these flags");
    m.def("scriptcache_insert", [wtxid_of](const py::bytes& wtxid, u32 flags) {
        ScriptCache::instance().insert(wtxid_of(wtxid), flags);
    }, py::arg("wtxid"), py::arg("flags"));
    m.def("eval_script", [](const std::vector<py::bytes>& stack, const py::bytes& script, u32 flags) {
        std::vector<Bytes> st = stack_of(stack);
        ScriptError err = ScriptError::UNKNOWN_ERROR;
        const bool ok = eval_script(st, bytes_of(script), flags, SigChecker(), SigVersion::BASE, &err);
        py::list out;
        for (auto& e : st) out.append(pyb(e));
        return py::make_tuple(ok, script_error_name(err), out);
    }, "EvalScript with no transaction context (signature checks fail)");
    m.def("signature_hash", [](const py::bytes& script_code, const py::bytes& tx_raw, unsigned n_in, int hash_type,
                               int64_t amount, int sigversion) {
        const Transaction tx = tx_of(tx_raw);
        const Uint256 h = signature_hash(bytes_of(script_code), tx, n_in, hash_type, amount,
                                         sigversion ? SigVersion::WITNESS_V0 : SigVersion::BASE);
        return pyb(h.data, 32);
    }, py::arg("script_code"), py::arg("tx"), py::arg("n_in"), py::arg("hash_type"), py::arg("amount") = 0,
       py::arg("sigversion") = 0, "SignatureHash (uint256 storage order)");
    m.def("check_transaction", [](const py::bytes& tx_raw, const ChainParams* params, const assets::Flags* flags,
                                  bool block_check, bool mempool_check) {
        return check_transaction(tx_of(tx_raw), true, params ? &params->assets : nullptr, flags, block_check,
                                 mempool_check);
    }, py::arg("tx"), py::arg("params") = nullptr, py::arg("asset_flags") = nullptr, py::arg("block_check") = false,
       py::arg("mempool_check") = false, "CheckTransaction reject reason, '' when valid (asset rules with params)");
    m.def("script_sigop_count", [](const py::bytes& s, bool accurate) {
        return script_sigop_count(bytes_of(s), accurate);
    }, py::arg("script"), py::arg("accurate") = false);
    // ---------------------------------------------------------------- UTXO set / ConnectBlock
    m.attr("COINBASE_MATURITY") = kCoinbaseMaturity;
    m.attr("BLOCK_SCRIPT_VERIFY_FLAGS") = kBlockScriptFlags;
    py::class_<CoinsView, std::shared_ptr<CoinsView>>(m, "CoinsView")
        .def(py::init<>())
        .def("__len__", &CoinsView::size)
        .def("append_journal", &CoinsView::append_journal, py::call_guard<py::gil_scoped_release>(),
             "append the outputs added / spent since the last flush as one fsynced journal record")
        .def("load_with_journal", &CoinsView::load_with_journal, py::call_guard<py::gil_scoped_release>())
        .def("compact", &CoinsView::compact, py::call_guard<py::gil_scoped_release>(),
             "fold the journal into a fresh snapshot and truncate it")
        .def_property_readonly("dirty", &CoinsView::dirty)
        .def_readonly("journal_seq", &CoinsView::journal_seq)
        .def_readonly("replayed", &CoinsView::replayed)
        .def("get", [](const CoinsView& v, const py::bytes& txid, u32 n) -> py::object {
            OutPoint o;
            const std::string h = txid;
            need32(h, "txid");
            o.hash = Uint256::from_bytes(reinterpret_cast<const u8*>(h.data()));
            o.n = n;
            const Coin* c = v.find(o);
            if (!c) return py::none();
            return py::make_tuple(c->out.value, pyb(c->out.script_pubkey), c->height, c->coinbase);
        }, "(value, scriptPubKey, height, coinbase) of an unspent output, or None")
        .def("height_of_txid", [](const CoinsView& v, const py::bytes& txid) -> py::object {
            // AccessByTxid (src/coins.cpp): probe output indexes up to MAX_OUTPUTS_PER_BLOCK
            // (MAX_BLOCK_WEIGHT / (WITNESS_SCALE_FACTOR * size of an empty CTxOut))
            OutPoint o;
            const std::string h = txid;
            need32(h, "txid");
            o.hash = Uint256::from_bytes(reinterpret_cast<const u8*>(h.data()));
            for (o.n = 0; o.n < 8000000u / (4u * 9u); ++o.n)
                if (const Coin* c = v.find(o)) return py::int_(c->height);
            return py::none();
        }, "height of the block holding a transaction with an unspent output, or None")
        .def("add", [](CoinsView& v, const py::bytes& txid, u32 n, int64_t value, const py::bytes& spk, u32 height,
                       bool coinbase) {
            OutPoint o;
            const std::string h = txid;
            need32(h, "txid");
            o.hash = Uint256::from_bytes(reinterpret_cast<const u8*>(h.data()));
            o.n = n;
            Coin c;
            c.out.value = value;
            c.out.script_pubkey = bytes_of(spk);
            c.height = height;
            c.coinbase = coinbase;
            v.add(o, std::move(c));
        })
        .def_property("best_block", [](const CoinsView& v) { return pyb(v.best_block.data, 32); },
                      [](CoinsView& v, const py::bytes& b) {
                          const std::string h = b;
                          need32(h, "best_block");
                          v.best_block = Uint256::from_bytes(reinterpret_cast<const u8*>(h.data()));
                      })
        .def("spend", [](CoinsView& v, const py::bytes& txid, u32 n) {
            OutPoint o;
            const std::string h = txid;
            need32(h, "txid");
            o.hash = Uint256::from_bytes(reinterpret_cast<const u8*>(h.data()));
            o.n = n;
            return v.spend(o);
        }, "remove an unspent output (True if it existed)")
        .def("save", &CoinsView::save, py::call_guard<py::gil_scoped_release>())
        .def("load", &CoinsView::load, py::call_guard<py::gil_scoped_release>())
        .def("stats", [](const CoinsView& v) {
            const auto s = v.stats();
            return py::make_tuple(s.txouts, s.transactions, s.total, pyb(s.hash.data, 32), s.bogosize);
        }, "(txouts, transactions, total amount, hash_serialized_2, bogosize)")
        .def("outputs_for_scripts", [](const CoinsView& v, const std::vector<py::bytes>& spks) {
            std::set<Bytes> want;
            for (auto& s : spks) want.insert(bytes_of(s));
            py::list out;
            v.for_each([&](const OutPoint& o, const Coin& c) {
                if (want.count(c.out.script_pubkey))
                    out.append(py::make_tuple(pyb(o.hash.data, 32), o.n, c.out.value, pyb(c.out.script_pubkey),
                                              c.height, c.coinbase));
            });
            return out;
        }, "unspent outputs paying any of these scriptPubKeys: (txid, n, value, spk, height, coinbase)")
        .def("asset_outputs", [](const CoinsView& v, py::object hashes) {
            // asset scripts (P2PKH prefix + OP_CLORE_ASSET payload) of these hash160s, or of all when None
            std::set<std::string> want;
            const bool all = hashes.is_none();
            if (!all)
                for (auto& h : hashes.cast<std::vector<py::bytes>>()) want.insert(std::string(h));
            py::list out;
            v.for_each([&](const OutPoint& o, const Coin& c) {
                const Bytes& s = c.out.script_pubkey;
                if (assets::asset_script_kind(s) == assets::OutKind::NONE) return;
                if (!all && !want.count(std::string(reinterpret_cast<const char*>(s.data() + 3), 20))) return;
                out.append(py::make_tuple(pyb(o.hash.data, 32), o.n, c.out.value, pyb(s), c.height, c.coinbase));
            });
            return out;
        }, py::arg("hashes") = py::none(),
           "unspent asset outputs to these hash160s (all when None): (txid, n, value, spk, height, coinbase)");
    py::class_<ConnectResult> cr(m, "ConnectResult");
    cr.def_readonly("ok", &ConnectResult::ok)
        .def_readonly("reject", &ConnectResult::reject)
        .def_readonly("dos", &ConnectResult::dos)
        .def_readonly("fees", &ConnectResult::fees)
        .def_readonly("sigop_cost", &ConnectResult::sigop_cost)
        .def_readonly("sig_at", &ConnectResult::sig_at)
        .def_readonly("script_cache_txs", &ConnectResult::script_cache_txs,
                      "with script_cache: block index of every transaction the script-execution cache answered for")
        .def("script_cache_erase", [](const ConnectResult& r) {
            size_t n = 0;
            for (const Uint256& w : r.script_cache_wtxids) n += ScriptCache::instance().erase(w, r.script_cache_flags);
            return n;
        }, "erase the script-cache entries of script_cache_txs, under the flags they were looked up with (the block "
           "is final) -> how many were still there")
        .def_property_readonly("asset_undo", [](const ConnectResult& r) { return pyb(r.asset_undo); })
        .def_property_readonly("num_sigs", [](const ConnectResult& r) { return r.sigs.size(); })
        .def_property_readonly("num_device_hashes", [](const ConnectResult& r) {
            size_t n = 0;
            for (auto& p : r.sigs) n += p.device_hash;
            return n;
        }, "deferred signatures whose message hash is left to the batch (defer_sighash)")
        .def("sig_items", [](const ConnectResult& r) {
            py::list out;
            for (size_t k = 0; k < r.sigs.size(); ++k)
                out.append(py::make_tuple(pyb(r.sigs[k].pubkey), pyb(r.sigs[k].sig), pyb(r.sig_msg(k).data, 32)));
            return out;
        }, "deferred signatures as (pubkey, DER signature, message) for ops/secp.verify_batch; with defer_sighash "
           "the messages left to the batch are computed here, on the host")
        .def("sighash_pack", [](const ConnectResult& r) {
            SighashPack p;
            {
                py::gil_scoped_release rel;
                p = pack_sighash(r);
            }
            return py::make_tuple(pyb(p.arena),
                                  py::bytes(reinterpret_cast<const char*>(p.jobs.data()), p.jobs.size() * sizeof(SighashJob)),
                                  py::bytes(reinterpret_cast<const char*>(p.secp_jobs.data()),
                                            p.secp_jobs.size() * sizeof(SecpVerifyJob)),
                                  p.device_jobs, p.host_jobs);
        }, "(arena, SighashJob table, SecpVerifyJob array, device-hashed count, host-hashed count) for "
           "ops/sighash.verify_block_sigs: the secp records of device-hashed signatures are INVALID with z = 0 until "
           "sighash_gather_batch fills them");
    cr.def_readonly("all_forms", &ConnectResult::all_forms, "connected with defer_all_forms")
        .def_property_readonly("num_device_v0", [](const ConnectResult& r) {
            size_t n = 0;
            for (auto& p : r.sigs) n += p.device_hash && p.sigversion == SigVersion::WITNESS_V0;
            return n;
        }, "of num_device_hashes: witness-v0 signatures (defer_all_forms)")
        .def_property_readonly("num_device_partial", [](const ConnectResult& r) {
            size_t n = 0;
            for (auto& p : r.sigs)
                n += p.device_hash && p.sigversion == SigVersion::BASE && !sighash_all_form(SigVersion::BASE, p.hash_type);
            return n;
        }, "of num_device_hashes: legacy signatures of another form than ALL's (defer_all_forms)")
        .def("sighash_pack_var", [](const ConnectResult& r) {
            SighashVarPack p;
            {
                py::gil_scoped_release rel;
                p = pack_sighash_var(r);
            }
            return py::make_tuple(pyb(p.arena),
                                  py::bytes(reinterpret_cast<const char*>(p.segs.data()), p.segs.size() * sizeof(SighashSeg)),
                                  py::bytes(reinterpret_cast<const char*>(p.jobs.data()), p.jobs.size() * sizeof(SighashVarJob)),
                                  py::bytes(reinterpret_cast<const char*>(p.secp_jobs.data()),
                                            p.secp_jobs.size() * sizeof(SecpVerifyJob)),
                                  p.device_jobs, p.host_jobs);
        }, "(arena, SighashSeg table, SighashVarJob table, SecpVerifyJob array, device-hashed count, host-hashed count) "
           "of a defer_all_forms result, for ops/sighash.verify_block_sigs: the secp records of device-hashed "
           "signatures are INVALID with z = 0 until sighash_gather_var fills them");
    m.def("sighash_pack_var_cases", [](const std::vector<std::tuple<py::bytes, unsigned, py::bytes, int, Amount, int>>& cases,
                                       const py::bytes& pubkey, const py::bytes& sig) {
        // the deferred record of each case as check_sig leaves it, one transaction entry per distinct raw
        ConnectResult r;
        r.all_forms = true;
        std::map<std::string, u32> seen;
        std::vector<Transaction> txs;
        const Bytes pk = bytes_of(pubkey), sg = bytes_of(sig);
        for (auto& c : cases) {
            const std::string raw = std::get<0>(c);
            auto it = seen.find(raw);
            if (it == seen.end()) {
                it = seen.emplace(raw, u32(txs.size())).first;
                txs.push_back(tx_of(std::get<0>(c)));
                r.forms.push_back(std::make_shared<const SighashTxForms>(txs.back()));
            }
            const Transaction& tx = txs[it->second];
            const unsigned n_in = std::get<1>(c);
            const Bytes code = bytes_of(std::get<2>(c));
            const int ht = std::get<3>(c);
            const SigVersion sv = std::get<5>(c) ? SigVersion::WITNESS_V0 : SigVersion::BASE;
            PendingSig p{Uint256(), sg, pk};
            if (sighash_deferrable(tx.vin.size(), tx.vout.size(), n_in, ht, sv)) {
                p.device_hash = true;
                p.tx_index = it->second;
                p.n_in = n_in;
                p.hash_type = ht;
                p.code = sighash_emitted_code(code, sv);
                p.sigversion = sv;
                p.amount = std::get<4>(c);
            } else {
                p.msg = signature_hash(code, tx, n_in, ht, std::get<4>(c), sv);
            }
            r.sigs.push_back(std::move(p));
            r.sig_at.emplace_back(it->second, n_in);
        }
        return r;
    }, py::arg("cases"), py::arg("pubkey"), py::arg("sig"),
       "a ConnectResult as connect_block(defer_all_forms=True) would leave it for these (raw tx, input, script code, "
       "hash type, amount, sigversion) signatures, all with one key and signature: for packing them without a block");
    m.attr("SIGHASH_JOB_BYTES") = sizeof(SighashJob);
    m.attr("SIGHASH_VAR_JOB_BYTES") = sizeof(SighashVarJob);
    m.attr("SIGHASH_SEG_BYTES") = sizeof(SighashSeg);
    m.attr("SIGHASH_VAR_MAX_SEGMENTS") = SIGHASH_VAR_MAX_SEGMENTS;
    m.def("sighash_form", [](int sigversion, int hash_type) {
        return std::string(sighash_form(sigversion ? SigVersion::WITNESS_V0 : SigVersion::BASE, hash_type));
    }, "the form of a signature's message hash: all, none, single, each with |acp under ANYONECANPAY");
    auto var_tables = [](const py::bytes& segs, const py::bytes& jobs, std::vector<SighashSeg>& sv,
                         std::vector<SighashVarJob>& jv) {
        const std::string s = segs, j = jobs;
        if (s.size() % sizeof(SighashSeg)) throw std::invalid_argument("segment table is not a whole number of records");
        if (j.size() % sizeof(SighashVarJob)) throw std::invalid_argument("job table is not a whole number of records");
        sv.resize(s.size() / sizeof(SighashSeg));
        jv.resize(j.size() / sizeof(SighashVarJob));
        if (!s.empty()) std::memcpy(sv.data(), s.data(), s.size());
        if (!j.empty()) std::memcpy(jv.data(), j.data(), j.size());
    };
    m.def("sighash_var_check", [var_tables](size_t arena_len, const py::bytes& segs, const py::bytes& jobs, py::object n_out) {
        std::vector<SighashSeg> sv;
        std::vector<SighashVarJob> jv;
        var_tables(segs, jobs, sv, jv);
        sighash_var_check(arena_len, sv.data(), sv.size(), jv.data(), jv.size(),
                          n_out.is_none() ? jv.size() : n_out.cast<size_t>());
    }, py::arg("arena_len"), py::arg("segs"), py::arg("jobs"), py::arg("n_out") = py::none(),
       "ValueError on a segment outside the arena, a job whose segments pass the table or number more than "
       "SIGHASH_VAR_MAX_SEGMENTS, a message of 2^29 bytes or more, or an output index >= n_out (default: the job count)");
    m.def("sighash_var_model", [var_tables](const py::bytes& arena, const py::bytes& segs, const py::bytes& jobs) {
        std::vector<SighashSeg> sv;
        std::vector<SighashVarJob> jv;
        var_tables(segs, jobs, sv, jv);
        const Bytes a = bytes_of(arena);
        Bytes out;
        {
            py::gil_scoped_release rel;
            out = sighash_var_model(a, sv.data(), sv.size(), jv.data(), jv.size());
        }
        return pyb(out);
    }, "host model of sighash_gather_var: SHA256d of each job's segments in order, 32 bytes per job");
    m.attr("SIGHASH_ARENA_SLACK") = SIGHASH_ARENA_SLACK;
    m.attr("SECP_KIND_INVALID") = SECP_KIND_INVALID;
    m.def("sighash_template", [](const py::bytes& tx_raw) {
        const SighashTemplate t(tx_of(tx_raw));
        return py::make_tuple(pyb(t.bytes), t.script_off);
    }, "(blanked legacy serialisation, offset of each input's script-length byte)");
    m.def("sighash_script_code", [](const py::bytes& code) { return pyb(sighash_script_code(bytes_of(code))); },
          "what SignatureHash writes for the signed input's script: compact size + code without OP_CODESEPARATORs");
    m.def("sighash_all_form", [](int sigversion, int hash_type) {
        return sighash_all_form(sigversion ? SigVersion::WITNESS_V0 : SigVersion::BASE, hash_type);
    }, "whether a signature's message hash can be left to the batch (legacy, SIGHASH_ALL form)");
    m.def("sighash_check_jobs", [](size_t arena_len, const py::bytes& jobs, py::object n_out) {
        const std::string j = jobs;
        if (j.size() % sizeof(SighashJob)) throw std::invalid_argument("job table is not a whole number of records");
        const size_t n = j.size() / sizeof(SighashJob);
        std::vector<SighashJob> v(n);
        std::memcpy(v.data(), j.data(), j.size());
        sighash_check_jobs(arena_len, v.data(), n, n_out.is_none() ? n : n_out.cast<size_t>());
    }, py::arg("arena_len"), py::arg("jobs"), py::arg("n_out") = py::none(),
       "ValueError on a segment outside the arena or an output index >= n_out (default: the job count)");
    m.def("sighash_gather_model", [](const py::bytes& arena, const py::bytes& jobs) {
        const std::string j = jobs;
        if (j.size() % sizeof(SighashJob)) throw std::invalid_argument("job table is not a whole number of records");
        const size_t n = j.size() / sizeof(SighashJob);
        std::vector<SighashJob> v(n);
        std::memcpy(v.data(), j.data(), j.size());
        const Bytes a = bytes_of(arena);
        Bytes out;
        {
            py::gil_scoped_release rel;
            out = sighash_gather_model(a, v.data(), n);
        }
        return pyb(out);
    }, "host model of sighash_gather_batch: SHA256d of each job's four arena segments, 32 bytes per job");
    // ---- a window of consecutive blocks as one batch (-gpusigwindow)
    m.attr("SIG_WINDOW_RECORD_BYTES") = sizeof(SigWindowRecord);
    m.attr("SIG_WINDOW_NONE") = SIG_WINDOW_NONE;
    m.attr("SIG_WINDOW_ARENA_LIMIT") = SIG_WINDOW_ARENA_LIMIT;
    m.def("sig_window_pack", [](const py::list& results, py::object arena_limit) {
        std::vector<const ConnectResult*> rs;
        for (auto r : results) rs.push_back(&r.cast<const ConnectResult&>());
        const u64 limit = arena_limit.is_none() ? SIG_WINDOW_ARENA_LIMIT : arena_limit.cast<u64>();
        SigWindowPack p;
        {
            py::gil_scoped_release rel;
            p = pack_sig_window(rs, limit);
        }
        const bool var = p.mode == SigWindowMode::ALL_FORMS;
        return py::make_tuple(
            int(p.mode), pyb(p.arena),
            py::bytes(reinterpret_cast<const char*>(p.segs.data()), p.segs.size() * sizeof(SighashSeg)),
            var ? py::bytes(reinterpret_cast<const char*>(p.var_jobs.data()), p.var_jobs.size() * sizeof(SighashVarJob))
                : py::bytes(reinterpret_cast<const char*>(p.jobs.data()), p.jobs.size() * sizeof(SighashJob)),
            py::bytes(reinterpret_cast<const char*>(p.secp_jobs.data()), p.secp_jobs.size() * sizeof(SecpVerifyJob)),
            p.sig_begin, p.device_jobs, p.host_jobs);
    }, py::arg("results"), py::arg("arena_limit") = py::none(),
       "(mode, arena, SighashSeg table, job table, SecpVerifyJob array, sig_begin, device-hashed count, host-hashed "
       "count) of consecutive blocks' ConnectResults as one batch for ops/sighash.verify_window. mode 0: hashes from "
       "the host (no arena, no job table); 1: defer_sighash (SighashJob table); 2: defer_all_forms (SighashVarJob "
       "table over the segment table). Every index is moved by its block's base; block b owns signatures "
       "[sig_begin[b], sig_begin[b+1]). ValueError on results of different modes; an arena that reaches arena_limit "
       "(default SIG_WINDOW_ARENA_LIMIT) is refused");
    m.def("sig_window_verdicts_model", [](const std::vector<u32>& verdicts, const std::vector<u32>& sig_begin) {
        if (sig_begin.empty()) throw std::invalid_argument("signature window: empty prefix table");
        const std::vector<SigWindowRecord> r =
            sig_window_verdicts_model(verdicts.data(), verdicts.size(), sig_begin.data(), sig_begin.size() - 1);
        return py::bytes(reinterpret_cast<const char*>(r.data()), r.size() * sizeof(SigWindowRecord));
    }, py::arg("verdicts"), py::arg("sig_begin"),
       "host model of sig_window_verdicts: per block (n_valid, n_invalid, n_ask_host, first_not_valid) as 4 "
       "little-endian u32, first_not_valid relative to the block (SIG_WINDOW_NONE if every verdict is 1); a verdict "
       "other than 0, 1 or 2 counts as invalid");
    // ---- CHECKMULTISIG groups (-gpumultisig)
    m.attr("SIG_GROUP_BYTES") = sizeof(SigGroup);
    m.attr("SIG_GROUP_MAX_PAIRS") = SIG_GROUP_MAX_PAIRS;
    auto group_bytes = [](const std::vector<SigGroup>& g) {
        return py::bytes(reinterpret_cast<const char*>(g.data()), g.size() * sizeof(SigGroup));
    };
    auto group_table = [](const py::bytes& table) {
        const std::string t = table;
        if (t.size() % sizeof(SigGroup)) throw std::invalid_argument("group table is not a whole number of records");
        std::vector<SigGroup> g(t.size() / sizeof(SigGroup));
        if (!t.empty()) std::memcpy(g.data(), t.data(), t.size());
        return g;
    };
    cr.def_property_readonly("sig_groups", [](const ConnectResult& r) {
        py::list out;
        for (const SigGroupRec& g : r.sig_groups) out.append(py::make_tuple(g.first, g.n_sigs, g.n_keys));
        return out;
    }, "with defer_multisig: (first, n_sigs, n_keys) of every CHECKMULTISIG taken as a group, ascending and disjoint: "
       "entry first + a * w + d of the deferred signatures is signature a against key a + d, w = n_keys - n_sigs + 1")
        .def("sig_group_table", [group_bytes](const ConnectResult& r) { return group_bytes(sig_group_table(r)); },
             "sig_groups as packed SigGroup records (first, n_sigs, n_keys, 0: 4 little-endian u32 each)");
    m.def("sig_window_groups", [group_bytes](const py::list& results) {
        std::vector<const ConnectResult*> rs;
        for (auto r : results) rs.push_back(&r.cast<const ConnectResult&>());
        return group_bytes(sig_window_groups(rs));
    }, py::arg("results"),
       "the group table of consecutive blocks' ConnectResults as one batch: every `first` moved by its block's "
       "signature base, the prefix sig_window_pack reports as sig_begin");
    m.def("sig_group_check", [group_table](size_t n_verdicts, const py::bytes& table) {
        const std::vector<SigGroup> g = group_table(table);
        sig_group_check(n_verdicts, g.data(), g.size());
    }, py::arg("n_verdicts"), py::arg("table"),
       "ValueError on a truncated table, a group with n_sigs = 0, n_sigs > n_keys, n_keys > 20, more than "
       "SIG_GROUP_MAX_PAIRS pairs or entries past n_verdicts, and on groups that overlap or descend");
    m.def("sig_group_resolve_model", [group_table](std::vector<u32> verdicts, const py::bytes& table) {
        const std::vector<SigGroup> g = group_table(table);
        sig_group_resolve_model(verdicts.data(), verdicts.size(), g.data(), g.size());
        return verdicts;
    }, py::arg("verdicts"), py::arg("table"),
       "host model of sig_group_resolve: CHECKMULTISIG's walk over each group's verdicts (anything but 1 or 2 is a "
       "failed check), all of the group's entries rewritten to 1 (the walk succeeds), 0 (it fails) or 2 (it read a "
       "2: the host decides); entries outside groups unchanged. Checks the table first");
    m.def("connect_block", [](const Block& block, int height, CoinsView& view, bool check_scripts, bool defer_sigs,
                              py::object mtp_at, int64_t block_mtp, u32 flags, int threads, assets::State* asset_state,
                              const assets::Flags& asset_flags, const py::bytes& block_hash, bool sigcache,
                              bool defer_sighash, bool defer_all_forms, bool defer_multisig, bool script_cache) {
        ConnectOptions opt;
        opt.script_cache = script_cache;
        opt.defer_sighash = defer_sighash;
        opt.defer_all_forms = defer_all_forms;
        opt.defer_multisig = defer_multisig;
        opt.assets = asset_state;
        opt.asset_flags = asset_flags;
        const std::string bh = block_hash;
        if (bh.size() == 32) opt.block_hash = Uint256::from_bytes(reinterpret_cast<const u8*>(bh.data()));
        opt.script_flags = flags;
        opt.check_scripts = check_scripts;
        opt.defer_sigs = defer_sigs;
        opt.sigcache = sigcache;
        opt.block_mtp = block_mtp;
        opt.threads = threads;
        if (!mtp_at.is_none())
            opt.mtp_at = [mtp_at](int h) {
                py::gil_scoped_acquire gil;
                return mtp_at(h).cast<int64_t>();
            };
        BlockUndo undo;
        ConnectResult r;
        Bytes ub;
        {
            py::gil_scoped_release rel;  // the UTXO pass and the script-check threads run without the GIL
            r = connect_block(block, height, view, opt, undo);
            if (r.ok) ub = serialize_block_undo(undo);
        }
        return py::make_tuple(std::move(r), pyb(ub));
    }, py::arg("block"), py::arg("height"), py::arg("view"), py::arg("check_scripts") = true,
       py::arg("defer_sigs") = false, py::arg("mtp_at") = py::none(), py::arg("block_mtp") = 0,
       py::arg("flags") = kBlockScriptFlags, py::arg("threads") = 1, py::arg("assets") = nullptr,
       py::arg("asset_flags") = assets::Flags{}, py::arg("block_hash") = py::bytes(), py::arg("sigcache") = true,
       py::arg("defer_sighash") = false, py::arg("defer_all_forms") = false, py::arg("defer_multisig") = false,
       py::arg("script_cache") = false,
       "ConnectBlock against the view -> (ConnectResult, serialized CBlockUndo); the view is unchanged on failure. "
       "script_cache: a transaction whose (wtxid, flags) is in the script-execution cache gets no script check, no "
       "deferred signature and no template or forms entry; its block index is listed in "
       "ConnectResult.script_cache_txs and nothing is erased here. "
       "defer_multisig (with defer_sigs only): a CHECKMULTISIG whose outcome depends on its pair verdicts alone leaves "
       "every candidate (signature, key) pair among the deferred signatures and a record in ConnectResult.sig_groups; "
       "those entries neither consult nor erase the signature cache. "
       "defer_sighash (with defer_sigs only): the legacy SIGHASH_ALL-form message hashes are left to the batch too "
       "(ConnectResult.sighash_pack); those signatures are not looked up in the signature cache, whose key is the "
       "message, so their entries age out of the bounded cache instead of being erased on use. defer_all_forms (with "
       "defer_sighash only): every form of both signature versions is left to the batch "
       "(ConnectResult.sighash_pack_var), and the same holds for the witness signatures' cache entries. With "
       "-scriptcache=1 (script_cache) a transaction the mempool verified is skipped as a whole, which is what spares "
       "those signatures");
    m.def("disconnect_block", [](const Block& block, const py::bytes& undo, CoinsView& view, assets::State* st,
                                 const py::bytes& asset_undo) {
        const Bytes au = bytes_of(asset_undo);
        return disconnect_block(block, deserialize_block_undo(bytes_of(undo)), view, st, &au);
    }, py::arg("block"), py::arg("undo"), py::arg("view"), py::arg("assets") = nullptr, py::arg("asset_undo") = py::bytes(),
       "DisconnectBlock with its undo data: False if they did not match the view (it is still reverted)");
    py::class_<ChainIndexes, std::shared_ptr<ChainIndexes>>(m, "ChainIndexes")
        .def(py::init([](bool tx, bool addr, bool spent, bool ts) {
                 auto x = std::make_shared<ChainIndexes>();
                 x->txindex = tx;
                 x->addressindex = addr;
                 x->spentindex = spent;
                 x->timestampindex = ts;
                 return x;
             }),
             py::arg("txindex") = false, py::arg("addressindex") = false, py::arg("spentindex") = false,
             py::arg("timestampindex") = false)
        .def_readonly("txindex", &ChainIndexes::txindex)
        .def_readonly("addressindex", &ChainIndexes::addressindex)
        .def_readonly("spentindex", &ChainIndexes::spentindex)
        .def_readonly("timestampindex", &ChainIndexes::timestampindex)
        .def_property("best_block", [](const ChainIndexes& x) { return pyb(x.best_block.data, 32); },
                      [](ChainIndexes& x, const py::bytes& b) {
                          const std::string h = b;
                          need32(h, "best_block");
                          x.best_block = Uint256::from_bytes(reinterpret_cast<const u8*>(h.data()));
                      })
        .def("connect", [](ChainIndexes& x, const Block& b, int height, const py::bytes& hash, const py::bytes& undo,
                           int file, u32 data_pos) {
            const std::string h = hash;
            need32(h, "hash");
            x.connect(b, height, Uint256::from_bytes(reinterpret_cast<const u8*>(h.data())),
                      deserialize_block_undo(bytes_of(undo)), file, data_pos);
        }, py::arg("block"), py::arg("height"), py::arg("hash"), py::arg("undo"), py::arg("file") = -1,
           py::arg("data_pos") = 0)
        .def_readwrite("journal", &ChainIndexes::journal)
        .def_property_readonly("pending_changes", &ChainIndexes::pending_changes)
        .def("disconnect", [](ChainIndexes& x, const Block& b, int height, const py::bytes& hash, const py::bytes& undo) {
            const std::string h = hash;
            need32(h, "hash");
            x.disconnect(b, height, Uint256::from_bytes(reinterpret_cast<const u8*>(h.data())),
                         deserialize_block_undo(bytes_of(undo)));
        })
        .def("tx_block", [](const ChainIndexes& x, const py::bytes& txid) -> py::object {
            const std::string t = txid;
            need32(t, "txid");
            const Uint256* b = x.tx_block(Uint256::from_bytes(reinterpret_cast<const u8*>(t.data())));
            if (!b) return py::none();
            return pyb(b->data, 32);
        })
        .def("deltas", [](const ChainIndexes& x, int type, const py::bytes& h160, const std::string& asset, int start,
                          int end) {
            const std::string h = h160;
            if (h.size() != 20) throw std::invalid_argument("hash160 must be 20 bytes");
            py::list out;
            for (auto& [name, d] : x.deltas(type, reinterpret_cast<const u8*>(h.data()), asset, start, end))
                out.append(py::make_tuple(name, d.height, d.tx_index, pyb(d.txid.data, 32), d.index, d.spending, d.amount));
            return out;
        }, py::arg("type"), py::arg("hash160"), py::arg("asset") = "CLORE", py::arg("start") = 0, py::arg("end") = 0,
           "[(asset, height, tx index, txid, index, spending, amount)] in chain order")
        .def("unspent", [](const ChainIndexes& x, int type, const py::bytes& h160, const std::string& asset) {
            const std::string h = h160;
            if (h.size() != 20) throw std::invalid_argument("hash160 must be 20 bytes");
            py::list out;
            for (auto& [name, u] : x.unspent(type, reinterpret_cast<const u8*>(h.data()), asset))
                out.append(py::make_tuple(name, pyb(u.txid.data, 32), u.index, u.amount, pyb(u.script), u.height));
            return out;
        }, py::arg("type"), py::arg("hash160"), py::arg("asset") = "CLORE",
           "[(asset, txid, index, amount, script, height)] by height")
        .def("spent", [](const ChainIndexes& x, const py::bytes& txid, u32 n) -> py::object {
            const std::string t = txid;
            need32(t, "txid");
            const SpentInfo* s = x.spent(Uint256::from_bytes(reinterpret_cast<const u8*>(t.data())), n);
            if (!s) return py::none();
            return py::make_tuple(pyb(s->txid.data, 32), s->input, s->height, s->amount, s->addr_type, pyb(s->h160, 20));
        })
        .def("timestamps", [](const ChainIndexes& x, u32 low, u32 high) {
            py::list out;
            for (auto& h : x.timestamps(low, high)) out.append(pyb(h.data, 32));
            return out;
        })
        .def("serialize", [](const ChainIndexes& x) { return pyb(x.serialize()); })
        .def("deserialize", [](ChainIndexes& x, const py::bytes& b) { return x.deserialize(bytes_of(b)); });
    m.def("verify_input_host", [](const Block& block, u32 tx_index, u32 n_in, int64_t value, const py::bytes& spk,
                                  u32 flags) {
        if (tx_index >= block.vtx.size() || n_in >= block.vtx[tx_index].vin.size())
            throw std::invalid_argument("no such input");
        Coin c;
        c.out.value = value;
        c.out.script_pubkey = bytes_of(spk);
        ScriptError err = ScriptError::UNKNOWN_ERROR;
        const bool ok = verify_input_host(block.vtx[tx_index], n_in, c, flags, &err);
        return py::make_tuple(ok, script_error_name(err));
    });
    m.def("block_undo_coin", [](const py::bytes& undo, u32 tx_index, u32 n_in) {
        const BlockUndo u = deserialize_block_undo(bytes_of(undo));
        if (tx_index == 0 || tx_index > u.vtxundo.size() || n_in >= u.vtxundo[tx_index - 1].prev.size())
            throw std::invalid_argument("no such spent coin in the undo data");
        const Coin& c = u.vtxundo[tx_index - 1].prev[n_in];
        return py::make_tuple(c.out.value, pyb(c.out.script_pubkey), c.height, c.coinbase);
    }, "the coin input n_in of transaction tx_index spent, from a block's undo data");
    m.def("block_undo_roundtrip", [](const py::bytes& b) {
        return pyb(serialize_block_undo(deserialize_block_undo(bytes_of(b))));
    });
    m.def("compress_amount", &compress_amount);
    m.def("decompress_amount", &decompress_amount);
    m.def("tx_legacy_sigops", [](const py::bytes& tx_raw) { return tx_legacy_sigops(tx_of(tx_raw)); },
          "GetLegacySigOpCount of a transaction (no spent outputs needed)");
    m.def("tx_sigop_cost", [](const py::bytes& tx_raw, const std::vector<py::bytes>& spent_spks, u32 flags) {
        const Transaction tx = tx_of(tx_raw);
        std::vector<Coin> coins(spent_spks.size());
        std::vector<const Coin*> ptrs;
        for (size_t i = 0; i < spent_spks.size(); ++i) {
            coins[i].out.script_pubkey = bytes_of(spent_spks[i]);
            ptrs.push_back(&coins[i]);
        }
        return tx_sigop_cost(tx, ptrs, flags);
    }, "GetTransactionSigOpCost: legacy x4 + P2SH redeem x4 + witness, given the spent scriptPubKeys");

    m.def("script_is_push_only", [](const py::bytes& s) { return script_is_push_only(bytes_of(s)); });
    m.def("is_valid_signature_encoding", [](const py::bytes& s) { return is_valid_signature_encoding(bytes_of(s)); });
}
