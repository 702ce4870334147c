// Script evaluation and transaction signature checking.
//
// Parity: EvalScript / VerifyScript / VerifyWitnessProgram (src/script/interpreter.cpp:289,1546),
// SignatureHash legacy + BIP143 (interpreter.cpp:1150-1380), TransactionSignatureChecker (CheckSig /
// CheckLockTime / CheckSequence), CScriptNum (src/script/script.h:221-340), the BIP66 DER and
// low-S rules, FindAndDelete, and Clore's OP_CLORE_ASSET (0xc0): GetOp returns everything after it
// as one data element (src/script/script.h:580-586) and EvalScript treats it as a no-op
// (interpreter.cpp:1119-1121). Flags and error names are the reference's
// (src/script/interpreter.h:39-114, script_error.h), so src/test/data/script_tests.json,
// sighash.json and tx_valid.json / tx_invalid.json run unchanged (tests/test_script.py).
//
// Signatures go through a SigChecker. The default checks each one on the host (secp256k1.cpp);
// block validation collects them in a batch for the GPU (hip/kernels/secp256k1_verify.hip) by
// running the scripts with a deferring checker (see ScriptCheckBatch).
#pragma once

#include <functional>
#include <string>
#include <vector>

#include "primitives.hpp"

namespace nodexa {

enum ScriptFlags : u32 {
    SCRIPT_VERIFY_NONE = 0,
    SCRIPT_VERIFY_P2SH = 1u << 0,
    SCRIPT_VERIFY_STRICTENC = 1u << 1,
    SCRIPT_VERIFY_DERSIG = 1u << 2,
    SCRIPT_VERIFY_LOW_S = 1u << 3,
    SCRIPT_VERIFY_NULLDUMMY = 1u << 4,
    SCRIPT_VERIFY_SIGPUSHONLY = 1u << 5,
    SCRIPT_VERIFY_MINIMALDATA = 1u << 6,
    SCRIPT_VERIFY_DISCOURAGE_UPGRADABLE_NOPS = 1u << 7,
    SCRIPT_VERIFY_CLEANSTACK = 1u << 8,
    SCRIPT_VERIFY_CHECKLOCKTIMEVERIFY = 1u << 9,
    SCRIPT_VERIFY_CHECKSEQUENCEVERIFY = 1u << 10,
    SCRIPT_VERIFY_WITNESS = 1u << 11,
    SCRIPT_VERIFY_DISCOURAGE_UPGRADABLE_WITNESS_PROGRAM = 1u << 12,
    SCRIPT_VERIFY_MINIMALIF = 1u << 13,
    SCRIPT_VERIFY_NULLFAIL = 1u << 14,
    SCRIPT_VERIFY_WITNESS_PUBKEYTYPE = 1u << 15,
};
// MANDATORY_SCRIPT_VERIFY_FLAGS / STANDARD_SCRIPT_VERIFY_FLAGS (src/policy/policy.h)
constexpr u32 kMandatoryScriptFlags = SCRIPT_VERIFY_P2SH;
constexpr u32 kStandardScriptFlags =
    SCRIPT_VERIFY_P2SH | SCRIPT_VERIFY_DERSIG | SCRIPT_VERIFY_STRICTENC | SCRIPT_VERIFY_MINIMALDATA |
    SCRIPT_VERIFY_NULLDUMMY | SCRIPT_VERIFY_DISCOURAGE_UPGRADABLE_NOPS | SCRIPT_VERIFY_CLEANSTACK |
    SCRIPT_VERIFY_MINIMALIF | SCRIPT_VERIFY_NULLFAIL | SCRIPT_VERIFY_CHECKLOCKTIMEVERIFY |
    SCRIPT_VERIFY_CHECKSEQUENCEVERIFY | SCRIPT_VERIFY_LOW_S | SCRIPT_VERIFY_WITNESS |
    SCRIPT_VERIFY_DISCOURAGE_UPGRADABLE_WITNESS_PROGRAM | SCRIPT_VERIFY_WITNESS_PUBKEYTYPE;

enum class ScriptError {
    OK, UNKNOWN_ERROR, EVAL_FALSE, OP_RETURN, SCRIPT_SIZE, PUSH_SIZE, OP_COUNT, STACK_SIZE, SIG_COUNT,
    PUBKEY_COUNT, VERIFY, EQUALVERIFY, CHECKMULTISIGVERIFY, CHECKSIGVERIFY, NUMEQUALVERIFY, BAD_OPCODE,
    DISABLED_OPCODE, INVALID_STACK_OPERATION, INVALID_ALTSTACK_OPERATION, UNBALANCED_CONDITIONAL,
    NEGATIVE_LOCKTIME, UNSATISFIED_LOCKTIME, SIG_HASHTYPE, SIG_DER, MINIMALDATA, SIG_PUSHONLY, SIG_HIGH_S,
    SIG_NULLDUMMY, PUBKEYTYPE, CLEANSTACK, MINIMALIF, NULLFAIL, DISCOURAGE_UPGRADABLE_NOPS,
    DISCOURAGE_UPGRADABLE_WITNESS_PROGRAM, WITNESS_PROGRAM_WRONG_LENGTH, WITNESS_PROGRAM_WITNESS_EMPTY,
    WITNESS_PROGRAM_MISMATCH, WITNESS_MALLEATED, WITNESS_MALLEATED_P2SH, WITNESS_UNEXPECTED,
    WITNESS_PUBKEYTYPE,
};
const char* script_error_name(ScriptError e);

enum class SigVersion { BASE = 0, WITNESS_V0 = 1 };

enum SigHashType : int { SIGHASH_ALL = 1, SIGHASH_NONE = 2, SIGHASH_SINGLE = 3, SIGHASH_ANYONECANPAY = 0x80 };

// Script limits (src/script/script.h:28-44)
constexpr size_t kMaxScriptElementSize = 520;
constexpr int kMaxOpsPerScript = 201;
constexpr int kMaxPubkeysPerMultisig = 20;
constexpr size_t kMaxScriptSize = 10000;
constexpr size_t kMaxStackSize = 1000;
constexpr u32 kLocktimeThreshold = 500000000;
constexpr u8 OP_CLORE_ASSET = 0xc0;

// One opcode (and its push data) at `pc`; false on a truncated push (GetScriptOp).
bool script_get_op(const Bytes& s, size_t& pc, u8& opcode, Bytes* data);
bool script_is_push_only(const Bytes& s);
bool script_is_p2sh(const Bytes& s);
bool script_is_witness_program(const Bytes& s, int& version, Bytes& program);
// Legacy sigop count (GetSigOpCount(false)) and the accurate P2SH form over the redeem script.
unsigned script_sigop_count(const Bytes& s, bool accurate);

// BIP143 midstate hashes of one transaction (PrecomputedTransactionData).
struct PrecomputedTx {
    Uint256 prevouts, sequence, outputs;
    bool ready = false;
    explicit PrecomputedTx(const Transaction& tx);
    PrecomputedTx() = default;
};

Uint256 signature_hash(const Bytes& script_code, const Transaction& tx, unsigned n_in, int hash_type, Amount amount,
                       SigVersion sigversion, const PrecomputedTx* cache = nullptr);

// The legacy (SigVersion::BASE) message hash in its SIGHASH_ALL form, split so that a batch can
// compute it elsewhere (ops/sighash, hip/kernels/sighash.hip): one template per transaction, and
// per signature only the script code bytes and the hash type.
// The template is the legacy serialisation with every input script empty (version, compact size
// of vin, 41 bytes per input, outputs, locktime); script_off[i] is the offset of input i's
// script-length byte (a single 0x00). The preimage of input i is
//   T[0:off_i] | sighash_script_code(code) | T[off_i+1:] | hash type as LE int32.
struct SighashTemplate {
    Bytes bytes;
    std::vector<u32> script_off;
    SighashTemplate() = default;
    explicit SighashTemplate(const Transaction& tx);
};
// What signature_hash writes for the signed input's script: compact size, then the code with its
// OP_CODESEPARATORs removed (with the reference's quirks: see signature_hash).
Bytes sighash_script_code(const Bytes& script_code);
// True for the signatures whose legacy hash has the SIGHASH_ALL form: no ANYONECANPAY, and a base
// type that is neither NONE nor SINGLE (so also the odd types 0x00, 0x04, 0x21 ..., which the
// reference hashes as ALL with the literal type appended).
inline bool sighash_all_form(SigVersion sv, int hash_type) {
    const int base = hash_type & 0x1f;
    return sv == SigVersion::BASE && !(hash_type & 0x80) && base != 2 && base != 3;
}
// SHA256d of the preimage above: equals signature_hash for every sighash_all_form signature.
Uint256 sighash_from_template(const SighashTemplate& t, unsigned n_in, const Bytes& emitted_code, int32_t hash_type);

// Every form of both signature versions, for the batch that hashes them all (defer_all_forms;
// hip/kernels/sighash_var.hip). "all", "none", "single", each with "|acp" under ANYONECANPAY; the
// odd base types count as "all", as the reference hashes them.
const char* sighash_form(SigVersion sv, int hash_type);
// What a batch needs of one transaction to lay out any of its signature hashes: the template, where
// its outputs lie in it (out_off has vout.size() + 1 entries: each output's start, then the
// lock time's; outs_off is the output count's compact size) and the BIP143 midstate hashes.
struct SighashTxForms {
    SighashTemplate t;
    u32 outs_off = 0;
    std::vector<u32> out_off;
    PrecomputedTx pre;
    SighashTxForms() = default;
    explicit SighashTxForms(const Transaction& tx);
    size_t n_in() const { return t.script_off.size(); }
    size_t n_out() const { return out_off.size() - 1; }
};
// Whether defer_all_forms leaves this hash to the batch: everything but the legacy hashes whose
// message is the constant one (input index past vin, or SINGLE without a matching output), which
// have nothing to hash.
inline bool sighash_deferrable(size_t n_vin, size_t n_vout, unsigned n_in, int hash_type, SigVersion sv) {
    if (n_in >= n_vin) return false;
    return sv == SigVersion::WITNESS_V0 || (hash_type & 0x1f) != SIGHASH_SINGLE || n_in < n_vout;
}
// The emitted script code of a deferred hash: sighash_script_code for a legacy signature, the
// compact size and the code unchanged for witness v0.
Bytes sighash_emitted_code(const Bytes& script_code, SigVersion sv);
// signature_hash from the recorded pieces alone; legacy needs n_in < vin.size(), and SINGLE
// n_in < vout.size() (the constant-one cases are never deferred).
Uint256 sighash_from_forms(const SighashTxForms& f, unsigned n_in, const Bytes& emitted_code, int32_t hash_type,
                           Amount amount, SigVersion sv);

// Signature / locktime oracle used by EvalScript.
class SigChecker {
public:
    virtual ~SigChecker() = default;
    virtual bool check_sig(const Bytes& sig, const Bytes& pubkey, const Bytes& script_code, SigVersion sv) const {
        (void)sig; (void)pubkey; (void)script_code; (void)sv;
        return false;
    }
    virtual bool check_lock_time(int64_t n) const { (void)n; return false; }
    virtual bool check_sequence(int64_t n) const { (void)n; return false; }
    // CHECKMULTISIG under a deferring checker (TxSigChecker::defer_multisig). groups_multisig: whether
    // the checker takes groups at all. defer_multisig_group: record every candidate pair of the
    // opcode's walk (sigs[0] is the signature on top of the stack, keys[0] the last key of the
    // script; every signature is non-empty and well encoded, every key passed the encoding rule) and
    // answer true, or answer false and record nothing: the caller then walks as usual.
    virtual bool groups_multisig() const { return false; }
    virtual bool defer_multisig_group(const std::vector<const Bytes*>& sigs, const std::vector<const Bytes*>& keys,
                                      const Bytes& script_code, SigVersion sv) const {
        (void)sigs; (void)keys; (void)script_code; (void)sv;
        return false;
    }
};

// A signature check deferred for a batch: message hash, DER signature (hash type stripped) and
// public key, as the GPU batch verifier takes them.
struct PendingSig {
    Uint256 msg;
    Bytes sig;
    Bytes pubkey;
    // With defer_sighash, a sighash_all_form signature leaves `msg` unset and carries what the
    // batch needs to compute it: its place in the block, the full hash type and the emitted
    // script code (sighash_script_code).
    bool device_hash = false;
    u32 tx_index = 0, n_in = 0;
    int32_t hash_type = 0;
    Bytes code;
    // With defer_all_forms every hash is left out (sighash_emitted_code in `code`), of both
    // signature versions; witness v0 commits to the spent amount.
    SigVersion sigversion = SigVersion::BASE;
    Amount amount = 0;
};

// One CHECKMULTISIG taken as a group (defer_multisig): n_sigs signatures against n_keys keys as
// n_sigs * w consecutive PendingSig entries from `first`, w = n_keys - n_sigs + 1; entry
// first + a * w + d is signature a against key a + d (a = 0: the signature on top of the stack,
// key 0: the last key of the script), the only pairs the opcode's walk can reach.
struct SigGroupRec {
    u32 first, n_sigs, n_keys;
};
constexpr u32 kSigGroupMaxPairs = 64;  // SIG_GROUP_MAX_PAIRS (hip/kernels/kernel_params.h)

class TxSigChecker : public SigChecker {
public:
    TxSigChecker(const Transaction* tx, unsigned n_in, Amount amount, const PrecomputedTx* cache = nullptr)
        : tx_(tx), n_in_(n_in), amount_(amount), cache_(cache) {}
    bool check_sig(const Bytes& sig, const Bytes& pubkey, const Bytes& script_code, SigVersion sv) const override;
    bool check_lock_time(int64_t n) const override;
    bool check_sequence(int64_t n) const override;
    // Batch mode: check_sig records the signature in `pending` and answers true (the caller
    // re-runs the input on the host if the batch rejects any of its signatures). Only
    // valid for scripts whose outcome cannot depend on a signature failing, i.e. for blocks,
    // where any failing signature invalidates the block anyway.
    std::vector<PendingSig>* pending = nullptr;
    // With `pending`: leave the message hash of sighash_all_form signatures to the batch too.
    // Those signatures are not looked up in the signature cache (its key is the message).
    bool defer_sighash = false;
    // With defer_sighash: leave the hash of every signature of both versions to the batch, except
    // the legacy hashes whose message is the constant one (nothing to hash).
    bool defer_all_forms = false;
    u32 tx_index = 0;  // the transaction's index in its block, recorded in deferred hashes
    // With `pending` and `groups`: a CHECKMULTISIG whose outcome depends on the pair verdicts alone
    // (no encoding error can arise on any walk, at most kSigGroupMaxPairs pairs) records all its
    // candidate pairs and one SigGroupRec, and the batch runs the pairing walk over their verdicts
    // (chain/sighash.hpp sig_group_resolve_model). Group entries neither consult nor erase the
    // signature cache.
    bool defer_multisig = false;
    std::vector<SigGroupRec>* groups = nullptr;
    bool groups_multisig() const override { return pending && groups && defer_multisig; }
    bool defer_multisig_group(const std::vector<const Bytes*>& sigs, const std::vector<const Bytes*>& keys,
                              const Bytes& script_code, SigVersion sv) const override;
    // Signature cache (sigcache.hpp): STORE remembers every signature that verifies (mempool
    // acceptance); USE answers from the cache first and erases what it hits (block validation,
    // CachingTransactionSignatureChecker with store = false).
    enum class CacheMode : u8 { NONE, STORE, USE };
    CacheMode sigcache = CacheMode::NONE;

protected:
    // The entry of a signature whose hash is left to the batch under the flags in force (`sig`
    // without its hash type); false if the message is computed on the host.
    bool deferred_entry(const Bytes& sig, const Bytes& pubkey, const Bytes& script_code, SigVersion sv, int hash_type,
                        PendingSig& p) const;
    const Transaction* tx_;
    unsigned n_in_;
    Amount amount_;
    const PrecomputedTx* cache_;
};

bool eval_script(std::vector<Bytes>& stack, const Bytes& script, u32 flags, const SigChecker& checker,
                 SigVersion sv, ScriptError* err);
bool verify_script(const Bytes& script_sig, const Bytes& script_pubkey, const std::vector<Bytes>* witness, u32 flags,
                   const SigChecker& checker, ScriptError* err);

// Context-free transaction checks (CheckTransaction, src/consensus/tx_verify.cpp:169; the asset
// null-data rules are not included). Returns "" or the reference's reject reason.
// CheckTransaction. With `asset_params`, also the asset rules of CheckTransaction (assets.hpp),
// under the given deployment flags (block_check: called from CheckBlock; mempool_check: from ATMP).
namespace assets {
struct Params;
struct Flags;
}  // namespace assets
std::string check_transaction(const Transaction& tx, bool check_duplicate_inputs = true,
                              const assets::Params* asset_params = nullptr, const assets::Flags* flags = nullptr,
                              bool block_check = false, bool mempool_check = false);
constexpr Amount kMaxMoney = Amount(1300000000) * COIN;  // src/amount.h:29

// DER / pubkey encoding rules exposed for tests and policy.
bool is_valid_signature_encoding(const Bytes& sig);
bool is_low_der_signature(const Bytes& sig);
bool is_compressed_or_uncompressed_pubkey(const Bytes& pk);

}  // namespace nodexa
