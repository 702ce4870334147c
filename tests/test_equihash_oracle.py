"""The CPU Equihash(200,9) verifier (csrc/pow/equihash.cpp equihash_verify) against the independent
oracle of tests/equihash_oracle.py, on solutions that only one rule rejects.

A corruption of a valid solution leaves a non-zero root with probability ~1, so it is rejected
whatever else the verifier forgets. The cases here are the ones a forgetful verifier accepts:
tests/data/equihash_adversarial.json holds mined solutions whose single fault is one bit of one
level's own digit (or of the root's last 40 bits), and equihash_oracle.derived_cases adds swapped
children (order alone) and repeats under a zero root (duplicate alone above order). The GPU
verifiers see the same cases in tests/test_gpu_equihash_verify.py."""
import os
import re

import pytest

import equihash_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixtures():
    return O.load_fixtures()


@pytest.fixture(scope="module")
def cases(fixtures):
    return fixtures + O.derived_cases(fixtures)


@pytest.fixture(scope="module")
def params(core):
    return core.EquihashParams(200, 9)


# ------------------------------------------------------------------ the oracle itself
def test_oracle_packing_known_answers():
    # 21-bit big-endian fields: index 1 first = bit 20 of the stream, i.e. 0x08 in byte 2
    assert O.pack([1] + [0] * 7) == bytes([0, 0, 0x08]) + bytes(18)
    assert O.pack([0] * 7 + [1]) == bytes(20) + bytes([1])
    assert O.pack([0x1FFFFF, 0] + [0] * 6)[:6] == bytes([0xFF, 0xFF, 0xF8, 0, 0, 0])
    # the second field ends at stream bit 41 = 0x40 of byte 5
    assert O.pack([0x100000, 0x000001] + [0] * 6)[:6] == bytes([0x80, 0, 0, 0, 0, 0x40])
    idx = [(i * 40961 + 7) % O.LEAVES for i in range(512)]
    assert len(O.pack(idx)) == O.SOL_BYTES == 1344 and O.unpack(O.pack(idx)) == idx


def test_oracle_numbering_is_the_kernels():
    text = open(os.path.join(ROOT, "nodexa_chain_core_amd", "hip", "kernels", "kernel_params.h")).read()
    header = {m[0]: int(m[1]) for m in re.findall(r"#define EQ_V_(\w+) (\d+)", text)}
    assert header == {"EMPTY": O.CODE_EMPTY, "OK": O.CODE_OK, **{k.upper(): v for k, v in O.CODES.items()}}
    assert O.expected_code(set()) == 0
    assert O.expected_code({"collision", "order"}) == 2
    assert O.expected_code({"collision", "order", "duplicate"}) == 3
    assert O.expected_code({"order", "duplicate", "nonzero"}) == 4


# ------------------------------------------------------------------ the fixture file
def test_fixture_rules_are_current(fixtures):
    """The stored rule sets are the oracle's of today, and each class is what its label says."""
    want = {"valid": frozenset(), "duplicate": frozenset({"duplicate"})}
    for c in fixtures:
        assert frozenset(O.failed_rules(c.inp, c.indices)) == c.recorded, c
        if c.cls == "defect":
            assert c.recorded == ({"nonzero"} if c.level == 9 else {"collision"}), c
        else:
            assert c.recorded == want[c.cls], c


def test_fixture_classes_complete(fixtures):
    """Every class of the table has a fixture, and a defect fixture's fault is the one bit of its
    label: at level l the first 20 l bits (all 200 at the root) of every node's XOR are zero but for
    bit b, which at least one node has set; b lies in the level's own digit."""
    have = {(c.level, c.bit) for c in fixtures if c.cls == "defect"}
    missing = [cb for cb in O.DEFECT_CLASSES if cb not in have]
    assert not missing, f"no fixture for (level, bit) {missing}"
    assert len(O.DEFECT_CLASSES) == 28
    for c in fixtures:
        if c.cls != "defect":
            continue
        lo, hi = (160, 200) if c.level == 9 else (20 * (c.level - 1), 20 * c.level)
        assert lo <= c.bit < hi, c
        heads = {x >> (O.N - hi) for x in O.level_xors(c.inp, c.indices, c.level)}
        assert heads - {0} == {1 << (hi - 1 - c.bit)}, c
    valid = [c for c in fixtures if c.cls == "valid"]
    lengths = sorted(len(c.inp) for c in valid)
    missing = [n for n in O.VALID_LENGTHS if n not in lengths]
    assert not missing, f"no valid solution for input length {missing}"
    two = [c for c in valid if len(c.inp) == 112]
    assert len(two) >= 2 and two[0].inp == two[1].inp and two[0].indices != two[1].indices


def test_derived_cases_are_what_they_claim(fixtures):
    derived = O.derived_cases(fixtures)
    by = {}
    for c in derived:
        by.setdefault(c.cls, []).append(c)
    nvalid = sum(c.cls == "valid" for c in fixtures)
    assert len(by["order"]) == 31 * nvalid      # levels 1..7: 4 nodes, level 8: 2, level 9: 1
    assert len(by["dup"]) == 4 * nvalid
    assert len(by["graft"]) == 9
    alone = set()
    for c in by["order"]:
        assert c.rules == {"order"}, c
        level, j = (int(x[1:]) for x in c.name.split("@")[0].split("-")[1:])
        fails = O.order_failures(c.indices)
        assert (level, j) in fails, c
        if j & 1 or level == 9:
            # under a right child no ancestor's first index moves: this node's test alone rejects it
            assert fails == [(level, j)], c
            alone.add((len(c.inp), level))
    assert alone == {(n, level) for n in O.VALID_LENGTHS for level in range(1, 10)}
    for c in by["dup"]:
        assert "duplicate" in c.rules and "nonzero" not in c.rules and c.code == 3, c
    for c in by["graft"] + by["flip"] + by["input"]:
        assert c.rules, c
    assert len({(c.inp, tuple(c.indices)) for c in derived}) == len(derived)


# ------------------------------------------------------------------ the CPU verifier
def test_cpu_verifier_agrees_with_oracle(core, params, cases):
    accepted = 0
    for c in cases:
        ok, why = core.equihash_verify(params, c.inp, c.indices)
        assert ok == (not c.rules), (c, why, sorted(c.rules))
        if len(c.rules) == 1:
            assert why == next(iter(c.rules)), c
        if ok:
            assert why == ""
            accepted += 1
    assert accepted == 6 and len(cases) > 200


def test_pack_unpack_agree_with_oracle(core, params, fixtures):
    lists = [c.indices for c in fixtures]
    lists += [[O.LEAVES - 1] * 512, [0] * 512, [(0x155555, 0x0AAAAA)[i & 1] for i in range(512)],
              [1 << (i % 21) for i in range(512)]]
    for idx in lists:
        packed = O.pack(idx)
        assert core.equihash_pack(params, idx) == packed
        assert core.equihash_unpack(params, packed) == idx == O.unpack(packed)


def test_valid_fixtures_are_the_cpu_solvers(core, params, fixtures):
    """The mined valid solutions of the 112-byte input and of the 119-byte one (leaf counter across
    two message words) are among the solutions the project's own CPU solver finds."""
    for length in (112, 119):
        vs = [c for c in fixtures if c.cls == "valid" and len(c.inp) == length]
        found, _ = core.equihash_solve_cpu(params, vs[0].inp, 64, 0)
        for c in vs:
            assert c.indices in found, c
