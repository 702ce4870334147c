"""The gfx950 Equihash(200,9) verifiers (hip/kernels/equihash.hip: eq_verify over packed solutions,
eq_verify_slots over the solver's output buffer) against the independent oracle of
tests/equihash_oracle.py: every verdict code, on solutions that only one rule rejects.

The cases are those of tests/test_equihash_oracle.py: the mined single-bit defects of
tests/data/equihash_adversarial.json (a prefix mask one bit short, a digit edge or a 32-bit word
left out), swapped children (an order test missing at one level or node), repeats under a zero root
(a duplicate pass that never fires), and inputs of 108, 117, 119 and 124 bytes (the leaf counter at
byte 4 of a message word, across two words, in the last word). One 256-thread workgroup per
solution: the whole file is a handful of launches."""
import random

import pytest

import equihash_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    fixtures = O.load_fixtures()
    return fixtures + O.derived_cases(fixtures)


@pytest.fixture(scope="module")
def by_length(cases):
    out = {}
    for c in cases:
        out.setdefault(len(c.inp), []).append(c)
    assert sorted(out) == list(O.VALID_LENGTHS)
    return out


def launch_eq_verify(batch, input_len):
    """eq_verify over `batch` the way ops/equihash.py verify_solutions launches it; the raw codes."""
    import torch

    from nodexa_chain_core_amd.ops import runtime
    from nodexa_chain_core_amd.ops.equihash import blake2b_h0

    h = runtime.hip()
    assert h.EQ_SOL_WORDS * 4 == O.SOL_BYTES
    msgs = bytearray(len(batch) * 128)
    sols = bytearray(len(batch) * O.SOL_BYTES)
    for k, c in enumerate(batch):
        assert len(c.inp) == input_len
        msgs[k * 128:k * 128 + input_len] = c.inp
        sols[k * O.SOL_BYTES:(k + 1) * O.SOL_BYTES] = c.packed
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        kern = runtime.static_kernel("equihash", "eq_verify")
        dm = torch.frombuffer(msgs, dtype=torch.int64).to(dev)
        ds = torch.frombuffer(sols, dtype=torch.int32).to(dev)
        res = torch.full((len(batch),), -1, dtype=torch.int32, device=dev)
        h.launch_equihash_verify(kern, blake2b_h0(), dm.data_ptr(), input_len, len(batch), ds.data_ptr(),
                                 res.data_ptr(), runtime.current_stream_handle())
        return res.cpu().tolist()


@pytest.mark.parametrize("input_len", O.VALID_LENGTHS)
def test_eq_verify_codes_equal_oracle(gpu, by_length, input_len):
    """Every code is the oracle's, whatever a solution's neighbours in the batch are."""
    batch = list(by_length[input_len])
    random.Random(input_len).shuffle(batch)
    want = [c.code for c in batch]
    assert 0 in want and {2, 3} <= set(want)
    if input_len == 112:
        assert {1, 4} <= set(want)
    for order in (batch, batch[::-1]):
        got = launch_eq_verify(order, input_len)
        bad = [(c.name, g, c.code, sorted(c.rules)) for c, g in zip(order, got) if g != c.code]
        assert not bad, bad


def slot_instances(pool, ms):
    """Four instances of the solver's output: (inputs, counts, slots, expected codes). Instance 0
    has the fixtures' first 112-byte input, the others the inputs of the other mined nonces or
    single-byte variants of it. Every instance's 16 slots hold well-formed solutions, its own
    input's cases first; the count says how many of them the kernel may judge."""
    inputs = [next(c.inp for c in pool if c.cls == "valid")]
    for cls in ("defect", "input"):
        for c in pool:
            if c.cls == cls and c.inp not in inputs:
                inputs.append(c.inp)
    assert len(inputs) >= 4
    inputs = inputs[:4]
    counts = [40, ms, 1, 0]
    rng = random.Random(0x51075)
    slots = []
    for inp in inputs:
        own = [c for c in pool if c.inp == inp]
        pick = []
        for cls, n in (("valid", 2), ("order", 4), ("dup", 2), ("defect", 4), ("graft", 2), ("flip", 2)):
            of = [c for c in own if c.cls == cls]
            pick += rng.sample(of, min(n, len(of)))
        pick += rng.sample([c for c in pool if c not in pick], ms - len(pick))
        rng.shuffle(pick)
        slots.append(pick)
    want = [[O.expected_code(O.rules_of(inputs[i], c.indices)) if k < min(counts[i], ms) else O.CODE_EMPTY
             for k, c in enumerate(slots[i])] for i in range(4)]
    assert {w for row in want for w in row} == {0, 1, 2, 3, 4, O.CODE_EMPTY}
    return inputs, counts, slots, want


def test_eq_verify_slots_codes_and_count_clamp(gpu, by_length):
    """The solver's buffer layout [inst][1 + EQ_MAX_SOL * 512] with counts 0, 1, EQ_MAX_SOL and 40
    (clamped) and another input per instance: the oracle's code below the count, EQ_V_EMPTY from it
    on, although well-formed (stale) solutions lie there."""
    import numpy as np
    import torch

    from nodexa_chain_core_amd.ops import runtime
    from nodexa_chain_core_amd.ops.equihash import blake2b_h0

    h = runtime.hip()
    ms = h.EQ_MAX_SOL
    assert h.EQ_V_EMPTY == O.CODE_EMPTY and ms == 16
    inputs, counts, slots, want = slot_instances(by_length[112], ms)
    buf = np.zeros((4, 1 + ms * 512), dtype=np.uint32)
    msgs = bytearray(4 * 128)
    for i in range(4):
        msgs[i * 128:i * 128 + 112] = inputs[i]
        buf[i, 0] = counts[i]
        for k, c in enumerate(slots[i]):
            buf[i, 1 + k * 512:1 + (k + 1) * 512] = c.indices
    dev = torch.device("cuda", 0)
    with torch.cuda.device(dev):
        kern = runtime.static_kernel("equihash", "eq_verify_slots")
        dm = torch.frombuffer(msgs, dtype=torch.int64).to(dev)
        ds = torch.from_numpy(buf.view(np.int32)).to(dev)
        res = torch.full((4 * ms,), -1, dtype=torch.int32, device=dev)
        h.launch_equihash_verify_slots(kern, blake2b_h0(), dm.data_ptr(), 112, 4, ds.data_ptr(), res.data_ptr(),
                                       runtime.current_stream_handle())
        got = res.cpu().view(4, ms).tolist()
    assert got == want, [[c.name for c in row] for row in slots]


def test_verify_solutions_booleans(gpu, by_length):
    """ops.equihash.verify_solutions: True exactly where the oracle finds nothing wrong; a solution
    of the wrong byte length is False and leaves its neighbours' verdicts alone."""
    from nodexa_chain_core_amd.ops.equihash import verify_solutions

    for input_len in O.VALID_LENGTHS:
        batch = list(by_length[input_len])
        random.Random(1000 + input_len).shuffle(batch)
        inputs = [c.inp for c in batch]
        sols = [c.packed for c in batch]
        want = [not c.rules for c in batch]
        assert any(want) and not all(want)
        assert verify_solutions(inputs, sols, device=0) == want
        if input_len != 112:
            continue
        first_ok = want.index(True)
        for at, wrong in ((0, sols[first_ok][:-1]), (first_ok + 1, sols[first_ok] + b"\0"), (len(batch) // 2, b""),
                          (len(batch) + 3, sols[first_ok][:1340])):
            inputs.insert(at, batch[first_ok].inp)
            sols.insert(at, wrong)
            want.insert(at, False)
        assert verify_solutions(inputs, sols, device=0) == want
