"""clore-tx against the reference's own util test vectors (its test/util/data: every clore-tx case of
clore-util-test.json with its arguments, stdin, expected hex / JSON output and exit code, packed into
tests/golden/clore_tx_vectors.json, one case per line). The vectors carry Bitcoin-style addresses and
keys, so they run with the 0 / 5 / 128 version bytes they were generated with."""
import io
import json
import os

import pytest

from nodexa_chain_core_amd.cli import clore_tx

VECTORS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clore_tx_vectors.json")
PREFIXES = ["-pubkeyprefix=0", "-scriptprefix=5", "-secretprefix=128"]


def _cases():
    with open(VECTORS) as f:
        return json.load(f)


@pytest.mark.parametrize("case", _cases(), ids=lambda c: " ".join(c["args"])[:60])
def test_util_vector(case, capsys):
    args = list(case["args"])
    flags = [a for a in args if a.startswith("-") and a != "-"]
    rest = [a for a in args if not (a.startswith("-") and a != "-")]
    stdin = io.StringIO(case["input_text"]) if "input" in case else None
    out = io.StringIO()
    rc = clore_tx.main(PREFIXES + flags + rest, stdin=stdin, stdout=out)
    assert rc == case.get("return_code", 0), capsys.readouterr().err
    if "output_cmp" in case:
        if case["output_cmp"].endswith(".json"):
            assert json.loads(out.getvalue()) == case["output"]
        else:
            assert out.getvalue().strip() == case["output"]
