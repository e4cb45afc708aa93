"""Every fused optimizer step entry point, in every combination of its flags, gives the bits recorded in
tests/golden/optimizer_bits.json (tests/optimizer_bits.py has the cases, the inputs and the recording)."""
import json

import pytest

from . import optimizer_bits as ob

with open(ob.GOLDEN) as f:
    RECORD = json.load(f)


def test_the_record_covers_exactly_the_cases():
    assert sorted(RECORD) == sorted(c["name"] for c in ob.CASES)
    entries = {c["entry"] for c in ob.CASES}
    assert len(entries) == 14 and {c["n"] for c in ob.CASES} == set(ob.SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ob.CASES, ids=lambda c: c["name"])
def test_step_bits(case):
    assert ob.digest(case) == RECORD[case["name"]]
