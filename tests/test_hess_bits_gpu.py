"""Output bits of predict_hessian, predict and predict_virial against the digests recorded before hess_device was rewritten
around csrc/hess_plan.h and the epilogue sums were folded into one helper (tests/golden/hess_parent_digests.json, written by
tools/hess_digests.py, which also lists the cases).  Every sum of these paths runs in a fixed order, so the outputs are
reproducible bit for bit; a change that is meant to alter them regenerates the file and says so."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import hess_digests  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, 'tests', 'golden', 'hess_parent_digests.json')) as _f:
    GOLDEN = json.load(_f)


def test_golden_lists_the_tools_cases():
    assert sorted(GOLDEN) == sorted(hess_digests.case_ids())


@pytest.mark.parametrize('case_id', hess_digests.case_ids())
def test_output_bits_are_the_parents(case_id):
    got = hess_digests.digests(case_id)
    want = GOLDEN[case_id]
    print(case_id, {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)})
    assert got == want
