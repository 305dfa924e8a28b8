"""Output bits of gdml_sym_eig, gdml_sym_eig_dev, gdml_sym_eig_absv, gdml_perm_match (its own eigenvectors), vibrations() and
stationary_point() against the digests recorded from the commit before the two eigen-kernels became one template with one
launcher and one plan (csrc/sym_eig.hip, csrc/sym_eig_plan.h) and csrc/vib.hip was split by subject
(tests/golden/eig_parent_digests.json, written by tools/eig_digests.py, which also lists the cases).  Every sum of these paths
runs in a fixed order, so the outputs are reproducible bit for bit; a change that is meant to alter them regenerates the file and
says so."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import eig_digests  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, 'tests', 'golden', 'eig_parent_digests.json')) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope='module')
def ctx():
    from sgdml_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def test_golden_lists_the_tools_cases():
    assert sorted(GOLDEN) == sorted(eig_digests.case_ids())


@pytest.mark.parametrize('case_id', eig_digests.case_ids())
def test_output_bits_are_the_parents(ctx, case_id):
    got = eig_digests.digests(case_id, ctx)
    want = GOLDEN[case_id]
    print(case_id, {k: (got.get(k), want.get(k)) for k in sorted(set(got) | set(want)) if got.get(k) != want.get(k)})
    assert got == want
