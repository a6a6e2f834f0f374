"""What the eight plan-creating entry points refuse, without a GPU: every
entry x base (element types, order) x bad argument set of
tests/golden/make_plan_abi_golden.py returns the code, leaves *out as, and
sets the fa_last_error() text that the library did before the entries were
rebuilt over one constructor (tests/golden/plan_refusals.json, recorded from
that commit).  Pairs of bad arguments pin which one wins: per arm of the
torch-GPU-order body, flag bits, NULL out, order, n, elem / tile, segments."""
import ctypes
import json
import os
import sys

import pytest

from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_plan_abi_golden as gold  # noqa: E402

from feddct_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    with open(gold.REFUSALS) as f:
        return json.load(f)


def test_case_list_is_the_generators(recorded):
    """Every case the generator enumerates is recorded, as a refusal or as one
    the recording library let through to its first device call."""
    rows = [tuple(r[:3]) for r in recorded["rows"]]
    dropped = [tuple(r) for r in recorded["dropped"]]
    assert len(set(rows)) == len(rows) and not set(rows) & set(dropped)
    assert sorted(rows + dropped) == sorted(gold.enumerate_cases())
    assert {r[0] for r in rows} == set(gold.ENTRIES) and len(gold.ENTRIES) == 8
    singles = {c for _, _, c in rows if "+" not in c}
    assert singles == set(gold.SINGLES)


@pytest.mark.parametrize("entry", list(gold.ENTRIES))
def test_refusals_match_the_parent(recorded, entry):
    bad = []
    for e, base, case, rc, out, msg in recorded["rows"]:
        if e == entry:
            got = gold.run_case(e, base, case)
            if got != (rc, out, msg):
                bad.append((base, case, got, (rc, out, msg)))
    assert not bad, bad[:10]


def test_cases_the_parent_let_through_are_still_let_through(recorded):
    """No argument check was added: what reached the device still does (a
    plan, or without a GPU the device's own error)."""
    for e, base, case in recorded["dropped"]:
        rc, h, msg = gold.run_case(e, base, case)
        assert rc in (_lib.FA_OK, _lib.FA_E_HIP), (e, base, case, rc, msg)
        if rc == _lib.FA_OK:
            _lib.check(_lib.lib.fa_plan_destroy(ctypes.c_void_p(h)), "fa_plan_destroy")
