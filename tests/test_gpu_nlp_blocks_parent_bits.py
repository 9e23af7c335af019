"""The five families of dense data blocks (csrc/nlp_blocks_dev.hpp and the family headers) file the bits they filed before they
were put on shared building blocks: tests/golden/nlp_*_parent_bits.npz, recorded from that commit's parent on the GPU by
tests/golden/make_nlp_blocks_parent_bits.py, hold f, grad, g, jval, hval of every evaluation of
tests/nlp_blocks_parent_cases.py -- every entry of each family's EDGE_CASES, every instance, and the two-block companion
models.  Equality is the criterion: no tolerance.  The same call without the Hessian pointer (the gradient-only branches of the
evaluators, and with them what an Armijo probe reads) must file the same f, grad, g and jval."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sqpsolver_jl_amd as pkg                                        # noqa: E402
import nlp_blocks_parent_cases as PC                                  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(family, name, build) for family in PC.FAMILIES for name, build in PC.case_list(family)]
_GOLD = {}


def _gold(family):
    if family not in _GOLD:
        _GOLD[family] = np.load(PC.golden_path(HERE, family))
    return _GOLD[family]


def test_the_records_hold_every_evaluation_and_nothing_else():
    """(needs no GPU: runs with the CPU suite)"""
    for family in PC.FAMILIES:
        names = {k.rsplit("/", 2)[0] for k in _gold(family).files}
        assert names == {name for name, _ in PC.case_list(family)}, family


@pytest.mark.gpu
@pytest.mark.parametrize("family,name,build", CASES, ids=["%s-%s" % c[:2] for c in CASES])
def test_a_block_files_the_parents_bits(family, name, build):
    gold = _gold(family)
    done = 0
    for b, ev, no in PC.run_case(pkg, build):
        for k in PC.KEYS:
            want = gold["%s/%d/%s" % (name, b, k)]
            assert np.array_equal(np.asarray(ev[k]), want), (family, name, b, k)
            if k != "hval":
                assert np.array_equal(np.asarray(no[k]), want), (family, name, b, k, "without the Hessian")
            done += 1
    assert done == len(PC.KEYS) * len([k for k in gold.files if k.startswith(name + "/") and k.endswith("/f")])
