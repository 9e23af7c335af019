"""The block plan of the item-parallel values kernel (k_mf_values; mfplan.hip, sparse.hpp MfValBlock) without a GPU,
through sqphip_mf_values_blocks: every item in exactly one block, whole destinations in order, at most 256 items per
block, the fallback for a destination of 257 items, and the host replay that sums block by block through a staging array
-- from the kernel's own item copy, every operand fetched whatever the type -- against the list-order replay, bit for bit."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
import mf_values_cases as VC

STRUCTURES = {S.name: S for S in VC.structures()}


def _blocks(S, cond, kind, seed):
    Jv, Hv, Dd, sigp, hd, rt, hsc = VC.values(S, kind, seed)
    return pkg.mf_values_blocks(S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, cond,
                                values=(Jv, Hv, Dd, sigp, hd, rt, hsc, 1e-3 * seed))


@pytest.mark.parametrize("name", list(STRUCTURES))
def test_blocks_partition_the_items_and_the_block_replay_gives_the_list_order_bits(name):
    S = STRUCTURES[name]
    for cond in (1, 0):
        out = _blocks(S, cond, "ipm", 3)
        ptr, blk = out["item_ptr"], out["blocks"]
        per_dest = np.diff(ptr)
        assert ptr[0] == 0 and ptr[-1] == out["n_items"] and per_dest.min() >= 1
        if cond == 1 and "max_items" in S.target:
            assert per_dest.max() == S.target["max_items"] and per_dest.min() == 1
        if per_dest.max() > 256:
            # a destination no block can hold: no blocks, the one-thread-per-destination kernel runs
            assert name == "items257" and cond == 1 and len(blk) == 0 and out["vals_block"] is None
            continue
        assert len(blk) > 0
        d0, i0, nd, ni = blk.T.astype(np.int64)
        # whole destinations in order, nothing left out, nothing twice
        assert d0[0] == 0 and np.array_equal(d0[1:], (d0 + nd)[:-1]) and d0[-1] + nd[-1] == len(per_dest)
        assert np.array_equal(i0, ptr[d0]) and np.array_equal(ni, ptr[d0 + nd] - ptr[d0])
        assert nd.min() >= 1 and ni.max() <= 256 and ni.sum() == out["n_items"]
        # greedy: the next destination would not have fitted
        assert np.all(ni[:-1] + per_dest[d0[1:]] > 256)
        for kind, seed in (("ipm", 3), ("well", 4), ("indef", 5)):
            o = out if (kind, seed) == ("ipm", 3) else _blocks(S, cond, kind, seed)
            assert np.isfinite(o["vals_list"]).all()
            assert np.array_equal(o["vals_block"], o["vals_list"]), (name, cond, kind)


def test_the_case118_structure_has_the_long_destinations_the_kernel_is_built_for():
    """condensed IEEE-118 (the bench's structure): 7 876 destinations, 10 770 items, most destinations of one item, the longest
    of 16 (duplicate COO entries are summed into one slot before the plan sees them) -- dozens of blocks, none over 256"""
    out = _blocks(STRUCTURES["case118"], 1, "well", 1)
    per_dest = np.diff(out["item_ptr"])
    assert len(per_dest) > 5000 and np.median(per_dest) == 1 and 10 <= per_dest.max() <= 256
    assert len(out["blocks"]) >= out["n_items"] // 256
