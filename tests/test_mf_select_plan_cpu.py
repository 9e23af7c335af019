"""CPU test (no GPU) of what a plan's factorisation will launch (sqphip_mf_factor_kernels): on every family of
tests/mf_structures.py and on the IEEE-14 / -118 / 1354-bus shapes, at a small batch (levels merged up to four tiles) and a
large one, under each switch set of tests/test_gpu_mf_structures.py -- the kernel, the image and the spine flag of every
factor launch are those the independent mirror tests/mf_select_ref.py gives for the launches of sqphip_mf_plan_info."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
import mf_select_ref as REF
from test_mf_defer_cpu import STRUCTURES, _narrow_level        # the families, the deferral example and the three bus shapes
from test_mf_select_cpu import ENV_VARIANTS, ids

BATCHES = (5, 128)


@pytest.mark.parametrize("env", ENV_VARIANTS, ids=ids)
@pytest.mark.parametrize("batch", BATCHES)
def test_the_hook_names_the_kernels_the_mirror_chooses(batch, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sw = REF.switches(env)
    seen = set()
    for S in STRUCTURES:
        args = (S.n, S.m, S.jrow, S.jcol, S.hrow, S.hcol, S.gL, S.gU, 1, batch)
        fr, la, _, spine_fronts = pkg.mf_plan_info(*args)
        narrow = _narrow_level(fr)
        for big_lds in (1, 0):
            ker = pkg.mf_factor_kernels(*args, big_lds)
            assert ker.shape == (len(la), 4), S.name
            # small: at most eight fronts when the schedule was built; the deferral pass only ever adds fronts to a launch that stays
            assert set(np.unique(ker[:, 1:]).tolist()) <= {0, 1} and np.all(ker[la[:, 2] <= 8, 3] == 1), S.name
            for k, (level, tiles, count, _tmin) in enumerate(la.tolist()):
                name, packed = REF.select_front(tiles, bool(ker[k, 3]), level >= narrow, bool(big_lds), sw)
                assert (REF.KERNEL_NAMES[ker[k, 0]], bool(ker[k, 1])) == (name, packed), (S.name, batch, env, big_lds, k, la[k])
                assert bool(ker[k, 2]) == (spine_fronts > 0 and bool(big_lds) and not sw.v1 and level >= narrow), (S.name, k)
                seen.add(name)
            if spine_fronts > 0 and big_lds:
                assert ker[:, 2].any(), S.name
                seen.add("k_mf_spine")
    assert len(seen) >= 5 and ("k_mf_spine" in seen) == (env.get("SQPHIP_MF_SPINE") == "1")
