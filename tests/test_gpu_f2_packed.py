"""The generic front kernels with an LDS image (k_mf_factor2<NW, MAXT, true>) with the image stored as packed lower-
triangular tiles (the default) against the square image (SQPHIP_MF_F2_PACKED=0), bit for bit, through one sweep of
sqphip_mf_batch_test on the families of tests/mf_structures.py that reach those kernels under SQPHIP_MF_STATIC=0: single
fronts of one to four tile rows, merged and per-class wide levels (fronts shorter than their launch's image), partial
four-column blocks."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
import mf_structures as MS

pytestmark = pytest.mark.gpu

NAMES = ("front15", "front31", "front47", "front63", "wide_small_T", "wide_classes", "nc_mod4_1_rows")
FAMILIES = {S.name: S for S in MS.families() if S.name in NAMES}
B, IDLE = 5, 3
IMG_KERNELS = ("k_mf_factor2<1, 3, true>", "k_mf_factor2<2, 5, true>", "k_mf_factor2<4, 4, true>")


def _sweep(S, kind):
    ctx = pkg.Context(S.n, S.m, 0, S.jrow, S.jcol, S.hrow, S.hcol, -np.ones(S.n), np.ones(S.n), S.gL, S.gU,
                      pkg.default_options(kkt_mode=S.kkt_mode, kkt_condense=1), batch=B)
    vals = [MS.values(S, kind, 17 * b + 1) for b in range(B)]
    st = lambda k: np.stack([v[k] for v in vals])
    rhs = np.random.default_rng(5).normal(size=(B, S.nu(1)))
    active = np.array([b != IDLE for b in range(B)], dtype=np.int32)
    dw = np.array([1e-3 * (b + 1) for b in range(B)]) if kind != "indef" else np.zeros(B)
    fa = np.array([0, 0, 1, 0, 2]) if kind == "indef" else np.zeros(B, dtype=int)
    out = ctx.mf_batch_test(active, st(0), st(1), st(2), st(3), st(4), st(5), np.array([v[6] for v in vals]), dw,
                            np.array([0.0, 1e-4, 0.0, 0.0, 5e-3]), fa, rhs)
    census = ctx.mf_census()
    ctx.close()
    return out, census


@pytest.mark.parametrize("name", NAMES)
def test_packed_image_gives_the_bits_of_the_square_image(name, monkeypatch):
    S = FAMILIES[name]
    monkeypatch.setenv("SQPHIP_MF_STATIC", "0")
    for kind in ("well", "indef"):
        monkeypatch.delenv("SQPHIP_MF_F2_PACKED", raising=False)
        new, census = _sweep(S, kind)
        assert sum(census[k] for k in IMG_KERNELS) > 0, (name, census)
        monkeypatch.setenv("SQPHIP_MF_F2_PACKED", "0")
        old, census0 = _sweep(S, kind)
        assert census0 == census
        for key in ("dinv0", "dinv1", "fused", "standalone", "decision", "dw"):
            assert np.array_equal(new[key], old[key]), (name, kind, key)
        assert np.isfinite(new["dinv0"][[b for b in range(B) if b != IDLE]]).all()
