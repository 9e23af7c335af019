"""The static front kernels with an LDS image (k_mf_front<T, NW, true>) with the image stored as packed lower-triangular
tiles (the default) against the square image (SQPHIP_MF_FRONT_PACKED=0), bit for bit, through one sweep of
sqphip_mf_batch_test on the families of tests/mf_structures.py that reach those kernels: single fronts on both sides of
every tile count from four to eight tile rows (and, under SQPHIP_MF_STATIC_MIN=1, of one to four), once more on half the
waves (SQPHIP_MF_NW4=0 SQPHIP_MF_NW8=0), a narrow level whose fronts are shorter than their launch's image (every tile of
the launch must be zeroed: the load reads them all), partial last four-column blocks, a root with children (extend-add)."""
import numpy as np
import pytest

import sqpsolver_jl_amd as pkg
import mf_structures as MS

pytestmark = pytest.mark.gpu

FAMILIES = {S.name: S for S in MS.families()}
B, IDLE = 5, 3
HALF_WAVES = {"SQPHIP_MF_NW4": "0", "SQPHIP_MF_NW8": "0"}
SINGLE_4_TO_8 = ("front62", "front63", "front64", "front78", "front79", "front80", "front94", "front95", "front96",
                 "front110", "front111", "front112", "front126", "front127")


def _img_kernels(T, half=False):
    """census names of the static LDS-image kernels of T tile rows that the switches of the case can reach"""
    if T <= 3:
        return (f"k_mf_front<{T}, 1, true>",)
    nw = (2 if half else 4) if T <= 5 else (4 if half else 8)
    return (f"k_mf_front<{T}, {nw}, true>",)


def _tiles(name):
    return FAMILIES[name].target["max_tiles"]


# (family, switches, tile rows of the static LDS-image kernel that must have been launched)
CASES = [(n, {}, _img_kernels(_tiles(n))) for n in SINGLE_4_TO_8]
# narrow_mixed_T: cliques of 10 .. 100 variables + 4 of the separator and the right-hand-side row -> the tallest has seven
# tile rows, and the whole level runs in its launch; nc_mod4_*: 52 + r + 4 rows + 1 -> four; top_84: the clique of 78 -> six
CASES += [("narrow_mixed_T", {}, _img_kernels(7)),
          ("nc_mod4_1_rows", {}, _img_kernels(4)), ("nc_mod4_2_rows", {}, _img_kernels(4)), ("nc_mod4_3_rows", {}, _img_kernels(4)),
          ("top_84", {}, _img_kernels(6))]
CASES += [(n, {"SQPHIP_MF_STATIC_MIN": "1"}, _img_kernels(_tiles(n)))
          for n in ("front15", "front16", "front31", "front32", "front47", "front48")]
CASES += [(n, HALF_WAVES, _img_kernels(_tiles(n), half=True)) for n in SINGLE_4_TO_8]


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


@pytest.mark.parametrize("name,env,kernels", CASES,
                         ids=["-".join([n] + [f"{k[len('SQPHIP_MF_'):]}={x}" for k, x in e.items()]) for n, e, _ in CASES])
def test_packed_image_gives_the_bits_of_the_square_image(name, env, kernels, monkeypatch):
    S = FAMILIES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for kind in ("well", "indef"):
        monkeypatch.delenv("SQPHIP_MF_FRONT_PACKED", raising=False)
        new, census = _sweep(S, kind)
        assert sum(census[k] for k in kernels) > 0, (name, kernels, {k: c for k, c in census.items() if c})
        monkeypatch.setenv("SQPHIP_MF_FRONT_PACKED", "0")
        old, census0 = _sweep(S, kind)
        assert census0 == census
        for key in ("dinv0", "dinv1", "fused", "standalone", "decision", "dw"):
            assert np.array_equal(new[key], old[key]), (name, kind, key)
        assert np.isfinite(new["dinv0"][[b for b in range(B) if b != IDLE]]).all()
