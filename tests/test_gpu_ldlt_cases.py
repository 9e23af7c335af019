"""Dense LDL^T (csrc/ldlt.hip) at every tile count, schedule switch and tile mask, through the kernel-level hook
sqphip_ldlt_case_test.  Every case: batch >= 2, distinct matrices per instance, the strict upper triangle of the device
buffers filled with quiet NaNs (the product never initialises it).

What is asserted (u = 2^-53, constants derived in tests/ldlt_cases.py):
  * componentwise backward error of the factor |L D L' - A| <= gamma_{N+4} |L||D||L'| in long double -- the whole lower
    triangle up to N = 257, above that a stratified sample (the whole diagonal and 64 seeded entries of every tile) plus
    the full product in fp64 with the bound doubled;
  * entry-wise agreement of L, dinv, y, v with the reference for well_scaled / flipped values (1e-12; long double up to
    N = 257, the oracle's C factorisation above), and for ipm_end up to N = 257 the device's error <= 8 e_ref + 1e-12, e_ref
    = error of the fp64 textbook factorisation against long double on the same matrix (printed per case);
  * pivot signs and the number of positive pivots, exact (construction, long-double pivots, eigvalsh where trustworthy);
  * both solutions (right-hand side fused into the factorisation; stand-alone forward / backward steps):
    |b - A x| <= gamma_{3N+4} |L||D||L'||x| in long double, and 1e-11 against the reference for well_scaled / flipped;
  * the identity padding, exact; the launch census of the case (diagonal tiles = T; on the auxiliary stream the whole panel
    chain of the dense part when T - Ts >= 24, else nothing -- counted where the launches are enqueued).
Which rule applies is fixed by family and size, never by outcome.

Measured on an MI355X when the file was written (720 instance checks): backward error at most 68 u (well_scaled), 53 u
(ipm_end), 65 u (flipped), 78 u (tiled) -- at most 0.27 of the bound; e_ref of ipm_end up to N = 257: L 1e-17 .. 1.7e-10,
dinv 3e-18 .. 5.1e-10, y 8e-14 .. 1.4e-10, v 1e-16 .. 6.3e-10 (tiled with ipm_end values: 6e-17 .. 3.8e-11), the device closest
to its allowance at ipm_end N = 191, v: 7e-11 against e_ref 1e-11 (0.86 of 8 e_ref + 1e-12).  Every instantiation with a
launch site was launched; no assertion failed under any switch.  SQPHIP_TPB=8 ran two tiles per workgroup in k_trailing
(N = 1600, 32 instances) and in k_colupdate (N = 320, 1024 instances) and SQPHIP_NO_LOOKAHEAD=1 one stream at 24 tile columns:
both bit-identical to the default schedule."""
import ctypes as C
import functools

import numpy as np
import pytest

import ldlt_cases as LC
from oracle import oracle as O
from sqpsolver_jl_amd import _lib

pytestmark = pytest.mark.gpu
dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
SENTINEL = -7.25e33
LOOKAHEAD_MIN = 24                 # LdltPlan::lookahead_min
N_KERNELS = 11
SWITCH_VARS = ("SQPHIP_KC", "SQPHIP_TRSM_MFMA", "SQPHIP_OUTER", "SQPHIP_SUPERTILE", "SQPHIP_TPB", "SQPHIP_TRAIL_PAD",
               "SQPHIP_NO_LOOKAHEAD", "SQPHIP_LOOKAHEAD_MIN", "SQPHIP_NO_PRIORITY")
CENSUS = {}                        # launches per kernel instantiation over every hook call of this module


@pytest.fixture(autouse=True)
def _no_inherited_switches(monkeypatch):
    for k in SWITCH_VARS:
        monkeypatch.delenv(k, raising=False)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(As, rhs=None, Ts=0, phase=None, want=1, nan_upper=True, no_tile_mask=False, expect_rc=0):
    """One call of the hook: returns the outputs at padded size plus the census of the call."""
    L = _lib.lib()
    B, N = len(As), As[0].shape[0]
    Npad = (N + 63) // 64 * 64
    if isinstance(As, np.ndarray):            # [B][N][N], symmetric: row-major storage of A is column-major storage of A'
        Af = np.ascontiguousarray(As, dtype=np.float64).reshape(B, N * N)
    else:
        Af = np.ascontiguousarray(np.stack([np.tril(a).ravel(order="F") for a in As]), dtype=np.float64)
    out = {k: np.full((B, Npad), np.nan) for k in ("dinv", "b", "v", "x_fused", "x_standalone")}
    fac = np.full((B, Npad * Npad), np.nan)
    npos = np.full(B, -1, dtype=np.int32)
    counts = np.zeros(32, dtype=np.int64)
    names = C.create_string_buffer(32 * 64)
    info = np.zeros(8, dtype=np.int64)
    r = None if rhs is None else np.ascontiguousarray(rhs, dtype=np.float64)
    ph = None if phase is None else np.ascontiguousarray(phase, dtype=np.int32)
    rc = L.sqphip_ldlt_case_test(0, B, N, Af.ctypes.data_as(dp), int(nan_upper), None if r is None else r.ctypes.data_as(dp),
                                 None if ph is None else ph.ctypes.data_as(ip), want, Ts, int(no_tile_mask), SENTINEL,
                                 fac.ctypes.data_as(dp), out["dinv"].ctypes.data_as(dp), npos.ctypes.data_as(ip),
                                 out["b"].ctypes.data_as(dp), out["v"].ctypes.data_as(dp), out["x_fused"].ctypes.data_as(dp),
                                 out["x_standalone"].ctypes.data_as(dp), counts.ctypes.data_as(lp), names, 32,
                                 info.ctypes.data_as(lp))
    assert rc == expect_rc, rc
    if rc:
        return None
    nk = int(info[0])
    assert nk == N_KERNELS and info[1] == Npad and info[2] == Npad // 64
    census = {names.raw[64 * k:64 * k + 64].split(b"\0")[0].decode(): int(counts[k]) for k in range(nk)}
    for k, c in census.items():
        CENSUS[k] = CENSUS.get(k, 0) + c
    out.update(F=[fac[b].reshape(Npad, Npad, order="F") for b in range(B)], npos=npos, census=census,
               diag_tiles=int(info[3]), aux=int(info[4]), masks=int(info[5]), tpb_trailing=int(info[6]),
               tpb_colupdate=int(info[7]), Npad=Npad, T=Npad // 64)
    return out


# ---------------------------------------------------------------------------------------------------- references
def reference(family, N, seed, tiled_case=None):
    """Everything about one matrix that does not depend on the device: A, right-hand side, the oracle's fp64 factors, and up
    to N = 257 the long-double factors, forward elimination and solution with the oracle's error against them (e_ref).
    Kept for re-use (switch matrix, triangle contract) up to 13 tiles only: the larger ones are used once."""
    tiles = sum(tiled_case[:2]) if tiled_case else (N + 63) // 64
    return (_reference_cached if tiles <= 13 else _reference)(family, N, seed, tiled_case)


def _reference(family, N, seed, tiled_case):
    if tiled_case is not None:
        Ts, Tr, pattern, values = tiled_case
        A, inf = LC.tiled(Ts, Tr, pattern, seed, values)
        npos = inf["npos"]
        family = values
    else:
        n1 = LC.default_n1(N)
        A = LC.FAMILIES[family](N, n1, seed)
        npos = LC.expected_npos(family, N, n1)
    N = A.shape[0]
    rhs = np.random.default_rng(900 + seed).standard_normal(N)
    a_o, dinv_o, npos_o, _ = O.ldlt_factor(A, N)
    Lo = np.tril(a_o, -1) + np.eye(N)
    yo, vo, xo = LC.solve_reference(Lo, 1.0 / dinv_o, rhs)             # fp64 textbook on the oracle's factors
    ref = dict(A=A, rhs=rhs, npos=npos, family=family, Lo=Lo, dinv_o=dinv_o, yo=yo, vo=vo, xo=xo)
    assert npos_o == npos
    if family != "ipm_end":
        assert int((np.linalg.eigvalsh(A) > 0).sum()) == npos           # Sylvester (well conditioned families only)
    if N <= LC.FULL_LD_MAX:
        Lr, dr = LC.ldl_reference(A)
        yr, vr, xr = LC.solve_reference(Lr, dr, rhs)
        f = lambda z: np.asarray(z, dtype=np.float64)
        ref.update(Lr=f(Lr), dinv_r=f(1 / dr), yr=f(yr), vr=f(vr), xr=f(xr), sign=np.sign(f(dr)),
                   e_ref=dict(L=LC.rel(Lo, f(Lr)), dinv=LC.rel(dinv_o, f(1 / dr)), y=LC.rel(yo, f(yr)), v=LC.rel(vo, f(vr))))
        assert int((dr > 0).sum()) == npos
    else:
        ref.update(sign=np.sign(dinv_o), x_np=np.linalg.solve(A, rhs))
    return ref


_reference_cached = functools.lru_cache(maxsize=40)(_reference)


def check_instance(tag, ref, out, b):
    """Every applicable assertion on instance b of a hook call (rules by family and size, see the module docstring)."""
    A, rhs, fam = ref["A"], ref["rhs"], ref["family"]
    N, Npad = A.shape[0], out["Npad"]
    F = out["F"][b]
    dinv, y, v = out["dinv"][b], out["b"][b], out["v"][b]
    for name in ("dinv", "b", "v", "x_fused", "x_standalone"):
        assert np.all(np.isfinite(out[name][b])), f"{tag}: non-finite {name}"
    low = np.tril(F, -1)
    assert np.all(np.isfinite(low)) and np.all(np.isfinite(np.diag(F))), f"{tag}: non-finite factor"
    # ---- padding, exact
    assert np.all(dinv[N:] == 1.0) and np.all(y[N:] == 0.0) and np.all(v[N:] == 0.0), f"{tag}: padding of dinv / b / v"
    assert np.all(out["x_fused"][b][N:] == 0.0) and np.all(out["x_standalone"][b][N:] == 0.0), f"{tag}: padding of x"
    assert not np.any(low[N:, :]) and np.all(np.diag(F)[N:] == 1.0), f"{tag}: padded part of the factor is not the identity"
    Ld = low[:N, :N] + np.eye(N)
    d = 1.0 / dinv[:N]
    # ---- pivot signs and inertia, exact
    assert np.array_equal(np.sign(dinv[:N]), ref["sign"]), f"{tag}: pivot signs"
    assert out["npos"][b] == ref["npos"], f"{tag}: npos {out['npos'][b]} != {ref['npos']}"
    # ---- backward error of the factor, componentwise
    g = LC.gamma_factor(N)
    if N <= LC.FULL_LD_MAX:
        be, at = LC.backward_error_full(A, Ld, d)
        how = "full"
    else:
        be, at, cnt = LC.backward_error_sampled(A, Ld, d, seed=N + b)
        how = f"{cnt} sampled"
        be64, at64 = LC.backward_error_full(A, Ld, d, dtype=np.float64)     # coarse net over every entry
        assert be64 <= 2 * g, f"{tag}: fp64 product: backward error {be64 / LC.U:.1f} u at {at64} (tile {at64[0] // 64, at64[1] // 64})"
    msg = f"{tag}: backward error {be / LC.U:.1f} u ({how}) at {at} (tile {at[0] // 64, at[1] // 64}), bound {g / LC.U:.0f} u"
    assert be <= g, msg
    # ---- entry-wise against the reference
    if N <= LC.FULL_LD_MAX:
        rL, rd, ry, rv = ref["Lr"], ref["dinv_r"], ref["yr"], ref["vr"]
    else:
        rL, rd, ry, rv = ref["Lo"], ref["dinv_o"], ref["yo"], ref["vo"]
    err = dict(L=LC.rel(Ld, rL), dinv=LC.rel(dinv[:N], rd), y=LC.rel(y[:N], ry), v=LC.rel(v[:N], rv))
    if fam != "ipm_end":
        assert all(e < 1e-12 for e in err.values()), f"{tag}: entry-wise {err}"
    elif N <= LC.FULL_LD_MAX:
        e_ref = ref["e_ref"]
        msg += " e_ref " + " ".join(f"{k} {e:.1e}" for k, e in e_ref.items()) + " device " + " ".join(f"{k} {e:.1e}" for k, e in err.items())
        for k in err:
            assert err[k] <= 8 * e_ref[k] + 1e-12, f"{tag}: {k}: device {err[k]:.2e} against e_ref {e_ref[k]:.2e}"
    # ---- both solutions
    gs = LC.gamma_solve(N)
    for name in ("x_fused", "x_standalone"):
        x = out[name][b][:N]
        rr = LC.residual_ratio(A, Ld, d, x, rhs)
        assert rr <= gs, f"{tag}: {name}: residual {rr / LC.U:.1f} u, bound {gs / LC.U:.0f} u"
        if fam != "ipm_end":
            xr = ref["xr"] if N <= LC.FULL_LD_MAX else ref["x_np"]
            assert LC.rel(x, xr) < 1e-11, f"{tag}: {name} against the reference: {LC.rel(x, xr):.2e}"
    # ---- census of the call
    T = out["T"]
    assert out["diag_tiles"] == T, f"{tag}: {out['diag_tiles']} diagonal tiles factorised, T = {T}"
    print(msg)


def check_census(tag, out, Ts, lookahead_min=LOOKAHEAD_MIN, no_lookahead=False, masks=False):
    c, T = out["census"], out["T"]
    # launches counted where they are enqueued on the auxiliary stream: with the look-ahead the whole panel chain of the dense
    # part (diagonal tiles, panel solves, left-looking column updates), without it nothing
    two_streams = T - Ts >= lookahead_min and not no_lookahead
    chain = (T - Ts) + max(T - Ts - 1, 0) + c["k_colupdate<16>"] + c["k_colupdate<32>"]
    assert out["aux"] == (chain if two_streams else 0), f"{tag}: {out['aux']} launches on the auxiliary stream, T - Ts = {T - Ts}"
    assert out["masks"] == int(masks)
    assert (c["k_trailing_list<16>"] > 0) == (masks and T > Ts), f"{tag}: k_trailing_list<16> launched {c['k_trailing_list<16>']} times"
    assert c["k_diag_factor"] == T - Ts + (1 if Ts else 0)


def plain_case(family, N, **kw):
    refs = [reference(family, N, 10 + b) for b in range(2)]
    out = run([r["A"] for r in refs], np.stack([r["rhs"] for r in refs]), **kw)
    for b, r in enumerate(refs):
        check_instance(f"{family} N={N} inst {b}", r, out, b)
    return out


def tiled_case(case, no_tile_mask=False):
    Ts, Tr, pattern, values = case
    refs = [reference("tiled", 0, 40 + b, case) for b in range(2)]
    out = run([r["A"] for r in refs], np.stack([r["rhs"] for r in refs]), Ts=Ts, no_tile_mask=no_tile_mask)
    for b, r in enumerate(refs):
        check_instance(f"tiled {case} inst {b}", r, out, b)
    return out


# ---------------------------------------------------------------------------------------------------- the matrix
@pytest.mark.parametrize("family", ["well_scaled", "ipm_end", "flipped"])
@pytest.mark.parametrize("N", LC.plain_sizes())
def test_plain_dense_at_every_tile_count(family, N):
    out = plain_case(family, N)
    check_census(f"{family} N={N}", out, 0)


@pytest.mark.parametrize("case", LC.TILED_CASES, ids=lambda c: "-".join(map(str, c)))
def test_independent_leading_tiles(case):
    out = tiled_case(case)
    check_census(f"tiled {case}", out, case[0], masks=case[1] > 0)


def test_leading_tiles_that_are_coupled_are_refused():
    A, _ = LC.tiled(2, 1, "all", 7)
    A[70, 3] = A[3, 70] = 0.5
    assert run([A, A], np.ones((2, A.shape[0])), Ts=2, expect_rc=-1) is None


SWITCHES = [{"SQPHIP_KC": "32"}, {"SQPHIP_TRSM_MFMA": "0"}, {"SQPHIP_OUTER": "1"}, {"SQPHIP_OUTER": "2"}, {"SQPHIP_OUTER": "3"},
            {"SQPHIP_SUPERTILE": "1"}, {"SQPHIP_SUPERTILE": "3"}, {"SQPHIP_TPB": "8"}, {"SQPHIP_TRAIL_PAD": "65536"},
            {"SQPHIP_NO_LOOKAHEAD": "1"}, {"SQPHIP_LOOKAHEAD_MIN": "0"}, {"SQPHIP_NO_TILE_MASK": "1"}]
SWITCH_T = (1, 2, 4, 5, 9, 13)
SWITCH_TILED = {5: (2, 3, "half", "well_scaled"), 9: (5, 4, "half", "ipm_end")}


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: "-".join(f"{k[7:]}={v}" for k, v in e.items()))
def test_switch_matrix(env, monkeypatch):
    """The full assertion set under every schedule switch of LdltPlan::init_lookahead (SQPHIP_FUSED_FWD of the older hook needs
    no run of its own: every case checks the fused and the stand-alone solve).  SQPHIP_NO_TILE_MASK is read by sqphip_create,
    not by the plan: the hook takes it as a flag, and it only changes the tiled cases.  Two switches select nothing at these
    sizes and batch 2 -- SQPHIP_TPB (runs of tiles need tiles x batch >= 4096 in a launch) and SQPHIP_NO_LOOKAHEAD (one stream
    below 24 tile columns anyway): here they only show that setting them is harmless; the code they select runs in
    test_tile_runs_per_workgroup and test_no_lookahead_gives_the_two_stream_bits."""
    no_mask = "SQPHIP_NO_TILE_MASK" in env
    for k, v in env.items():
        if not no_mask:
            monkeypatch.setenv(k, v)
    la_min = int(env.get("SQPHIP_LOOKAHEAD_MIN", LOOKAHEAD_MIN))
    no_la = "SQPHIP_NO_LOOKAHEAD" in env
    for T in SWITCH_T:
        if not no_mask:
            for N in (64 * T, 64 * T + 1):
                fams = ["well_scaled"] + (["ipm_end"] if T in (5, 9) else [])
                for fam in fams:
                    out = plain_case(fam, N)
                    check_census(f"{env} {fam} N={N}", out, 0, la_min, no_la)
                    c = out["census"]
                    if "SQPHIP_KC" in env:
                        assert c["k_trailing<16>"] == c["k_colupdate<16>"] == 0
                        assert (c["k_trailing<32>"] > 0) == (out["T"] > 4) and (c["k_colupdate<32>"] > 0) == (out["T"] > 1)
                    if "SQPHIP_TRSM_MFMA" in env:
                        assert c["k_panel_trsm_mfma"] == 0 and c["k_panel_trsm<1>"] == out["T"] - 1
        if T in SWITCH_TILED:
            case = SWITCH_TILED[T]
            out = tiled_case(case, no_tile_mask=no_mask)
            check_census(f"{env} tiled {case}", out, case[0], la_min, no_la, masks=not no_mask)
            if no_mask:
                assert out["census"]["k_trailing_list<16>"] == 0 and out["census"]["k_trailing<16>"] > 0


def random_batch(B, N, seed):
    """[B][N][N] distinct well_scaled-like matrices in one draw (the family's recipe, vectorised over the batch)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((B, N, N)) * 0.3
    A = (A + A.transpose(0, 2, 1)) / 2
    n1 = LC.default_n1(N)
    i = np.arange(N)
    A[:, i, i] = np.concatenate([np.ones(n1), -np.ones(N - n1)]) * (0.9 * np.sqrt(N) + rng.uniform(0.5, 1.5, (B, N)))
    return A


@pytest.mark.parametrize("N,B,kernel", [(64 * 25, 32, "trailing"), (64 * 5, 1024, "colupdate")], ids=["trailing", "colupdate"])
def test_tile_runs_per_workgroup(N, B, kernel, monkeypatch):
    """SQPHIP_TPB=8: a Schur-update workgroup takes a run of min(8, tiles x batch / 2048) tiles and hands the operand pipeline
    over from one tile to the next (schur_update_run: tile_decode of the next tile, the fetch across the tile boundary, the
    stage parity carried over).  Needs tiles x batch >= 4096 in a launch: 25 tile columns x 32 instances for k_trailing (153
    tiles in the first update behind the head), 5 x 1024 for k_colupdate (4 tiles in the second column of the panel).  The run
    length changes who computes a tile, not the arithmetic: every output bit equals the run with the switch unset, and the
    factor keeps the backward-error bound."""
    A = random_batch(B, N, 5)
    rhs = np.random.default_rng(6).standard_normal((B, N))
    o1 = run(A, rhs)
    monkeypatch.setenv("SQPHIP_TPB", "8")
    o8 = run(A, rhs)
    print(f"tiles per workgroup: k_trailing {o1['tpb_trailing']} -> {o8['tpb_trailing']}, k_colupdate {o1['tpb_colupdate']} -> {o8['tpb_colupdate']}")
    assert o1["tpb_trailing"] <= 1 and o1["tpb_colupdate"] <= 1
    assert o8["tpb_" + kernel] > 1
    assert o1["census"] == o8["census"]
    il = np.tril_indices(o1["Npad"])
    for b in range(B):
        assert np.array_equal(bits(o1["F"][b][il]), bits(o8["F"][b][il])), f"factor of instance {b} differs"
    for k in OUT_VECTORS:
        assert np.array_equal(bits(o1[k]), bits(o8[k])), k
    assert np.array_equal(o1["npos"], o8["npos"]) and np.all(o8["npos"] == LC.default_n1(N))
    for b in (0, B - 1):
        Ld = np.tril(o8["F"][b], -1)[:N, :N] + np.eye(N)
        d = 1.0 / o8["dinv"][b][:N]
        be, at, _ = LC.backward_error_sampled(A[b], Ld, d, seed=b)
        assert be <= LC.gamma_factor(N), f"instance {b}: backward error {be / LC.U:.1f} u at {at}"
        assert LC.residual_ratio(A[b], Ld, d, o8["x_fused"][b][:N], rhs[b]) <= LC.gamma_solve(N)


@pytest.mark.parametrize("N,la_min", [(64 * 24, None), (64 * 9 + 1, "0")], ids=["T=24", "T=10-LOOKAHEAD_MIN=0"])
def test_no_lookahead_gives_the_two_stream_bits(N, la_min, monkeypatch):
    """SQPHIP_NO_LOOKAHEAD=1 where it changes the schedule (24 tile columns, or fewer with SQPHIP_LOOKAHEAD_MIN=0): nothing is
    enqueued on the auxiliary stream, and every output bit equals the two-stream run."""
    if la_min is not None:
        monkeypatch.setenv("SQPHIP_LOOKAHEAD_MIN", la_min)
    refs = [reference("well_scaled", N, 10 + b) for b in range(2)]
    As, rhs = [r["A"] for r in refs], np.stack([r["rhs"] for r in refs])
    o2 = run(As, rhs)
    monkeypatch.setenv("SQPHIP_NO_LOOKAHEAD", "1")
    o1 = run(As, rhs)
    la = LOOKAHEAD_MIN if la_min is None else int(la_min)
    check_census("two streams", o2, 0, la)
    check_census("one stream", o1, 0, la, no_lookahead=True)
    assert o2["aux"] > 0 and o1["aux"] == 0 and o1["census"] == o2["census"]
    for b, r in enumerate(refs):
        assert_same_bits("NO_LOOKAHEAD", o1, o2, b)
        check_instance(f"NO_LOOKAHEAD=1 N={N} inst {b}", r, o1, b)


# ---------------------------------------------------------------------------------------------------- contracts
OUT_VECTORS = ("dinv", "b", "v", "x_fused", "x_standalone")


def assert_same_bits(tag, o1, o2, b):
    il = np.tril_indices(o1["Npad"])
    assert np.array_equal(bits(o1["F"][b][il]), bits(o2["F"][b][il])), f"{tag}: factor of instance {b} differs"
    for k in OUT_VECTORS:
        assert np.array_equal(bits(o1[k][b]), bits(o2[k][b])), f"{tag}: {k} of instance {b} differs"
    assert o1["npos"][b] == o2["npos"][b]


@pytest.mark.parametrize("env", [{}, {"SQPHIP_KC": "32"}, {"SQPHIP_TRSM_MFMA": "0"}], ids=["default", "KC=32", "TRSM_MFMA=0"])
def test_upper_triangle_is_never_read(env, monkeypatch):
    """ldlt.hip: only the lower triangle is meaningful; the product never initialises the strict upper one.  NaNs there
    must not change a bit of any output."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cases = [("well_scaled", N, None, 0) for N in (65, 257, 600)] + [("tiled", 0, (5, 4, "half", "well_scaled"), 5)]
    for fam, N, tc, Ts in cases:
        refs = [reference(fam, N, 40 + b if tc else 10 + b, tc) for b in range(2)]
        As, rhs = [r["A"] for r in refs], np.stack([r["rhs"] for r in refs])
        o_nan = run(As, rhs, Ts=Ts, nan_upper=True)
        o_zero = run(As, rhs, Ts=Ts, nan_upper=False)
        for b in range(2):
            il = np.tril_indices(o_nan["Npad"])
            assert np.all(np.isfinite(o_nan["F"][b][il])) and all(np.all(np.isfinite(o_nan[k][b])) for k in OUT_VECTORS)
            assert_same_bits(f"{env} {fam} N={As[0].shape[0]}", o_nan, o_zero, b)


@pytest.mark.parametrize("lookahead_min0", [False, True], ids=["default", "LOOKAHEAD_MIN=0"])
@pytest.mark.parametrize("shape", ["plain", "tiled"])
def test_phase_mask(shape, lookahead_min0, monkeypatch):
    """Instances outside the mask come back bit-unchanged (matrix, dinv, b, v, x); the ones inside are bit-identical to a run
    of the same eight matrices without a mask: per-instance arithmetic does not depend on the neighbours."""
    if lookahead_min0:
        monkeypatch.setenv("SQPHIP_LOOKAHEAD_MIN", "0")
    B = 8
    if shape == "plain":
        N, Ts = 64 * 6 + 1, 0
        As = [LC.well_scaled(N, LC.default_n1(N), 60 + b) for b in range(B)]
    else:
        Ts = 2
        As = [LC.tiled(2, 5, "half", 60 + b, "well_scaled")[0] for b in range(B)]
        N = As[0].shape[0]
    rng = np.random.default_rng(77)
    rhs = rng.standard_normal((B, N))
    phase = np.array([3, 1, 3, 3, 1, 0, 3, 1], dtype=np.int32)[rng.permutation(B)]      # want = 3: five in, three out
    want = 3
    assert 2 <= int((phase == want).sum()) <= B - 2
    rhs_mask = rhs.copy()
    rhs_mask[phase != want] = SENTINEL            # b of an instance outside the mask: a sentinel too
    o_mask = run(As, rhs_mask, Ts=Ts, phase=phase, want=want, nan_upper=False)
    o_all = run(As, rhs, Ts=Ts, nan_upper=False)
    Npad = o_mask["Npad"]
    il = np.tril_indices(Npad)
    for b in range(B):
        if phase[b] == want:
            assert_same_bits(f"{shape} active", o_mask, o_all, b)
            continue
        K0 = LC.pad_to_tiles(As[b])
        assert np.array_equal(bits(o_mask["F"][b][il]), bits(K0[il])), f"matrix of masked-out instance {b} changed"
        rp = np.zeros(Npad)
        rp[:N] = SENTINEL
        assert np.all(o_mask["dinv"][b] == SENTINEL) and np.all(o_mask["v"][b] == SENTINEL), f"dinv / v of masked-out instance {b}"
        for k in ("b", "x_fused", "x_standalone"):
            assert np.array_equal(bits(o_mask[k][b]), bits(rp)), f"{k} of masked-out instance {b} changed"
    # the unmasked run is a correct factorisation of every instance (so "identical" above means "identical and right")
    for b in (0, B - 1):
        Ld = np.tril(o_all["F"][b], -1)[:N, :N] + np.eye(N)
        assert LC.backward_error_sampled(As[b], Ld, 1.0 / o_all["dinv"][b][:N], seed=b)[0] <= LC.gamma_factor(N)


# ---------------------------------------------------------------------------------------------------- census
CENSUS_NO_LAUNCH_SITE = ["k_panel_trsm<2>"]      # a template nobody instantiates: ldlt_factor launches <1> or the MFMA variant only


def test_census_reached_every_instantiation(monkeypatch):
    """Every kernel instantiation ldlt_factor / ldlt_solve can launch was launched.  A representative subset is run here
    (no references: the other tests judge the numbers) so that the test also stands alone; the counts are added to those of
    the tests that ran before it in this module."""
    def go(N, env=None, tiled=None, no_tile_mask=False):
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        if tiled:
            As = [LC.tiled(*tiled[:3], 40 + b, tiled[3])[0] for b in range(2)]
        else:
            As = [LC.well_scaled(N, LC.default_n1(N), 10 + b) for b in range(2)]
        out = run(As, np.ones((2, As[0].shape[0])), Ts=tiled[0] if tiled else 0, no_tile_mask=no_tile_mask)
        for k in (env or {}):
            monkeypatch.delenv(k)
        la = int((env or {}).get("SQPHIP_LOOKAHEAD_MIN", LOOKAHEAD_MIN))
        Ts = tiled[0] if tiled else 0
        check_census(f"census N={N} {env} {tiled}", out, Ts, la, masks=bool(tiled) and tiled[1] > 0 and not no_tile_mask)
        assert out["diag_tiles"] == out["T"]
        return out
    for N in (65, 64 * 9, 64 * 23, 64 * 24):              # T - Ts = 23: one stream; 24: the look-ahead
        go(N)
    go(64 * 9 + 1, {"SQPHIP_KC": "32"})
    go(64 * 5, {"SQPHIP_TRSM_MFMA": "0"})
    go(64 * 5, {"SQPHIP_LOOKAHEAD_MIN": "0"})
    go(0, tiled=(5, 4, "half", "well_scaled"))
    go(0, tiled=(5, 4, "half", "well_scaled"), no_tile_mask=True)
    go(0, tiled=(2, 24, "half", "well_scaled"))
    print("launch census:", ", ".join(f"{k}: {c}" for k, c in CENSUS.items()))
    print("without a launch site, never instantiated (no counter):", CENSUS_NO_LAUNCH_SITE)
    never = [k for k, c in CENSUS.items() if c == 0]
    print("never launched:", never or "none")
    assert len(CENSUS) == N_KERNELS and not never, never
