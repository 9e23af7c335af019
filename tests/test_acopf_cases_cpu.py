"""The cases of tests/acopf_cases.py, the 50-digit reference of tests/acopf_ref.py and the CPU oracle, validated against
each other without a GPU: tests/test_gpu_acopf_cases.py then holds the device evaluators to the same reference, the same
scaled bound and the same constants.

    oracle against reference    every small case, form and point, entry by entry: |got - ref| <= K 2^-52 scale, exact zeros
    the constants               K = 4 x the oracle's measured error, rounded up to a power of two -- measured here
    structure                   d g_i / d x_j along EVERY variable: nothing outside a row's declared variables
    stride cases                oracle f and g against the reference; J v against a 50-digit directional difference of g
    layout identities           lower triangle, bus pairs, orientations, folded angle limits, balance incidence counts
    a wrong sign                one Bs coefficient flipped: the comparison fails, at that row and nowhere else"""
import dataclasses

import numpy as np
import pytest

import acopf_cases as AC
import acopf_ref as AR
from oracle import oracle as O

SMALL = [(n, f) for n in AC.SMALL_NAMES for f in AC.FORMS]
STRIDE = [(n, f) for n in AC.STRIDE_NAMES for f in AC.FORMS]
ids = lambda cases: [f"{n}-{f}" for n, f in cases]


def _outputs(lay, ref, got):
    """(kind, got, ref, scale) of the five outputs, J and H placed densely"""
    return (("f", got["f"], ref.f, ref.fscale), ("grad", got["grad"], ref.grad, ref.gradscale), ("g", got["g"], ref.g, ref.gscale),
            ("J", AR.place_J(lay, got["jval"]), ref.J, np.broadcast_to(ref.jscale[:, None], ref.J.shape)),
            ("H", AR.place_H(lay, got["hval"]), ref.H, ref.hscale))


@pytest.mark.parametrize("name,form", SMALL, ids=ids(SMALL))
def test_oracle_matches_the_reference_entry_by_entry(name, form):
    M, lay = AC.model(name, form), AC.layout(name, form)
    assert (M.n, M.m) == (lay.n, lay.m)
    P = O.problem_acopf(AC.net_of(name), lay)
    for k in range(AC.NPOINTS):
        msgs = AC.check(M, lay, AC.reference(name, form, k), AC.oracle_eval(P, AC.points(name, form)[k]))
        assert not msgs, f"{name} point {k}: " + "; ".join(msgs[:8])


def test_the_constants_are_four_times_the_measured_ones():
    """K_oracle per output over every small case, form and point, measured here; the committed K must be 4 x the recorded
    measurement rounded up to a power of two, and the measurement of this machine must fit under K / 4 as well."""
    worst = {k: 0.0 for k in AC.K}
    for name, form in SMALL:
        lay = AC.layout(name, form)
        P = O.problem_acopf(AC.net_of(name), lay)
        for k in range(AC.NPOINTS):
            got = AC.oracle_eval(P, AC.points(name, form)[k])
            for what, g, r, s in _outputs(lay, AC.reference(name, form, k), got):
                kmax, _, bad = AR.entrywise(np.atleast_1d(g), np.atleast_1d(r), np.atleast_1d(s))
                assert not bad, (name, form, k, what, bad[:4])
                worst[what] = max(worst[what], kmax)
    print("K_oracle measured:", {k: round(v, 3) for k, v in worst.items()}, "recorded:", AC.K_ORACLE_MEASURED, "K:", AC.K)
    for what in AC.K:
        assert AC.K[what] == AC.k_from_measured(AC.K_ORACLE_MEASURED[what]), what
        assert 4.0 * worst[what] <= AC.K[what], (what, worst[what])


@pytest.mark.parametrize("name,form", SMALL, ids=ids(SMALL))
def test_nothing_outside_a_rows_declared_variables_has_a_derivative(name, form):
    """The dense m x n pass at the wide point: g_all, written block by block over the whole vector, differentiated along
    every variable, against the Jacobian assembled from the per-row closures; and the layout's Jacobian structure holds
    every nonzero of it."""
    M, lay = AC.model(name, form), AC.layout(name, form)
    p, ref = AC.points(name, form)[2], AC.reference(name, form, 2)
    D = AR.dense_jacobian(M, p.x)
    zero = ref.J == 0.0
    noise = AR.SNAP * (1.0 + ref.gscale)[:, None]
    assert (np.abs(D) <= noise)[zero].all(), np.argwhere(zero & (np.abs(D) > noise))[:4]
    assert (np.abs(D - ref.J) <= 2.0 ** -52 * np.abs(ref.J))[~zero].all()
    S = np.zeros((lay.m, lay.n), dtype=bool)
    S[lay.jrow - 1, lay.jcol - 1] = True
    assert not (~S & ~zero).any(), [(M.rows[i].label, AR.var_name(M, j)) for i, j in np.argwhere(~S & ~zero)[:4]]
    T = np.zeros((lay.n, lay.n), dtype=bool)
    T[lay.hrow - 1, lay.hcol - 1] = True
    for k in range(AC.NPOINTS):
        H = AC.reference(name, form, k).H
        assert not (~T & (H != 0.0)).any(), [(AR.var_name(M, i), AR.var_name(M, j)) for i, j in np.argwhere(~T & (H != 0.0))[:4]]


@pytest.mark.parametrize("name,form", STRIDE, ids=ids(STRIDE))
def test_stride_cases_oracle_values_and_jacobian_products(name, form):
    """At n near 16 000 the reference gives values only (O(m) closures).  The oracle's derivative code is exercised through
    J v against (g(x + h v) - g(x - h v)) / 2h at 50 digits: per row |J v - ref| <= (K_J + nnz_i) 2^-52 jscale_i sum_j |v_j|
    over the row's entries -- K_J for the entries, nnz_i for the float64 sum of nnz_i products."""
    M, lay = AC.model(name, form), AC.layout(name, form)
    assert (M.n, M.m) == (lay.n, lay.m)
    SJ, _ = AC.summed(name, form)
    for k in (2,):                          # the wide point
        p = AC.points(name, form)[k]
        R = AC.oracle_reference(name, form, k)
        f, g, fscale = AC.reference_values(name, form, k)
        msgs = AR.compare(M, "f", R.f, f, fscale, AC.K["f"]) + AR.compare(M, "g", R.g, g, R.gscale, AC.K["g"])
        assert not msgs, f"{name} point {k}: " + "; ".join(msgs[:8])
        rng = np.random.default_rng(40 + k)
        for _ in range(2):
            v = rng.standard_normal(lay.n)
            Jv = np.bincount(SJ.row, weights=R.J * v[SJ.col], minlength=lay.m)
            nnz = np.bincount(SJ.row, minlength=lay.m)
            tol = (AC.K["J"] + nnz) * AR.EPS * np.bincount(SJ.row, weights=R.jscale * np.abs(v[SJ.col]), minlength=lay.m)
            d = AR.directional(M, p.x, v)
            bad = np.flatnonzero(np.abs(Jv - d) > tol)
            assert not len(bad), [(M.rows[i].label, Jv[i], d[i]) for i in bad[:4]]


def test_stride_shapes_straddle_one_stride():
    T = AC.TPB
    got = {}
    for name in AC.STRIDE_NAMES:
        net, lay = AC.stride_net(name), AC.layout(name, "acwr")
        got[name] = (net.nb, net.ng, len(lay.sh_bus), net.ndc, net.nl, len(lay.bp_i))
    assert got["below"] == (T - 1,) * 6 and got["at"] == (T,) * 6
    assert got["above"] == (T + 1,) * 4 + (2 * T + 1, 2 * T + 1)
    assert got["pairs"] == (T + 1,) * 4 + (2 * T + 1, T + 1)
    assert (AC.layout("pairs", "acwr").br_sig < 0).any() and AC.stride_net("above").tap is not None


@pytest.mark.parametrize("name", AC.SMALL_NAMES + AC.STRIDE_NAMES)
def test_layout_identities(name):
    net = AC.net_of(name)
    for form in AC.FORMS:
        lay = AC.layout(name, form)
        assert (lay.hrow >= lay.hcol).all() and lay.hcol.min() >= 1 and lay.hrow.max() <= lay.n
        assert lay.jrow.min() >= 1 and lay.jrow.max() <= lay.m and lay.jcol.min() >= 1 and lay.jcol.max() <= lay.n
        assert lay.bal_ptr[0] == 0 and lay.bal_ptr[net.nb] == 2 * net.nl + net.ng + 2 * net.ndc
        assert len(lay.bal_colP) == len(lay.bal_colQ) == len(lay.bal_coef) == lay.bal_ptr[net.nb]
    lay = AC.layout(name, "acwr")
    pairs = sorted({(min(a, b), max(a, b)) for a, b in zip(net.f_bus.tolist(), net.t_bus.tolist())})
    assert len(lay.bp_i) == len(pairs) and list(zip(lay.bp_i.tolist(), lay.bp_j.tolist())) == pairs
    assert (lay.bp_i < lay.bp_j).all()
    assert np.array_equal(lay.br_sig, np.where(net.f_bus < net.t_bus, 1.0, -1.0))
    for l in range(net.nl):
        k = lay.br_bp[l]
        assert (lay.bp_i[k], lay.bp_j[k]) == (min(net.f_bus[l], net.t_bus[l]), max(net.f_bus[l], net.t_bus[l]))
    assert (lay.bp_tmin <= lay.bp_tmax).all() and (lay.bp_tmin < 0).all() and (lay.bp_tmax > 0).all()


def test_small_cases_have_the_topologies_they_are_named_for():
    S = AC.SMALL
    par = AC.layout("parallel", "acwr")
    assert len(par.bp_i) == S["parallel"].nl - 2 and sorted(par.br_sig[:3].tolist()) == [-1.0, 1.0, 1.0]
    assert len({(S["parallel"].angmin[l], S["parallel"].angmax[l]) for l in range(3)}) == 3
    # the fold is the tightest of the three in the pair's orientation: the reversed branch enters with its limits negated
    p = S["parallel"]
    assert np.isclose(par.bp_tmax[0], np.tan(min(p.angmax[0], p.angmax[1], -p.angmin[2])), rtol=1e-15)
    assert np.isclose(par.bp_tmin[0], np.tan(max(p.angmin[0], p.angmin[1], -p.angmax[2])), rtol=1e-15)
    assert (S["reversed"].f_bus > S["reversed"].t_bus).all() and (AC.layout("reversed", "acwr").br_sig == -1.0).all()
    assert S["ref-middle"].ref_bus == 2 and S["ref-last"].ref_bus == S["ref-last"].nb - 1
    g = S["generators"]
    deg = np.bincount(np.concatenate([g.f_bus, g.t_bus]), minlength=g.nb)
    assert (g.gen_bus == 1).sum() == 3 and 2 not in g.gen_bus and g.pd[2] == 0.0 and deg[5] == 1 and 5 in g.gen_bus
    h = S["hub"]
    assert np.bincount(np.concatenate([h.f_bus, h.t_bus]), minlength=h.nb).max() >= 6
    assert (S["outage"].status == 0).sum() == 2
    t = S["transformers"]
    assert (t.tap != 1).any() and (t.shift > 0).any() and (t.shift < 0).any() and (t.shift[t.f_bus > t.t_bus] != 0).any()
    s = S["shunts"]
    assert ((s.gs != 0) & (s.bs == 0)).any() and ((s.gs == 0) & (s.bs != 0)).any() and (s.bs < 0).any()
    assert s.gs[s.ref_bus] != 0 or s.bs[s.ref_bus] != 0
    d = S["dclines"]
    ends = np.concatenate([d.dcline["f_bus"], d.dcline["t_bus"]])
    assert np.bincount(ends).max() >= 2 and d.ref_bus in ends
    ac = {(min(a, b), max(a, b)) for a, b in zip(d.f_bus.tolist(), d.t_bus.tolist())}
    assert any((min(a, b), max(a, b)) in ac for a, b in zip(d.dcline["f_bus"].tolist(), d.dcline["t_bus"].tolist()))
    for net in S.values():
        assert net.nb <= 8 and net.nl <= 14


@pytest.mark.parametrize("form", AC.FORMS)
def test_one_flipped_susceptance_sign_fails_at_its_row(form):
    """The Bs coefficient of the q_f row of branch 3 of the combined network (2 -> 1, a reversed phase shifter), sign
    flipped in the array handed to the oracle: the entrywise comparison reports that row, and only that row."""
    name, l, kind = "combined", 3, 1
    net, lay, M = AC.net_of(name), AC.layout(name, form), AC.model(name, form)
    co = net.branch_coeffs()
    co[l, 3 * kind + 2] = -co[l, 3 * kind + 2]
    assert co[l, 3 * kind + 2] != 0.0
    wrong = dataclasses.replace(net)
    wrong.branch_coeffs = lambda: co
    P = O.problem_acopf(wrong, lay)
    row = [i for i, r in enumerate(M.rows) if r.label.startswith(f"Ohm row q_f of branch {l} ")]
    assert len(row) == 1
    k = 2
    ref, got = AC.reference(name, form, k), AC.oracle_eval(P, AC.points(name, form)[k])
    msgs = AC.check(M, lay, ref, got)
    assert msgs and all(M.rows[row[0]].label in m for m in msgs if " row " in m), msgs[:6]
    _, kg, _ = AR.entrywise(got["g"], ref.g, ref.gscale)
    assert np.flatnonzero(kg > AC.K["g"]).tolist() == row
    _, kj, _ = AR.entrywise(AR.place_J(lay, got["jval"]), ref.J, np.broadcast_to(ref.jscale[:, None], ref.J.shape))
    assert sorted(set(np.argwhere(kj > AC.K["J"])[:, 0].tolist())) == row
