"""An independent reference of the three ACOPF forms (polar, rectangular, W-space) in 50-digit arithmetic (mpmath).

Nothing here is taken from the evaluators: no `Network.branch_coeffs()`, none of the twelve coefficients per branch, no
Jacobian or Hessian formula.  Every row is written from the physics over complex numbers,

    branch      pi-model with an ideal transformer tau e^{j phi} at the from end, y = 1 / (r + j x):
                    I_f = (y + j bc/2) / tau^2 V_f - y / (tau e^{-j phi}) V_t
                    I_t = -y / (tau e^{j phi}) V_f + (y + j bc/2) V_t
                S_f = V_f conj(I_f), S_t = V_t conj(I_t); an outaged branch (status 0) carries nothing
    Ohm rows    flow variable - Re / Im of S_f, S_t
    balance     sum of the flow variables leaving the bus (AC arcs, dc-line ends) - generation + conj(gs + j bs) |V|^2
    thermal     p^2 + q^2 at either end
    dc line     (1 - loss1) p_f + p_t
    cost        sum c2 pg^2 + c1 pg

with V = vm e^{j va} (polar) or vr + j vi (rectangular).  The W-space form is the same physics with |V_i|^2 -> w_i and
V_i conj(V_j) -> wr_k + j wi_k for the pair k = (i < j) (conjugated for a branch that runs from j to i), the angle rows
wi_k - tan(limit) wr_k with the tightest limits over the branches of the pair, and the model-voltage rows that tie
w, wr, wi to vr, vi.  From the layouts only the ORDER of variables and rows is taken (the docstrings of acopf_layout,
acr_layout, acwr_layout); a layout's jrow / jcol / hrow / hcol are used by `place_*` to put a COO value list into a dense
matrix and nowhere else, so they never decide which derivatives exist.

Two implementations live side by side and check each other: `Model.g_all` evaluates every row from the whole vector x,
block by block; `Model.rows` holds one closure per row over that row's own variables.  First and second derivatives are
central differences of the closures at 50 digits (steps 1e-15 and 1e-12: truncation below 1e-24 of the row's scale, far
under one float64 ulp), over the row's own variables only -- O(nnz) work.  `dense_jacobian` differentiates `g_all` along
every variable: it shows that nothing outside a row's declared variables has a derivative.

A difference quotient of an exactly vanishing derivative is rounding noise near 1e-26, not 0: a derivative below
1e-18 of the row's scale (|g_i| + sum_j |dg_i/dx_j| |x_j| + 1) is SNAPPED to an exact zero, and an evaluator must then
return an exact zero there.

Scales of the comparison (`Result`):
    jscale_i   max_j |J_ij|
    gscale_i   |g_i| + sum_j |J_ij| |x_j|
    hscale_jk  sigma |d2f|_jk + sum_i |lambda_i| max|d2 g_i| [j and k are variables of row i]
    fscale     ng * (sum |c2 pg^2| + |c1 pg|): the objective is one float64 sum of ng terms, serial in the oracle and a tree
               on the device, and a sum of N terms in any order is off by at most (N - 1) 2^-53 sum |t_i| (Higham, Accuracy
               and Stability of Numerical Algorithms, section 4.2) -- without the factor the bound would shrink, relative
               to what a correct serial sum can do, as the network grows
    gradscale_j  |2 c2 pg| + |c1|
"""
from __future__ import annotations

import dataclasses

import mpmath as mp
import numpy as np

DPS = 50
EPS = 2.0 ** -52
SNAP = 1e-18


def _steps():
    return mp.mpf(10) ** -15, mp.mpf(10) ** -12


# ------------------------------------------------------------------------------------------------ physics
def _admittances(net, l):
    """(Yff, Yft, Ytf, Ytt) of branch l: I_f = Yff V_f + Yft V_t, I_t = Ytf V_f + Ytt V_t"""
    if float(net.status[l]) == 0.0:
        z = mp.mpc(0)
        return z, z, z, z
    y = 1 / mp.mpc(mp.mpf(float(net.r[l])), mp.mpf(float(net.x[l])))
    ysh = y + mp.mpc(0, mp.mpf(float(net.bc[l])) / 2)
    tau = mp.mpf(1.0 if net.tap is None else float(net.tap[l]))
    phi = mp.mpf(0.0 if net.shift is None else float(net.shift[l]))
    return ysh / tau ** 2, -y / (tau * mp.expj(-phi)), -y / (tau * mp.expj(phi)), ysh


def _flows_v(Y, Vf, Vt):
    """S_f, S_t from the end voltages: S = V conj(I)"""
    If = Y[0] * Vf + Y[1] * Vt
    It = Y[2] * Vf + Y[3] * Vt
    return Vf * mp.conj(If), Vt * mp.conj(It)


def _flows_w(Y, wf, wt, P):
    """The same S = V conj(I), expanded: V_f conj(Yff V_f + Yft V_t) = conj(Yff) |V_f|^2 + conj(Yft) V_f conj(V_t), with
    |V_f|^2 -> wf, |V_t|^2 -> wt, V_f conj(V_t) -> P (so V_t conj(V_f) -> conj(P))"""
    return mp.conj(Y[0]) * wf + mp.conj(Y[1]) * P, mp.conj(Y[3]) * wt + mp.conj(Y[2]) * mp.conj(P)


def _part(S, k):
    return (S[0].real, S[0].imag, S[1].real, S[1].imag)[k]


@dataclasses.dataclass
class Row:
    vars: list          # 0-based variable indices the closure reads, in the order of its argument
    fn: object          # fn(list of mpf) -> mpf
    label: str          # names the row for a failure message: kind, branch / bus / pair


class Model:
    """Variable and row order of one form of one network, its rows as closures, and `g_all`."""

    def __init__(self, net, form):
        assert form in ("polar", "acr", "acwr")
        self.net, self.form = net, form
        nb, ng, nl, ndc = net.nb, net.ng, net.nl, net.ndc
        self.f = [int(a) for a in net.f_bus]
        self.t = [int(a) for a in net.t_bus]
        with mp.workdps(DPS):
            self.Y = [_admittances(net, l) for l in range(nl)]
            gs = np.zeros(nb) if net.gs is None else np.asarray(net.gs, dtype=np.float64)
            bs = np.zeros(nb) if net.bs is None else np.asarray(net.bs, dtype=np.float64)
            self.ysh = [mp.conj(mp.mpc(mp.mpf(float(gs[i])), mp.mpf(float(bs[i])))) for i in range(nb)]
            self.c2 = [mp.mpf(float(a)) for a in net.c2]
            self.c1 = [mp.mpf(float(a)) for a in net.c1]
            self.dck = [1 - mp.mpf(float(a)) for a in net.dcline["loss1"]] if ndc else []
        # ---- variable order
        o = {}
        if form == "acwr":
            pairs = sorted({(min(a, b), max(a, b)) for a, b in zip(self.f, self.t)})
            self.pairs = pairs
            lut = {p: k for k, p in enumerate(pairs)}
            self.pair_of = [lut[(min(a, b), max(a, b))] for a, b in zip(self.f, self.t)]
            nbp = len(pairs)
            o["VI"], o["VR"], o["W"], o["WR"], o["WI"] = 0, nb, 2 * nb, 3 * nb, 3 * nb + nbp
            o["PG"] = 3 * nb + 2 * nbp
        else:
            nbp = 0
            self.pairs = []
            o["VA" if form == "polar" else "VI"], o["VM" if form == "polar" else "VR"] = 0, nb
            o["PG"] = 2 * nb
        self.nbp = nbp
        o["QG"] = o["PG"] + ng
        o["PF"] = o["QG"] + ng
        o["PT"], o["QF"], o["QT"] = o["PF"] + nl, o["PF"] + 2 * nl, o["PF"] + 3 * nl
        o["DPF"] = o["PF"] + 4 * nl
        o["DPT"], o["DQF"], o["DQT"] = o["DPF"] + ndc, o["DPF"] + 2 * ndc, o["DPF"] + 3 * ndc
        self.o = o
        self.n = o["DPF"] + 4 * ndc
        # ---- what leaves each bus: (P variable, Q variable, sign)
        inc = [[] for _ in range(nb)]
        for l in range(nl):
            inc[self.f[l]].append((o["PF"] + l, o["QF"] + l, 1))
            inc[self.t[l]].append((o["PT"] + l, o["QT"] + l, 1))
        for g in range(ng):
            inc[int(net.gen_bus[g])].append((o["PG"] + g, o["QG"] + g, -1))
        for d in range(ndc):
            inc[int(net.dcline["f_bus"][d])].append((o["DPF"] + d, o["DQF"] + d, 1))
            inc[int(net.dcline["t_bus"][d])].append((o["DPT"] + d, o["DQT"] + d, 1))
        self.inc = inc
        if form == "acwr":
            with mp.workdps(DPS):
                lo = [-mp.inf] * nbp
                hi = [mp.inf] * nbp
                for l in range(nl):
                    a, b = mp.mpf(float(net.angmin[l])), mp.mpf(float(net.angmax[l]))
                    if self.f[l] > self.t[l]:           # the limits bound va_f - va_t; the pair's angle is va_i - va_j, i < j
                        a, b = -b, -a
                    k = self.pair_of[l]
                    lo[k], hi[k] = max(lo[k], a), min(hi[k], b)
                self.tlo, self.thi = [mp.tan(a) for a in lo], [mp.tan(b) for b in hi]
        self.rows = self._rows()
        self.m = len(self.rows)

    # -------------------------------------------------------------------------------------------- voltages
    def _V(self, a, b):
        """bus voltage from its two coordinates in variable order: (va, vm) polar, (vi, vr) rectangular"""
        return b * mp.expj(a) if self.form == "polar" else mp.mpc(b, a)

    def _Pft(self, l, wr, wi):
        return mp.mpc(wr, wi) if self.f[l] < self.t[l] else mp.mpc(wr, -wi)

    # -------------------------------------------------------------------------------------------- per-row closures
    def _rows(self):
        net, o, form = self.net, self.o, self.form
        nb, nl, ndc, nbp = net.nb, net.nl, net.ndc, self.nbp
        A, B = (o["VA"], o["VM"]) if form == "polar" else (o["VI"], o["VR"])
        f, t = self.f, self.t

        def angle(l):
            return Row([A + f[l], A + t[l]], lambda v: v[0] - v[1], f"angle difference of branch {l} ({f[l]}->{t[l]})")

        def ref():
            return Row([A + net.ref_bus], lambda v: v[0], f"reference row (bus {net.ref_bus})")

        def balance(i, q):
            terms = self.inc[i]
            lin = [(tv[1] if q else tv[0]) for tv in terms]
            sg = [tv[2] for tv in terms]
            volt = [o["W"] + i] if form == "acwr" else [A + i, B + i]
            ysh = self.ysh[i]
            nt = len(lin)

            def fn(v):
                s = mp.mpf(0)
                for k in range(nt):
                    s += sg[k] * v[k]
                w = v[nt] if form == "acwr" else abs(self._V(v[nt], v[nt + 1])) ** 2
                S = ysh * w
                return s + (S.imag if q else S.real)
            return Row(lin + volt, fn, f"{'Q' if q else 'P'} balance of bus {i}")

        def thermal(l, to):
            p, q = (o["PT"] + l, o["QT"] + l) if to else (o["PF"] + l, o["QF"] + l)
            return Row([p, q], lambda v: v[0] ** 2 + v[1] ** 2, f"thermal limit, {'to' if to else 'from'} end of branch {l} ({f[l]}->{t[l]})")

        def ohm(l, k):
            own = (o["PF"], o["QF"], o["PT"], o["QT"])[k] + l
            Y = self.Y[l]
            lab = f"Ohm row {('p_f', 'q_f', 'p_t', 'q_t')[k]} of branch {l} ({f[l]}->{t[l]})"
            if form == "acwr":
                kk = self.pair_of[l]
                vs = [own, o["W"] + f[l], o["W"] + t[l], o["WR"] + kk, o["WI"] + kk]
                return Row(vs, lambda v: v[0] - _part(_flows_w(Y, v[1], v[2], self._Pft(l, v[3], v[4])), k), lab)
            vs = [own, A + f[l], B + f[l], A + t[l], B + t[l]]
            return Row(vs, lambda v: v[0] - _part(_flows_v(Y, self._V(v[1], v[2]), self._V(v[3], v[4])), k), lab)

        def dcloss(d):
            c = self.dck[d]
            return Row([o["DPF"] + d, o["DPT"] + d], lambda v: c * v[0] + v[1], f"loss row of dc line {d}")

        def vmag(i, which):
            return Row([A + i, B + i], lambda v: abs(self._V(v[0], v[1])) ** 2, f"voltage magnitude row ({which}) of bus {i}")

        rows = []
        if form == "polar":
            rows += [angle(l) for l in range(nl)] + [angle(l) for l in range(nl)] + [ref()]
            for i in range(nb):
                rows += [balance(i, 0), balance(i, 1)]
            for l in range(nl):
                rows += [thermal(l, 0), thermal(l, 1)]
            rows += [ohm(l, k) for l in range(nl) for k in range(4)]
        elif form == "acr":
            rows.append(ref())
            for i in range(nb):
                rows += [balance(i, 0), balance(i, 1)]
            for i in range(nb):
                rows += [vmag(i, "lower"), vmag(i, "upper")]
            for l in range(nl):
                rows += [thermal(l, 0), thermal(l, 1)]
            rows += [ohm(l, k) for l in range(nl) for k in range(4)]
        else:
            rows.append(ref())
            for i in range(nb):
                rows += [balance(i, 0), balance(i, 1)]
            for k in range(nbp):
                i, j = self.pairs[k]
                for tn, nm in ((self.thi[k], "upper"), (self.tlo[k], "lower")):
                    rows.append(Row([o["WI"] + k, o["WR"] + k], lambda v, tn=tn: v[0] - tn * v[1],
                                    f"angle row ({nm}) of bus pair {k} ({i},{j})"))
            rows += [ohm(l, k) for l in range(nl) for k in range(4)]
            for i in range(nb):
                rows.append(Row([o["W"] + i, A + i, B + i], lambda v: v[0] - abs(self._V(v[1], v[2])) ** 2,
                                f"model-voltage row w of bus {i}"))
            for k in range(nbp):
                i, j = self.pairs[k]
                vs = [A + i, B + i, A + j, B + j]
                rows.append(Row([o["WR"] + k] + vs, lambda v: v[0] - (self._V(v[1], v[2]) * mp.conj(self._V(v[3], v[4]))).real,
                                f"model-voltage row wr of bus pair {k} ({i},{j})"))
                rows.append(Row([o["WI"] + k] + vs, lambda v: v[0] - (self._V(v[1], v[2]) * mp.conj(self._V(v[3], v[4]))).imag,
                                f"model-voltage row wi of bus pair {k} ({i},{j})"))
            for l in range(nl):
                rows += [thermal(l, 0), thermal(l, 1)]
        rows += [dcloss(d) for d in range(ndc)]
        return rows

    # -------------------------------------------------------------------------------------------- whole-vector evaluation
    def g_all(self, x):
        """Every row from the whole vector x (list of mpf), block by block; each branch's flows are formed once."""
        net, o, form = self.net, self.o, self.form
        nb, nl, ndc, nbp = net.nb, net.nl, net.ndc, self.nbp
        f, t = self.f, self.t
        if form == "acwr":
            S = [_flows_w(self.Y[l], x[o["W"] + f[l]], x[o["W"] + t[l]],
                          self._Pft(l, x[o["WR"] + self.pair_of[l]], x[o["WI"] + self.pair_of[l]])) for l in range(nl)]
            V = [mp.mpc(x[o["VR"] + i], x[o["VI"] + i]) for i in range(nb)]
            W = [x[o["W"] + i] for i in range(nb)]
        else:
            V = [x[nb + i] * mp.expj(x[i]) if form == "polar" else mp.mpc(x[nb + i], x[i]) for i in range(nb)]
            S = [_flows_v(self.Y[l], V[f[l]], V[t[l]]) for l in range(nl)]
            W = [abs(v) ** 2 for v in V]
        bal = []
        for i in range(nb):
            sh = self.ysh[i] * W[i]
            bal.append(sum((sg * x[p] for p, _, sg in self.inc[i]), mp.mpf(0)) + sh.real)
            bal.append(sum((sg * x[q] for _, q, sg in self.inc[i]), mp.mpf(0)) + sh.imag)
        th = []
        for l in range(nl):
            th.append(x[o["PF"] + l] ** 2 + x[o["QF"] + l] ** 2)
            th.append(x[o["PT"] + l] ** 2 + x[o["QT"] + l] ** 2)
        ohm = []
        for l in range(nl):
            ohm += [x[o["PF"] + l] - S[l][0].real, x[o["QF"] + l] - S[l][0].imag,
                    x[o["PT"] + l] - S[l][1].real, x[o["QT"] + l] - S[l][1].imag]
        dc = [self.dck[d] * x[o["DPF"] + d] + x[o["DPT"] + d] for d in range(ndc)]
        if form == "polar":
            ang = [x[f[l]] - x[t[l]] for l in range(nl)]
            return ang + ang + [x[net.ref_bus]] + bal + th + ohm + dc
        if form == "acr":
            vm = [w for w in W for _ in (0, 1)]
            return [x[net.ref_bus]] + bal + vm + th + ohm + dc
        ang = []
        for k in range(nbp):
            ang += [x[o["WI"] + k] - self.thi[k] * x[o["WR"] + k], x[o["WI"] + k] - self.tlo[k] * x[o["WR"] + k]]
        mv = [W[i] - abs(V[i]) ** 2 for i in range(nb)]
        for k, (i, j) in enumerate(self.pairs):
            P = V[i] * mp.conj(V[j])
            mv += [x[o["WR"] + k] - P.real, x[o["WI"] + k] - P.imag]
        return [x[net.ref_bus]] + bal + ang + ohm + mv + th + dc

    def cost(self, x):
        pg = self.o["PG"]
        return sum((self.c2[g] * x[pg + g] ** 2 + self.c1[g] * x[pg + g] for g in range(self.net.ng)), mp.mpf(0))


def _mpx(x):
    return [mp.mpf(float(a)) for a in x]


# ------------------------------------------------------------------------------------------------ values only (O(m))
def values(model, x):
    """(f, g) as float64 arrays rounded once from 50 digits, and fscale (module docstring)"""
    with mp.workdps(DPS):
        xm = _mpx(x)
        g = np.array([float(a) for a in model.g_all(xm)])
        f = float(model.cost(xm))
        pg = model.o["PG"]
        fscale = model.net.ng * float(sum((abs(model.c2[k] * xm[pg + k] ** 2) + abs(model.c1[k] * xm[pg + k]) for k in range(model.net.ng)), mp.mpf(0)))
    return f, g, fscale


def directional(model, x, v):
    """dg/dt of g(x + t v) at t = 0 by a central difference at 50 digits"""
    with mp.workdps(DPS):
        h = _steps()[0]
        xm, vm = _mpx(x), _mpx(v)
        gp = model.g_all([a + h * b for a, b in zip(xm, vm)])
        gm = model.g_all([a - h * b for a, b in zip(xm, vm)])
        return np.array([float((p - q) / (2 * h)) for p, q in zip(gp, gm)])


def dense_jacobian(model, x):
    """dg_i/dx_j for EVERY i and j, by central differences of g_all along each variable: the structure check"""
    with mp.workdps(DPS):
        h = _steps()[0]
        xm = _mpx(x)
        J = np.zeros((model.m, model.n))
        for j in range(model.n):
            xp = list(xm); xq = list(xm)
            xp[j] += h; xq[j] -= h
            gp, gq = model.g_all(xp), model.g_all(xq)
            J[:, j] = [float((p - q) / (2 * h)) for p, q in zip(gp, gq)]
    return J


# ------------------------------------------------------------------------------------------------ derivatives per row
@dataclasses.dataclass
class Derivs:
    """What depends on x alone: values and, per row, first and second derivatives over the row's own variables (mpf)"""
    x: np.ndarray
    f: object
    g: list
    d1: list      # per row: list of mpf, aligned with row.vars
    d2: list      # per row: {(a, b): mpf}, a >= b positions in row.vars, snapped entries absent
    fd1: dict     # {j: mpf} of the cost
    fd2: dict     # {j: mpf} diagonal second derivatives of the cost


def derivatives(model, x):
    with mp.workdps(DPS):
        h1, h2 = _steps()
        xm = _mpx(x)
        gall = model.g_all(xm)
        g, d1, d2 = [], [], []
        for i, row in enumerate(model.rows):
            v = [xm[j] for j in row.vars]
            nv = len(v)
            g0 = row.fn(v)
            assert abs(g0 - gall[i]) <= mp.mpf(10) ** -40 * (1 + abs(g0)), f"row closure and g_all disagree: {row.label}"

            def at(shifts, h):
                w = list(v)
                for a, s in shifts:
                    w[a] += s * h
                return row.fn(w)
            one = [(at([(a, 1)], h1) - at([(a, -1)], h1)) / (2 * h1) for a in range(nv)]
            scale = 1 + abs(g0) + sum((abs(one[a] * v[a]) for a in range(nv)), mp.mpf(0))
            tiny = mp.mpf(SNAP) * scale
            one = [d if abs(d) > tiny else mp.mpf(0) for d in one]
            plus = [at([(a, 1)], h2) for a in range(nv)]
            minus = [at([(a, -1)], h2) for a in range(nv)]
            two = {}
            for a in range(nv):
                d = (plus[a] - 2 * g0 + minus[a]) / h2 ** 2
                if abs(d) > tiny:
                    two[a, a] = d
                for b in range(a):
                    d = (at([(a, 1), (b, 1)], h2) - at([(a, 1), (b, -1)], h2) - at([(a, -1), (b, 1)], h2)
                         + at([(a, -1), (b, -1)], h2)) / (4 * h2 ** 2)
                    if abs(d) > tiny:
                        two[a, b] = d
            g.append(g0); d1.append(one); d2.append(two)
        # the cost: a closure per generator over its own variable
        pg = model.o["PG"]
        fd1, fd2 = {}, {}
        for k in range(model.net.ng):
            c = lambda p, k=k: model.c2[k] * p ** 2 + model.c1[k] * p
            p0 = xm[pg + k]
            fd1[pg + k] = (c(p0 + h1) - c(p0 - h1)) / (2 * h1)
            fd2[pg + k] = (c(p0 + h2) - 2 * c(p0) + c(p0 - h2)) / h2 ** 2
        return Derivs(np.asarray(x, dtype=np.float64).copy(), model.cost(xm), g, d1, d2, fd1, fd2)


@dataclasses.dataclass
class Result:
    f: float
    fscale: float
    grad: np.ndarray
    gradscale: np.ndarray
    g: np.ndarray
    gscale: np.ndarray
    J: np.ndarray          # dense m x n
    jscale: np.ndarray     # per row
    H: np.ndarray          # dense n x n, lower triangle
    hscale: np.ndarray     # dense n x n, lower triangle


def combine(model, D, sigma, lam):
    """The reference outputs at (x, sigma, lambda) from the derivatives at x; every sum in 50 digits, rounded once."""
    n, m = model.n, model.m
    with mp.workdps(DPS):
        xm = _mpx(D.x)
        pg = model.o["PG"]
        fscale = model.net.ng * float(sum((abs(model.c2[k] * xm[pg + k] ** 2) + abs(model.c1[k] * xm[pg + k]) for k in range(model.net.ng)), mp.mpf(0)))
        grad = np.zeros(n); gradscale = np.zeros(n)
        for k in range(model.net.ng):
            grad[pg + k] = float(D.fd1[pg + k])
            gradscale[pg + k] = float(abs(2 * model.c2[k] * xm[pg + k]) + abs(model.c1[k]))
        g = np.array([float(a) for a in D.g])
        J = np.zeros((m, n)); gscale = np.abs(g).copy()
        Jm = {}
        for i, row in enumerate(model.rows):
            for a, j in enumerate(row.vars):        # a row never lists a variable twice
                Jm[i, j] = Jm.get((i, j), mp.mpf(0)) + D.d1[i][a]
        for (i, j), d in Jm.items():
            J[i, j] = float(d)
            gscale[i] += float(abs(d * xm[j]))
        jscale = np.abs(J).max(axis=1)
        sg = mp.mpf(float(sigma))
        Hm = {}
        hscale = np.zeros((n, n))
        for j, d in D.fd2.items():
            Hm[j, j] = sg * d
            hscale[j, j] += float(abs(sg * d))
        for i, row in enumerate(model.rows):
            li = mp.mpf(float(lam[i]))
            hmax = max((abs(d) for d in D.d2[i].values()), default=mp.mpf(0))
            for (a, b), d in D.d2[i].items():
                j, k = row.vars[a], row.vars[b]
                key = (max(j, k), min(j, k))
                Hm[key] = Hm.get(key, mp.mpf(0)) + li * d
            w = float(abs(li) * hmax)
            if w > 0.0:
                vs = row.vars
                for a in range(len(vs)):
                    for b in range(a + 1):
                        hscale[max(vs[a], vs[b]), min(vs[a], vs[b])] += w
        H = np.zeros((n, n))
        for (j, k), d in Hm.items():
            H[j, k] = float(d)
    return Result(float(D.f), fscale, grad, gradscale, g, gscale, J, jscale, H, hscale)


# ------------------------------------------------------------------------------------------------ placing and comparing
def place_J(lay, jval):
    J = np.zeros((lay.m, lay.n))
    np.add.at(J, (np.asarray(lay.jrow) - 1, np.asarray(lay.jcol) - 1), jval)
    return J


def place_H(lay, hval):
    H = np.zeros((lay.n, lay.n))
    np.add.at(H, (np.asarray(lay.hrow) - 1, np.asarray(lay.hcol) - 1), hval)
    return H


def entrywise(got, ref, scale):
    """(K, failures): K = the largest |got - ref| / (EPS scale) over the entries whose reference is not an exact zero;
    failures = indices where the reference is an exact zero and `got` is not (K says nothing about those)."""
    got, ref, scale = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    zero = ref == 0.0
    bad = np.argwhere(zero & (got != 0.0))
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(zero, 0.0, err / (EPS * scale))
    k = np.where(np.isnan(k), np.inf, k)
    return (float(k.max()) if k.size else 0.0), k, [tuple(int(a) for a in ix) for ix in bad]


def var_name(model, j):
    names = sorted(((off, nm) for nm, off in model.o.items()), reverse=True)
    for off, nm in names:
        if j >= off:
            return f"{nm}[{j - off}]"
    return str(j)


def compare(model, what, got, ref, scale, K, at=None):
    """Messages of every entry of output `what` ('f', 'grad', 'g', 'J', 'H') that misses |got - ref| <= K EPS scale, or is
    nonzero where the reference is an exact zero; empty when all is well.  Each names form, row or entry, branch or bus.
    `at`: for J and H given as flat lists of summed entries, the (row, column) of every list position."""
    got, ref, scale = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (got, ref, scale))
    _, k, bad = entrywise(got, ref, scale)
    out = []

    def where(ix):
        if at is not None:
            ix = (int(at[0][ix[0]]), int(at[1][ix[0]]))
        if what == "f":
            return "objective"
        if what == "grad":
            return f"gradient entry {var_name(model, ix[0])}"
        if what == "g":
            return f"row {ix[0]}: {model.rows[ix[0]].label}"
        if what == "J":
            return f"Jacobian row {ix[0]} ({model.rows[ix[0]].label}), column {var_name(model, ix[1])}"
        return f"Hessian entry ({var_name(model, ix[0])}, {var_name(model, ix[1])})"
    for ix in bad:
        out.append(f"{model.form} {where(ix)}: reference is exactly 0, got {got[ix]!r}")
    for ix in np.argwhere(k > K):
        ix = tuple(int(a) for a in ix)
        out.append(f"{model.form} {where(ix)}: got {got[ix]!r}, reference {ref[ix]!r}, error {k[ix]:.3g} eps scale > {K}")
    return out
