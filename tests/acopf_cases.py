"""Networks and evaluation points for the three dedicated ACOPF evaluators (csrc/acopf_dev.hpp: the polar body of
acopf_eval_dedicated, acr_eval, acwr_eval), their oracle twin (oracle/problems.c) and the layouts of acopf_synth.py.

SMALL: hand-built networks (nb <= 8, nl <= 14) with the topologies case files have and `acopf_synth` never produces --
parallel branches with one reversed, every branch reversed, a reference bus that is not the first, several generators or
none at a bus, a hub, outages, transformers and phase shifters, shunts, dc lines -- and one network with all of it.
STRIDE: `acopf_synth` networks whose loop counts (buses, generators, shunts, dc lines, branches, bus pairs) sit just below,
at and just above one stride of the evaluators' thread loops, the branch loop past two.

Every case comes in the three forms and with three points x: the layout's x0, x0 + 0.05 noise, and a wide point (angles
all over (-pi, pi), magnitudes in [0.5, 1.5], lifted variables off their model values, flows of both signs).  Multipliers
have zeros, negatives and magnitudes from 1e-3 to 1e3; sigma is 0.7 and 0, both at the wide point."""
from __future__ import annotations

import dataclasses
import functools
import zlib

import numpy as np

from sqpsolver_jl_amd.acopf_synth import Network, acopf_synth, acopf_layout, acr_layout, acwr_layout

import acopf_ref as AR

# The stride of every thread loop of the evaluators: TPB = SQPHIP_VEC_THREADS of csrc/dev_util.hpp.  The library does not
# export it; 1024 is what dev_util.hpp defines unless the build overrides it.
TPB = 1024

FORMS = ("polar", "acr", "acwr")
LAYOUT = {"polar": acopf_layout, "acr": acr_layout, "acwr": acwr_layout}

# ---- the constants of |got - ref| <= K * 2^-52 * scale (scales: acopf_ref.py), per output.
# K_ORACLE_MEASURED: the largest error of the CPU oracle against the 50-digit reference over every small case, form and
# point (tests/test_acopf_cases_cpu.py::test_oracle_constants_are_the_measured_ones prints and re-checks them on the CPU).
# K = 4 * K_oracle rounded up to a power of two: the factor 4 covers the device's sincos differing from the C library's
# by a couple of ulp and a different contraction into fused multiply-adds.  Both the oracle and the device are held to K;
# K is never tuned against device output.
# Measured (x86-64 with FMA, glibc sincos; 11 small cases x 3 forms x 4 points):
#     f 0.499    grad 0.0 (2 c2 pg + c1 contracts into one fused multiply-add: correctly rounded)    g 0.813    J 2.50    H 2.46
# so 4 K_oracle = 2.0, 0, 3.25, 10.0, 9.85 -> 2, 1, 4, 16, 16.  The floor of 1 for the gradient: without the contraction
# 2 c2 pg + c1 takes two roundings of at most 2^-53 scale each.
K_ORACLE_MEASURED = {"f": 0.499, "grad": 0.0, "g": 0.813, "J": 2.50, "H": 2.46}
K = {"f": 2.0, "grad": 1.0, "g": 4.0, "J": 16.0, "H": 16.0}


def k_from_measured(k_oracle):
    """4 x the measured constant, rounded up to a power of two (at least 1)"""
    return float(2.0 ** max(0, int(np.ceil(np.log2(max(4.0 * k_oracle, 1e-300))))))


# ------------------------------------------------------------------------------------------------ small networks
def _dc(rows):
    """dc lines from (f_bus, t_bus, loss0, loss1)"""
    k = len(rows)
    return dict(f_bus=np.array([r[0] for r in rows], dtype=np.int32), t_bus=np.array([r[1] for r in rows], dtype=np.int32),
                pminf=np.linspace(-0.3, 0.05, k), pmaxf=np.linspace(0.3, 0.6, k), qminf=np.full(k, -0.4), qmaxf=np.full(k, 0.4),
                qmint=np.full(k, -0.35), qmaxt=np.full(k, 0.45), loss0=np.array([r[2] for r in rows], dtype=np.float64),
                loss1=np.array([r[3] for r in rows], dtype=np.float64))


def _net(seed, nb, branches, gens, ref=0, **kw):
    """A network over the given (f, t) list and generator buses; electrical data drawn like acopf_synth draws it, angle
    limits different on every branch"""
    rng = np.random.default_rng(seed)
    nl, ng = len(branches), len(gens)
    r = rng.uniform(0.005, 0.05, nl)
    x = np.maximum(rng.uniform(0.05, 0.3, nl), 3.0 * r)
    pd = rng.uniform(0.1, 1.0, nb)
    net = Network(
        nb=nb, ng=ng, nl=nl, pd=pd, qd=0.3 * pd, vmin=np.full(nb, 0.94), vmax=np.full(nb, 1.06), ref_bus=ref,
        gen_bus=np.asarray(gens, dtype=np.int32), pmin=np.zeros(ng), pmax=rng.uniform(1.0, 3.0, ng),
        qmin=-rng.uniform(0.5, 1.5, ng), qmax=rng.uniform(0.5, 1.5, ng), c2=rng.uniform(0.01, 0.1, ng) * 1e4,
        c1=rng.uniform(10.0, 40.0, ng) * 100.0,
        f_bus=np.asarray([b[0] for b in branches], dtype=np.int32), t_bus=np.asarray([b[1] for b in branches], dtype=np.int32),
        r=r, x=x, bc=rng.uniform(0.0, 0.1, nl), rate_a=rng.uniform(1.0, 3.0, nl),
        angmin=-rng.uniform(np.pi / 8, np.pi / 3, nl), angmax=rng.uniform(np.pi / 8, np.pi / 3, nl), status=np.ones(nl))
    return dataclasses.replace(net, **kw)


def _small():
    S = {}
    # one pair carrying three branches, two of them 0 -> 1 and one 1 -> 0, with different angle limits each: the W-space
    # form folds the tightest limits over the pair and gives the reversed branch br_sig = -1
    S["parallel"] = _net(11, 4, [(0, 1), (0, 1), (1, 0), (1, 2), (2, 3), (0, 3)], [0, 2])
    S["reversed"] = _net(12, 5, [(1, 0), (2, 1), (3, 2), (4, 3), (4, 0), (3, 1)], [1, 4])
    S["ref-middle"] = _net(13, 5, [(0, 1), (1, 2), (3, 2), (3, 4), (0, 4)], [0, 3], ref=2)
    S["ref-last"] = _net(14, 5, [(0, 1), (2, 1), (2, 3), (3, 4), (4, 0)], [1, 2], ref=4)
    # bus 1: three generators; bus 2: no generator, no load; bus 5: degree 1 with a generator
    g = _net(15, 6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (4, 5), (1, 3)], [1, 1, 1, 5, 0])
    pd = g.pd.copy(); pd[2] = 0.0
    S["generators"] = dataclasses.replace(g, pd=pd, qd=0.3 * pd)
    # bus 3 has degree 8 (seven neighbours, one of them twice), both directions
    S["hub"] = _net(16, 8, [(3, 0), (1, 3), (3, 2), (3, 4), (5, 3), (3, 6), (7, 3), (3, 0), (0, 1), (6, 7)], [3, 6])
    o = _net(17, 5, [(0, 1), (1, 2), (2, 1), (2, 3), (3, 4), (4, 0), (0, 2)], [0, 3])
    st = np.ones(o.nl); st[2] = 0.0; st[5] = 0.0          # one of the parallel pair 1-2, and a single branch
    S["outage"] = dataclasses.replace(o, status=st)
    tr = _net(18, 5, [(0, 1), (2, 1), (2, 3), (4, 3), (4, 0), (1, 3), (3, 1)], [0, 2])
    S["transformers"] = dataclasses.replace(tr, tap=np.array([1.05, 0.94, 1.0, 1.07, 0.97, 1.02, 0.95]),
                                            shift=np.array([0.0, 0.07, -0.05, -0.08, 0.0, 0.06, -0.03]))
    # gs only, bs only, a negative bs, and one at the reference bus (bus 2); bus 4 has none
    S["shunts"] = _net(19, 5, [(0, 1), (1, 2), (3, 2), (3, 4), (4, 0), (1, 3)], [0, 4], ref=2,
                       gs=np.array([0.02, 0.0, 0.015, 0.0, 0.0]), bs=np.array([0.0, 0.12, 0.08, -0.05, 0.0]))
    # two dc lines sharing bus 3, one at the reference bus (1), one alongside the AC branch 0 - 4
    S["dclines"] = _net(20, 5, [(0, 1), (1, 2), (2, 3), (3, 4), (0, 4)], [0, 2], ref=1,
                        dcline=_dc([(3, 1, 0.002, 0.03), (2, 3, 0.0, 0.0), (4, 0, 0.001, 0.05)]))
    c = _net(21, 8, [(0, 1), (0, 1), (1, 0), (2, 1), (3, 2), (3, 4), (5, 3), (3, 6), (7, 3), (3, 0), (3, 1), (6, 7), (4, 5),
                     (7, 6)], [3, 3, 3, 7, 0], ref=5)
    st = np.ones(c.nl); st[1] = 0.0; st[8] = 0.0
    pd = c.pd.copy(); pd[2] = 0.0
    S["combined"] = dataclasses.replace(
        c, status=st, pd=pd, qd=0.3 * pd,
        tap=np.array([1.0, 1.04, 0.95, 1.06, 1.0, 0.93, 1.0, 1.03, 1.05, 1.0, 0.98, 1.0, 1.02, 0.96]),
        shift=np.array([0.0, 0.05, -0.06, 0.08, 0.0, -0.04, 0.0, 0.0, 0.03, 0.0, -0.07, 0.0, 0.0, 0.02]),
        gs=np.array([0.01, 0.0, 0.0, 0.025, 0.0, 0.02, 0.0, 0.0]), bs=np.array([0.0, 0.1, 0.0, -0.04, 0.0, 0.06, -0.02, 0.0]),
        dcline=_dc([(5, 3, 0.002, 0.03), (3, 7, 0.0, 0.02), (6, 7, 0.001, 0.0)]))
    return S


SMALL = _small()
SMALL_NAMES = tuple(SMALL)


# ------------------------------------------------------------------------------------------------ stride networks
def _dress(net, seed, ndc):
    """A third of the branches transformers (a few of them phase shifters), a shunt at every bus, ndc dc lines"""
    rng = np.random.default_rng(seed)
    tr = rng.random(net.nl) < 0.33
    fb = rng.integers(0, net.nb, ndc)
    tb = (fb + 1 + rng.integers(0, net.nb - 1, ndc)) % net.nb
    dc = dict(f_bus=fb.astype(np.int32), t_bus=tb.astype(np.int32), pminf=rng.uniform(-0.3, 0.0, ndc),
              pmaxf=rng.uniform(0.1, 0.6, ndc), qminf=np.full(ndc, -0.4), qmaxf=np.full(ndc, 0.4), qmint=np.full(ndc, -0.4),
              qmaxt=np.full(ndc, 0.4), loss0=rng.uniform(0.0, 0.003, ndc), loss1=rng.uniform(0.0, 0.05, ndc))
    return dataclasses.replace(
        net, tap=np.where(tr, rng.uniform(0.93, 1.07, net.nl), 1.0),
        shift=np.where(tr & (rng.random(net.nl) < 0.3), rng.uniform(-0.08, 0.08, net.nl), 0.0),
        gs=rng.uniform(0.001, 0.03, net.nb), bs=rng.uniform(0.01, 0.19, net.nb) * np.where(rng.random(net.nb) < 0.3, -1.0, 1.0),
        dcline=dc)


def _duplicated(net, extra, seed):
    """`extra` more branches, each alongside an existing one (every other one reversed), with electrical data of their own"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, net.nl, extra)
    rev = (np.arange(extra) % 2).astype(bool)
    f = np.where(rev, net.t_bus[src], net.f_bus[src]).astype(np.int32)
    t = np.where(rev, net.f_bus[src], net.t_bus[src]).astype(np.int32)
    cat = lambda a, b: np.concatenate([a, b])
    r = rng.uniform(0.005, 0.05, extra)
    return dataclasses.replace(
        net, nl=net.nl + extra, f_bus=cat(net.f_bus, f), t_bus=cat(net.t_bus, t), r=cat(net.r, r),
        x=cat(net.x, np.maximum(rng.uniform(0.05, 0.3, extra), 3.0 * r)), bc=cat(net.bc, rng.uniform(0.0, 0.1, extra)),
        rate_a=cat(net.rate_a, net.rate_a[src]), angmin=cat(net.angmin, -rng.uniform(np.pi / 8, np.pi / 4, extra)),
        angmax=cat(net.angmax, rng.uniform(np.pi / 8, np.pi / 4, extra)), status=np.ones(net.nl + extra))


# name -> (nb = ng = nsh = ndc, nl, branches added alongside existing ones)
STRIDE_SHAPES = {
    "below": (TPB - 1, TPB - 1, 0),
    "at": (TPB, TPB, 0),
    "above": (TPB + 1, 2 * TPB + 1, 0),
    "pairs": (TPB + 1, 2 * TPB + 1, TPB),      # nbp = TPB + 1 bus pairs under 2 TPB + 1 branches
}
STRIDE_NAMES = tuple(STRIDE_SHAPES)


@functools.lru_cache(maxsize=None)
def stride_net(name):
    nb, nl, dup = STRIDE_SHAPES[name]
    net = acopf_synth(nb, nb, nl - dup, 7000 + nb + dup)
    if dup:
        net = _duplicated(net, dup, 7100 + nb)
    net = _dress(net, 7200 + nb + dup, nb)
    assert (net.nb, net.ng, net.nl, net.ndc, len(net.shunts()[0])) == (nb, nb, nl, nb, nb)
    return net


def net_of(name):
    return SMALL[name] if name in SMALL else stride_net(name)


@functools.lru_cache(maxsize=None)
def layout(name, form):
    lay = LAYOUT[form](net_of(name))
    for a in (lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.x0):
        a.setflags(write=False)
    return lay


@functools.lru_cache(maxsize=None)
def model(name, form):
    return AR.Model(net_of(name), form)


# ------------------------------------------------------------------------------------------------ points
@dataclasses.dataclass(frozen=True)
class Point:
    x: np.ndarray
    sigma: float
    lam: np.ndarray


def _lam(rng, m):
    lam = rng.choice([-1.0, 1.0], m) * 10.0 ** rng.uniform(-3.0, 3.0, m)
    lam[rng.random(m) < 0.15] = 0.0
    return lam


@functools.lru_cache(maxsize=None)
def points(name, form):
    """(x0, sigma 0.7), (x0 + 0.05 noise, sigma 0), (wide, sigma 0.7), (the same wide x, sigma 0); multipliers differ per point"""
    lay, M = layout(name, form), model(name, form)
    net, o = M.net, M.o
    nb = net.nb
    assert M.n == lay.n
    rng = np.random.default_rng(zlib.crc32(f"{name}/{form}".encode()))
    near = lay.x0 + 0.05 * rng.standard_normal(lay.n)
    wide = rng.uniform(-2.0, 2.0, lay.n)                    # generation, flows of both signs, dc-line variables
    va, vm = rng.uniform(-np.pi, np.pi, nb), rng.uniform(0.5, 1.5, nb)
    if form == "polar":
        wide[o["VA"]:o["VA"] + nb] = va
        wide[o["VM"]:o["VM"] + nb] = vm
    else:
        V = vm * np.exp(1j * va)
        wide[o["VI"]:o["VI"] + nb] = V.imag
        wide[o["VR"]:o["VR"] + nb] = V.real
        if form == "acwr":                                   # lifted variables: the image of V plus noise
            i, j = np.array([p[0] for p in M.pairs]), np.array([p[1] for p in M.pairs])
            P = V[i] * np.conj(V[j])
            wide[o["W"]:o["W"] + nb] = vm ** 2 + 0.1 * rng.standard_normal(nb)
            wide[o["WR"]:o["WR"] + M.nbp] = P.real + 0.1 * rng.standard_normal(M.nbp)
            wide[o["WI"]:o["WI"] + M.nbp] = P.imag + 0.1 * rng.standard_normal(M.nbp)
    pts = (Point(lay.x0.copy(), 0.7, _lam(rng, lay.m)), Point(near, 0.0, _lam(rng, lay.m)), Point(wide, 0.7, _lam(rng, lay.m)),
           Point(wide, 0.0, _lam(rng, lay.m)))
    for p in pts:
        p.x.setflags(write=False); p.lam.setflags(write=False)
    return pts


# ------------------------------------------------------------------------------------------------ references, made once
NPOINTS = 4
_XSLOT = (0, 1, 2, 2)          # points 2 and 3 share their x: the derivatives are formed once


@functools.lru_cache(maxsize=None)
def _derivatives(name, form, slot):
    return AR.derivatives(model(name, form), points(name, form)[slot].x)


@functools.lru_cache(maxsize=None)
def reference(name, form, k):
    """acopf_ref.Result of point k of a small case"""
    p = points(name, form)[k]
    return AR.combine(model(name, form), _derivatives(name, form, _XSLOT[k]), p.sigma, p.lam)


@functools.lru_cache(maxsize=None)
def reference_values(name, form, k):
    """(f, g, fscale) of point k of any case at 50 digits: values only"""
    return AR.values(model(name, form), points(name, form)[k].x)


def check(M, lay, ref, got, Kc=None):
    """Failure messages of an evaluation `got` = dict(f, grad, g, jval, hval) against an acopf_ref.Result"""
    Kc = Kc or K
    out = AR.compare(M, "f", got["f"], ref.f, ref.fscale, Kc["f"])
    out += AR.compare(M, "grad", got["grad"], ref.grad, ref.gradscale, Kc["grad"])
    out += AR.compare(M, "g", got["g"], ref.g, ref.gscale, Kc["g"])
    out += AR.compare(M, "J", AR.place_J(lay, got["jval"]), ref.J, np.broadcast_to(ref.jscale[:, None], ref.J.shape), Kc["J"])
    out += AR.compare(M, "H", AR.place_H(lay, got["hval"]), ref.H, ref.hscale, Kc["H"])
    return out


def oracle_eval(P, p):
    return dict(f=P.eval_f(p.x), grad=P.eval_grad_f(p.x), g=P.eval_g(p.x), jval=P.eval_jac_g(p.x),
                hval=P.eval_h(p.x, p.sigma, p.lam))


# ------------------------------------------------------------------------------------------------ stride cases: the oracle as reference
class Summed:
    """The distinct (row, column) positions of a 1-based COO structure and the sum of a value list over the entries of each"""

    def __init__(self, row1, col1, ncol):
        key = (np.asarray(row1, dtype=np.int64) - 1) * ncol + (np.asarray(col1, dtype=np.int64) - 1)
        uniq, self.inv = np.unique(key, return_inverse=True)
        self.row, self.col = uniq // ncol, uniq % ncol
        self.key, self.ncol = uniq, ncol

    def __call__(self, val):
        return np.bincount(self.inv, weights=np.asarray(val, dtype=np.float64), minlength=len(self.key))


@functools.lru_cache(maxsize=None)
def summed(name, form):
    lay = layout(name, form)
    return Summed(lay.jrow, lay.jcol, lay.n), Summed(lay.hrow, lay.hcol, lay.n)


@dataclasses.dataclass
class OracleRef:
    """The oracle's outputs at a point with the scales of acopf_ref.py formed from the oracle's own values; J, H and their
    scales are lists over the distinct positions of `summed`"""
    f: float
    fscale: float
    grad: np.ndarray
    gradscale: np.ndarray
    g: np.ndarray
    gscale: np.ndarray
    J: np.ndarray
    jscale: np.ndarray
    H: np.ndarray
    hscale: np.ndarray


def _row_class(label):
    return label.split(" of ")[0]


@functools.lru_cache(maxsize=None)
def oracle_reference(name, form, k):
    """hscale needs max |d2 g_i| per row and the positions a row's second derivatives occupy.  Both come from the oracle's
    Hessian callback itself: within one class of rows (the rows of one kind: one Ohm flow, one side of the thermal limits,
    ...) no COO slot is fed by two rows, so a call with lambda = 1 on the class gives the slot's coefficient u and a call
    with lambda_i = i + 1 gives (i + 1) u: the owner of every slot with u != 0."""
    from oracle import oracle as O
    M, lay, p = model(name, form), layout(name, form), points(name, form)[k]
    net = M.net
    P = O.problem_acopf(net, lay)
    ev = oracle_eval(P, p)
    SJ, SH = summed(name, form)
    ax = np.abs(p.x)
    pg = p.x[M.o["PG"]:M.o["PG"] + net.ng]
    fscale = net.ng * float(np.sum(np.abs(net.c2 * pg * pg) + np.abs(net.c1 * pg)))
    gradscale = np.zeros(lay.n)
    gradscale[M.o["PG"]:M.o["PG"] + net.ng] = np.abs(2 * net.c2 * pg) + np.abs(net.c1)
    J = SJ(ev["jval"])
    jscale_row = np.zeros(lay.m); np.maximum.at(jscale_row, SJ.row, np.abs(J))
    gscale = np.abs(ev["g"]) + np.bincount(SJ.row, weights=np.abs(J) * ax[SJ.col], minlength=lay.m)
    hscale = SH(np.abs(P.eval_h(p.x, 1.0, np.zeros(lay.m)))) * abs(p.sigma)
    classes = {}
    for i, row in enumerate(M.rows):
        classes.setdefault(_row_class(row.label), []).append(i)
    hmax = np.zeros(lay.m)
    owned = []
    for rows in classes.values():
        rows = np.asarray(rows)
        l1 = np.zeros(lay.m); l1[rows] = 1.0
        l2 = np.zeros(lay.m); l2[rows] = rows + 1.0
        u, v = P.eval_h(p.x, 0.0, l1), P.eval_h(p.x, 0.0, l2)
        s = np.flatnonzero(u != 0.0)
        if not len(s):
            continue
        q = v[s] / u[s]
        owner = np.rint(q).astype(np.int64) - 1
        assert np.abs(q - (owner + 1)).max() <= 1e-6 and np.isin(owner, rows).all(), "a Hessian slot fed by two rows of one class"
        np.maximum.at(hmax, owner, np.abs(u[s]))
        owned.append((owner, SH.inv[s]))
    if owned:
        owner, pos = np.concatenate([a for a, _ in owned]), np.concatenate([b for _, b in owned])
        pair = np.unique(owner * len(SH.key) + pos)                    # a row counts once per position
        owner, pos = pair // len(SH.key), pair % len(SH.key)
        hscale += np.bincount(pos, weights=np.abs(p.lam[owner]) * hmax[owner], minlength=len(SH.key))
    return OracleRef(ev["f"], fscale, ev["grad"], gradscale, ev["g"], gscale, J, jscale_row[SJ.row], SH(ev["hval"]), hscale)


def check_against_oracle(name, form, k, got):
    """Failure messages of `got` = dict(f, grad, g, jval, hval) against the oracle at point k, entry by entry"""
    M, R = model(name, form), oracle_reference(name, form, k)
    SJ, SH = summed(name, form)
    out = AR.compare(M, "f", got["f"], R.f, R.fscale, K["f"])
    out += AR.compare(M, "grad", got["grad"], R.grad, R.gradscale, K["grad"])
    out += AR.compare(M, "g", got["g"], R.g, R.gscale, K["g"])
    out += AR.compare(M, "J", SJ(got["jval"]), R.J, R.jscale, K["J"], at=(SJ.row, SJ.col))
    out += AR.compare(M, "H", SH(got["hval"]), R.H, R.hscale, K["H"], at=(SH.row, SH.col))
    return out
