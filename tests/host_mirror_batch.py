"""Lockstep driver for many host models on one context -- TEST HARNESS, not product.

tests/host_mirror.py runs one `SqpTR` over the scalar seat: every numerical step is one library call on a context of
its own.  A host that drives N models (contingency scenarios, multistart, a parameter sweep) can instead keep them
in step: each model runs until it needs the library, the driver gathers the pending requests of all models that are still
running, issues one `*_batch` call per kind of request and hands every model its own result.  Model k lives on
instance k of one shared context (its bounds through set_bounds).

`SqpTRLockstep.steps()` is `SqpTR.run()` of host_mirror line by line, written as a generator: where run() calls the
context, steps() yields the request and receives the result.  No threads; the models interleave only at those points.
Requests:
    ("qp", mode, x_k, delta, mu, df, E, jval, hval)       -> dict of Context.qp_solve
    ("nv", E, x, p)                                        -> norm_violations
    ("kt", df, lam, mult_x_U, mult_x_L, jval)              -> kt_residuals
    ("phi", f_trial, E_trial, x_trial, mu, fr)             -> compute_phi
    ("qm", x, p, df, E, jval, hval, mu, with_step)         -> compute_qmodel
"""
from __future__ import annotations

import math
import types

import numpy as np

from host_mirror import (SqpTR, Model, Parameters, Context, default_options, _f, _OK, _INFEAS, _isapprox,  # noqa: F401
                         MODE_QP, MODE_FR, MODE_SOC, MODE_LP)


def make_context(model: Model, batch: int, **options) -> Context:
    """The context SqpTR.__init__ creates for `model`, with `batch` instances."""
    par = model.parameters
    opts = default_options(tol_direction=par.tol_direction, tol_residual=par.tol_residual, tol_infeas=par.tol_infeas,
                           max_iter=par.max_iter, init_mu=par.init_mu, tr_size=par.tr_size, use_soc=int(par.use_soc),
                           **options)
    jr = [r for r, _ in model.j_str]; jc = [c for _, c in model.j_str]
    hr = [r for r, _ in model.h_str]; hc = [c for _, c in model.h_str]
    return Context(model.n, model.m, model.num_linear_constraints, jr, jc, hr, hc, model.x_L, model.x_U, model.g_L,
                   model.g_U, opts, batch=batch)


class SqpTRLockstep(SqpTR):
    """SqpTR whose numerical steps are requests to a driver; `inst` is its instance of the shared context."""

    def __init__(self, problem: Model, ctx: Context, inst: int):
        pr = problem
        self.problem = pr
        n, m = pr.n, pr.m
        self.x = pr.x.copy()
        self.p = np.zeros(n); self.p_soc = np.zeros(n)
        self.lam = np.zeros(m); self.mult_x_L = np.zeros(n); self.mult_x_U = np.zeros(n)
        self.df = np.zeros(n); self.E = np.zeros(m)
        self.dE = np.zeros(len(pr.j_str)); self.h_val = np.zeros(len(pr.h_str))
        self.f = 0.0
        self.phi = 1e20; self.mu = 1e4; self.Delta = 10.0; self.Delta_max = 1e8
        self.step_acceptance = True
        self.prim_infeas = math.inf; self.dual_infeas = math.inf
        self.feasibility_restoration = False
        self.iter = 1; self.ret = -5
        self.sub_status = None
        self.trace = []
        self.ctx, self.inst = ctx, inst
        self.optimizer = None

    def _hval(self):
        return self.h_val if self.problem.eval_h is not None else None

    def _phi_request(self, x, alpha, p):     # compute_phi, sqp.jl:170-183
        pr = self.problem
        tmpx = x + alpha * p
        f, tmpE = self.f, self.E
        if alpha > 0.0:
            f = pr.eval_f(tmpx)
            tmpE = _f(pr.eval_g(tmpx))
        return ("phi", f, tmpE, tmpx, self.mu, self.feasibility_restoration)

    def _qm_request(self, p, with_step):     # compute_qmodel, sqp_trust_region.jl:487-508
        return ("qm", self.x, p, self.df, self.E, self.dE, self._hval(), self.mu, with_step)

    def steps(self):
        pr, par, ctx = self.problem, self.problem.parameters, self.ctx
        self.mu = par.init_mu
        self.Delta = par.tr_size
        self.f = pr.eval_f(self.x)
        if not math.isnan(self.f):
            self.E = _f(pr.eval_g(self.x))
        lpviol = 0.0
        for i in range(pr.num_linear_constraints):
            lpviol += max(0.0, pr.g_L[i] - self.E[i]) - min(0.0, pr.g_U[i] - self.E[i])
        lpviol += float(np.maximum(0.0, pr.x_L - self.x).sum() - np.minimum(0.0, pr.x_U - self.x).sum())
        if math.isnan(self.f):
            pr.status = -13
            return
        if lpviol > par.tol_infeas:
            self.df = _f(pr.eval_grad_f(self.x))
            self.dE = _f(pr.eval_jac_g(self.x))
            r = yield ("qp", MODE_LP, self.x, math.inf, 1.0, self.df, self.E, self.dE, self._hval())
            dz = lambda v: np.where(np.abs(v) < 1e-10, 0.0, v)
            self.x, self.lam, self.mult_x_U, self.mult_x_L = dz(r["p"]), dz(r["lam"]), dz(r["mult_x_U"]), dz(r["mult_x_L"])
            self.sub_status = r["status"]
            self._push_trace()
        while True:
            if self.iter > par.max_iter:
                self.ret = 6 if self.prim_infeas <= par.tol_infeas else -1
                break
            if self.step_acceptance:
                self.eval_functions()
                self.prim_infeas = yield ("nv", self.E, self.x, 1)
                self.dual_infeas = yield ("kt", self.df, self.lam, self.mult_x_U, self.mult_x_L, self.dE)
            mode = MODE_FR if self.feasibility_restoration else MODE_QP
            r = yield ("qp", mode, self.x, self.Delta, 1.0, self.df, self.E, self.dE, self._hval())
            self.p, lam, mu_u, mu_l, self.sub_status = r["p"], r["lam"], r["mult_x_U"], r["mult_x_L"], r["status"]
            p_lambda = lam - self.lam
            p_mult_x_L = mu_l - self.mult_x_L
            p_mult_x_U = mu_u - self.mult_x_U
            self.mu = max(self.mu, np.abs(self.lam).max(initial=0.0), np.abs(self.mult_x_L).max(initial=0.0),
                          np.abs(self.mult_x_U).max(initial=0.0))
            pn = float(np.abs(self.p).max(initial=0.0))
            if self.sub_status in _OK:
                if self.Delta == self.Delta_max and _isapprox(pn, self.Delta):
                    self.ret = 4
                    break
            elif self.sub_status in _INFEAS:
                if self.feasibility_restoration:
                    self.ret = 6 if self.prim_infeas <= par.tol_infeas else 2
                    break
                self.feasibility_restoration = True
                self._push_trace()
                self.iter += 1
                continue
            else:
                if self.prim_infeas <= par.tol_infeas * 10.0:
                    self.ret = 6
                break
            if self.step_acceptance:
                self.phi = yield self._phi_request(self.x, 0.0, self.p)
            self._push_trace()
            if pn <= par.tol_direction:
                if self.feasibility_restoration:
                    self.feasibility_restoration = False
                    self.iter += 1
                    continue
                self.ret = 0
                break
            if (self.prim_infeas <= par.tol_infeas and self.dual_infeas <= par.tol_residual
                    and not _isapprox(self.Delta, pn) and not self.feasibility_restoration):
                self.ret = 0
                break
            phi_k = yield self._phi_request(self.x, 1.0, self.p)
            ared = self.phi - phi_k
            pred, q_0 = 1.0, 0.0
            if not self.feasibility_restoration:
                q_0 = yield self._qm_request(self.p, False)
                pred = q_0 - (yield self._qm_request(self.p, True))
            accept, new_delta = ctx.tr_update(ared, pred, self.Delta, pn, self.Delta_max)     # host arithmetic only
            if accept:
                self.x = self.x + self.p
                self.lam = self.lam + p_lambda
                self.mult_x_L = self.mult_x_L + p_mult_x_L
                self.mult_x_U = self.mult_x_U + p_mult_x_U
                self.Delta = new_delta
                self.step_acceptance = True
            else:
                perform_soc = False
                tmpx = self.x + self.p
                c_k = yield ("nv", _f(pr.eval_g(tmpx)), tmpx, 1)
                if par.use_soc and c_k > 0 and not self.feasibility_restoration:
                    jp = self._jac_times(self.p)
                    e_soc = _f(pr.eval_g(tmpx)) - jp
                    r = yield ("qp", MODE_SOC, self.x, self.Delta, self.mu, self.df, e_soc, self.dE, self._hval())
                    self.p_soc = self.p + r["p"]
                    phi_soc = yield self._phi_request(self.x, 1.0, self.p_soc)
                    ared = self.phi - phi_soc
                    pred = q_0 - (yield self._qm_request(self.p_soc, True))
                    if ared > 0 and ared / pred > 0:
                        self.x = self.x + self.p_soc
                        self.lam = self.lam + p_lambda
                        self.mult_x_L = self.mult_x_L + p_mult_x_L
                        self.mult_x_U = self.mult_x_U + p_mult_x_U
                        self.step_acceptance = True
                        perform_soc = True
                if not perform_soc:
                    self.Delta = new_delta
                    self.step_acceptance = False
            if self.feasibility_restoration and self.step_acceptance:
                self.feasibility_restoration = False
            self.iter += 1
        pr.obj_val = pr.eval_f(self.x)
        pr.status = int(self.ret)
        pr.x[:] = self.x
        pr.g[:] = self.E
        pr.mult_g[:] = -self.lam
        pr.mult_x_U[:] = -self.mult_x_U
        pr.mult_x_L[:] = self.mult_x_L
        pr.statistics["iter"] = self.iter

    def run(self):
        raise RuntimeError("a lockstep model is driven by run_lockstep()")


def _key(req):
    """requests that can share a batch call: same entry point, same per-call flags, Hessian given or not"""
    kind = req[0]
    if kind == "qp":
        return (kind, req[8] is None)
    if kind == "nv":
        return (kind, req[3])
    if kind == "phi":
        return (kind, bool(req[5]))
    if kind == "qm":
        return (kind, bool(req[8]), req[6] is None)
    return (kind,)


def _issue(ctx: Context, key, insts, reqs):
    col = lambda j: [r[j] for r in reqs]
    kind = key[0]
    if kind == "qp":
        return ctx.qp_solve_batch(insts, col(1), col(2), col(3), col(4), col(5), col(6), col(7), None if key[1] else col(8))
    if kind == "nv":
        return ctx.norm_violations_batch(insts, col(1), col(2), key[1])
    if kind == "kt":
        return ctx.kt_residuals_batch(insts, col(1), col(2), col(3), col(4), col(5))
    if kind == "phi":
        return ctx.compute_phi_batch(insts, col(1), col(2), col(3), col(4), key[1])
    if kind == "qm":
        return ctx.compute_qmodel_batch(insts, col(1), col(2), col(3), col(4), col(5), None if key[2] else col(6), col(7), key[1])
    raise ValueError(kind)


def run_lockstep(models, ctx: Context | None = None, **options):
    """Run every model of `models` (same dimensions and sparsity) to termination, model k on instance k of one context.
    Returns (list of SqpTRLockstep, calls) with calls = {request kind: batch calls issued}."""
    if ctx is None:
        ctx = make_context(models[0], len(models), **options)
    if len(models) > ctx.batch:
        raise ValueError("more models than instances")
    sqps = []
    for k, mdl in enumerate(models):
        ctx.set_bounds(k, types.SimpleNamespace(xL=mdl.x_L, xU=mdl.x_U, gL=mdl.g_L, gU=mdl.g_U))
        sqps.append(SqpTRLockstep(mdl, ctx, k))
    gens = [s.steps() for s in sqps]
    pending, calls = {}, {}
    for k, g in enumerate(gens):
        try:
            pending[k] = next(g)
        except StopIteration:
            pass
    while pending:
        groups = {}
        for k in sorted(pending):
            groups.setdefault(_key(pending[k]), []).append(k)
        results = {}
        for key, ks in groups.items():
            out = _issue(ctx, key, ks, [pending[k] for k in ks])
            calls[key[0]] = calls.get(key[0], 0) + 1
            for j, k in enumerate(ks):
                results[k] = out[j] if key[0] == "qp" else float(out[j])
        nxt = {}
        for k in sorted(pending):
            try:
                nxt[k] = gens[k].send(results[k])
            except StopIteration:
                pass
        pending = nxt
    return sqps, calls
