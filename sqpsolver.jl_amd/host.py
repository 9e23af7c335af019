"""Host-side binding of the libsqphip C ABI with the reference's operator interface for the replaced path.

The reference host is Julia (`SqpSolver.Optimizer` -> `Model` -> `SqpTR.run!`); it stays Julia and reaches the
library through the `ccall` shim of julia/SqpHip.jl.  No Julia toolchain exists in this image, so
the same thin layer is written here in Python over ctypes with the reference's names, argument meaning and error
behaviour:

    Context         one sqphip_ctx: every entry point of include/sqphip.h (the *_batch methods: many host models on the
                    instances of one context, one call per round)
    QpData          /root/reference/src/algorithms/subproblem.jl:12-23
    QpHip           the `AbstractSubOptimizer` seat (subproblem.jl:1), API of QpJuMP:
                    sub_optimize / sub_optimize_FR / sub_optimize_lp / sub_optimize_L1QP /
                    sub_optimize_infeas  (subproblem_JuMP.jl:127-183, :352-393, :185-244, :283-347, :398-429)

The stand-in for the Julia HOST itself (`Model`, `Parameters`, `SqpTR.run!`: a transliteration of
sqp_trust_region.jl:98-223 that calls the seat) is test harness, not product, and lives in tests/host_mirror.py.

Nothing here computes on the CPU beyond control flow; if libsqphip.so is missing every entry point
raises.  The oracle under oracle/ is never imported from this package.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import numpy as np

from . import _lib

MODE_QP, MODE_FR, MODE_SOC, MODE_LP, MODE_L1QP, MODE_INFEAS = range(6)
# MOI.TerminationStatusCode integers
LOCALLY_SOLVED, LOCALLY_INFEASIBLE, ITERATION_LIMIT, NUMERICAL_ERROR = 4, 5, 11, 20
_OK = (1, 7, 10, 4)          # OPTIMAL, ALMOST_OPTIMAL, ALMOST_LOCALLY_SOLVED, LOCALLY_SOLVED
_INFEAS = (2, 5)             # INFEASIBLE, LOCALLY_INFEASIBLE

_dp = C.POINTER(C.c_double)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _f(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _l(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class SqpHipError(RuntimeError):
    pass


def default_options(**kw) -> _lib.Options:
    o = _lib.Options()
    _lib.lib().sqphip_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise KeyError(k)
        setattr(o, k, v)
    return o


def kkt_order(n, m, jrow, jcol, hrow, hcol, gL, gU, rows_last=True):
    """(pos, n_lead_tiles, order) of `sqphip_kkt_order`: host-only, works without a GPU."""
    L = _lib.lib()
    jr, jc, hr, hc = (np.ascontiguousarray(a, dtype=np.int64) for a in (jrow, jcol, hrow, hcol))
    # rows that stay in the condensed matrix: the equalities and rows with more than 32 entries (csrc/sparse.hpp)
    mk = int(np.sum((np.asarray(gL) == np.asarray(gU)) | (np.bincount(jr - 1, minlength=m) > 32)))
    pos = np.zeros(n + mk, dtype=np.int32); ts = C.c_int32(); nf = C.c_int32()
    rc = L.sqphip_kkt_order(n, m, len(jr), jr.ctypes.data_as(C.POINTER(C.c_int64)), jc.ctypes.data_as(C.POINTER(C.c_int64)),
                            len(hr), hr.ctypes.data_as(C.POINTER(C.c_int64)), hc.ctypes.data_as(C.POINTER(C.c_int64)),
                            _d(_f(gL)), _d(_f(gU)), int(rows_last), pos.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ts), C.byref(nf))
    if rc != 0:
        raise SqpHipError(f"sqphip_kkt_order failed ({rc})")
    return pos, ts.value, nf.value


def kkt_order_info(n, m, jrow, jcol, hrow, hcol, gL, gU, condense=1, tile_order=1):
    """What `sqphip_create` sets up for the dense path (`sqphip_kkt_order_info`, host only): a dict with pos [nu], nu, Ts,
    Tr, Nf, Fpad, masks (whether the kernels get the coupling mask), tmask [Tr, max(Ts, 1)], pair_ptr, pair_k."""
    L = _lib.lib()
    jr, jc, hr, hc = (np.ascontiguousarray(a, dtype=np.int64) for a in (jrow, jcol, hrow, hcol))
    pos = np.zeros(n + m, dtype=np.int32); info = np.zeros(6, dtype=np.int32); nk = C.c_int32()
    args = (n, m, len(jr), _l(jr), _l(jc), len(hr), _l(hr), _l(hc), _d(_f(gL)), _d(_f(gU)), int(condense), int(tile_order))
    rc = L.sqphip_kkt_order_info(*args, _i(pos), _i(info), None, 0, None, 0, None, 0, C.byref(nk))
    if rc != 0:
        raise SqpHipError(f"sqphip_kkt_order_info failed ({rc})")
    nu, Ts, Tr = (int(x) for x in info[:3])
    tmask = np.zeros((Tr, max(Ts, 1)), dtype=np.uint8); pptr = np.zeros(Tr * (Tr + 1) // 2 + 1, dtype=np.int32)
    pk = np.zeros(max(1, nk.value), dtype=np.int32)
    rc = L.sqphip_kkt_order_info(*args, _i(pos), _i(info), tmask.ctypes.data_as(C.POINTER(C.c_uint8)), tmask.size, _i(pptr),
                                 pptr.size, _i(pk), pk.size, C.byref(nk))
    if rc != 0:
        raise SqpHipError(f"sqphip_kkt_order_info failed ({rc})")
    return {"pos": pos[:nu].copy(), "nu": nu, "Ts": Ts, "Tr": Tr, "Nf": int(info[3]), "Fpad": int(info[4]),
            "masks": bool(info[5]), "tmask": tmask, "pair_ptr": pptr, "pair_k": pk[:nk.value].copy()}


def kkt_symbolic(n, m, jrow, jcol, hrow, hcol, gL, gU, condense=True, rows_after_vars=True, small_front=0,
                 zero_frac=-1.0):
    """(pos, stats dict) of `sqphip_kkt_symbolic`: the symbolic analysis of the sparse Newton matrix; host-only."""
    L = _lib.lib()
    jr, jc, hr, hc = (np.ascontiguousarray(a, dtype=np.int64) for a in (jrow, jcol, hrow, hcol))
    pos = np.zeros(n + m, dtype=np.int32); st = _lib.SymbolicStats()
    rc = L.sqphip_kkt_symbolic(n, m, len(jr), _l(jr), _l(jc), len(hr), _l(hr), _l(hc), _d(_f(gL)), _d(_f(gU)),
                               int(condense), int(rows_after_vars), int(small_front), float(zero_frac), _i(pos), C.byref(st))
    if rc != 0:
        raise SqpHipError(f"sqphip_kkt_symbolic failed ({rc})")
    out = {k: getattr(st, k) for k, _ in _lib.SymbolicStats._fields_}
    return pos[:out["order"]], out


def mf_host_solve(n, m, jrow, jcol, hrow, hcol, gL, gU, condense, jval, hval, Dd, sigp, hd, rtype, hsc, dw, rhs):
    """Host reference of the multifrontal numeric phase (`sqphip_mf_host_solve`): (sol, dinv_by_unknown, npos)."""
    L = _lib.lib()
    jr, jc, hr, hc = (np.ascontiguousarray(a, dtype=np.int64) for a in (jrow, jcol, hrow, hcol))
    rhs = _f(rhs); sol = np.zeros_like(rhs); dinv = np.zeros_like(rhs); npos = C.c_int32()
    rt = np.ascontiguousarray(rtype, dtype=np.int32)
    rc = L.sqphip_mf_host_solve(n, m, len(jr), _l(jr), _l(jc), len(hr), _l(hr), _l(hc), _d(_f(gL)), _d(_f(gU)),
                                int(condense), _d(_f(jval)), _d(_f(hval)), _d(_f(Dd)), _d(_f(sigp)), _d(_f(hd)), _i(rt),
                                float(hsc), float(dw), _d(rhs), _d(sol), _d(dinv), C.byref(npos))
    if rc != 0:
        raise SqpHipError(f"sqphip_mf_host_solve failed ({rc})")
    return sol, dinv, npos.value


def mf_host_top2_err() -> float:
    """After `mf_host_solve`: relative error of the host replay of the streamed top-of-tree solve from its own plan arrays
    against the plain recursion of that call (-1: the plan has no such top)."""
    return float(_lib.lib().sqphip_mf_host_top2_err())


def mf_host_spine_err() -> float:
    """After `mf_host_solve`: relative error of the host replay of the spine kernel's front assembly (k_mf_spine) from its own
    plan arrays against the images of the plain recursion (-1: the plan has no spine)."""
    return float(_lib.lib().sqphip_mf_host_spine_err())


def mf_plan_info(n, m, jrow, jcol, hrow, hcol, gL, gU, condense=1, batch=1):
    """Shape of the multifrontal plan `sqphip_create` builds (`sqphip_mf_plan_info`, host only): fronts (columns, rows, level)
    as an (ns, 3) array, factor launches (level, tiles of the kernel, fronts, tiles of the smallest front) as an (nl, 4)
    array, LDS bytes of the streamed top-of-tree
    solve (0: none), fronts of the spine kernel (0: none)."""
    L = _lib.lib()
    jr, jc, hr, hc = (np.ascontiguousarray(a, dtype=np.int64) for a in (jrow, jcol, hrow, hcol))
    nf, nl, top, sp = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
    args = (n, m, len(jr), _l(jr), _l(jc), len(hr), _l(hr), _l(hc), _d(_f(gL)), _d(_f(gU)), int(condense), int(batch))
    if L.sqphip_mf_plan_info(*args, None, 0, C.byref(nf), None, 0, C.byref(nl), C.byref(top), C.byref(sp)) != 0:
        raise SqpHipError("sqphip_mf_plan_info failed")
    fr = np.zeros((nf.value, 3), dtype=np.int32); la = np.zeros((nl.value, 4), dtype=np.int32)
    if L.sqphip_mf_plan_info(*args, _i(fr), nf.value, C.byref(nf), _i(la), nl.value, C.byref(nl), C.byref(top), C.byref(sp)) != 0:
        raise SqpHipError("sqphip_mf_plan_info failed")
    return fr, la, top.value, sp.value


def mf_front_launches(n, m, jrow, jcol, hrow, hcol, gL, gU, condense=1, batch=1):
    """Where the deferral pass of the plan put its fronts (`sqphip_mf_front_launches`, host only): an (ns, 3) array of (factor
    launch the front runs in, its launch in the schedule before the pass -- the rows of `mf_plan_info` under
    SQPHIP_MF_DEFER=0 --, parent front or -1 for a root)."""
    L = _lib.lib()
    jr, jc, hr, hc = (np.ascontiguousarray(a, dtype=np.int64) for a in (jrow, jcol, hrow, hcol))
    nf = C.c_int32()
    args = (n, m, len(jr), _l(jr), _l(jc), len(hr), _l(hr), _l(hc), _d(_f(gL)), _d(_f(gU)), int(condense), int(batch))
    if L.sqphip_mf_front_launches(*args, None, 0, C.byref(nf)) != 0:
        raise SqpHipError("sqphip_mf_front_launches failed")
    fr = np.zeros((nf.value, 3), dtype=np.int32)
    if L.sqphip_mf_front_launches(*args, _i(fr), nf.value, C.byref(nf)) != 0:
        raise SqpHipError("sqphip_mf_front_launches failed")
    return fr


def mf_factor_kernels(n, m, jrow, jcol, hrow, hcol, gL, gU, condense=1, batch=1, big_lds=1):
    """What the factorisation launches for the plan of `mf_plan_info` under the current environment
    (`sqphip_mf_factor_kernels`, host only): an (nl, 4) array, one row per factor launch, of (index of the chosen front kernel
    in the census of `Context.mf_census`, packed LDS image, the spine kernel takes the launch instead, the launch held at most
    eight fronts before the deferral pass)."""
    L = _lib.lib()
    jr, jc, hr, hc = (np.ascontiguousarray(a, dtype=np.int64) for a in (jrow, jcol, hrow, hcol))
    nl = C.c_int32()
    args = (n, m, len(jr), _l(jr), _l(jc), len(hr), _l(hr), _l(hc), _d(_f(gL)), _d(_f(gU)), int(condense), int(batch), int(big_lds))
    if L.sqphip_mf_factor_kernels(*args, None, 0, C.byref(nl)) != 0:
        raise SqpHipError("sqphip_mf_factor_kernels failed")
    ker = np.zeros((nl.value, 4), dtype=np.int32)
    if L.sqphip_mf_factor_kernels(*args, _i(ker), nl.value, C.byref(nl)) != 0:
        raise SqpHipError("sqphip_mf_factor_kernels failed")
    return ker


def mf_values_blocks(n, m, jrow, jcol, hrow, hcol, gL, gU, condense=1, values=None):
    """Blocks of the item-parallel values kernel (`sqphip_mf_values_blocks`, host only): a dict with blocks ((nb, 4): first
    destination, first item, destinations, items; nb = 0: the plan keeps the one-thread-per-destination kernel) and item_ptr;
    with values = (jval, hval, Dd, sigp, hd, rtype, hsc, dw) also vals_list and vals_block, the two host replays (vals_block
    is None when there are no blocks)."""
    L = _lib.lib()
    jr, jc, hr, hc = (np.ascontiguousarray(a, dtype=np.int64) for a in (jrow, jcol, hrow, hcol))
    nb, nd, ni = C.c_int32(), C.c_int64(), C.c_int64()
    head = (n, m, len(jr), _l(jr), _l(jc), len(hr), _l(hr), _l(hc), _d(_f(gL)), _d(_f(gU)), int(condense))
    none = (None, None, None, None, None, None, 0.0, 0.0)
    if L.sqphip_mf_values_blocks(*head, *none, None, 0, C.byref(nb), None, 0, C.byref(nd), C.byref(ni), None, None) != 0:
        raise SqpHipError("sqphip_mf_values_blocks failed")
    blocks = np.zeros((nb.value, 4), dtype=np.int32); ptr = np.zeros(nd.value + 1, dtype=np.int32)
    out = {"blocks": blocks, "item_ptr": ptr, "n_items": ni.value, "vals_list": None, "vals_block": None}
    vals = none; vl = vb = None
    if values is not None:
        jval, hval, Dd, sigp, hd, rtype, hsc, dw = values
        rt = np.ascontiguousarray(rtype, dtype=np.int32)
        vals = (_d(_f(jval)), _d(_f(hval)), _d(_f(Dd)), _d(_f(sigp)), _d(_f(hd)), _i(rt), float(hsc), float(dw))
        vl = np.zeros(nd.value); vb = np.zeros(nd.value)
    if L.sqphip_mf_values_blocks(*head, *vals, _i(blocks) if nb.value else None, nb.value, C.byref(nb), _i(ptr), nd.value,
                                 C.byref(nd), C.byref(ni), _d(vl) if vl is not None else None,
                                 _d(vb) if vb is not None else None) != 0:
        raise SqpHipError("sqphip_mf_values_blocks failed")
    if values is not None:
        out["vals_list"] = vl; out["vals_block"] = vb if nb.value else None
    return out


class Context:
    """Owns a sqphip_ctx (one NLP structure, `batch` instances)."""

    def __init__(self, n, m, num_linear, jrow, jcol, hrow, hcol, xL, xU, gL, gU,
                 options: _lib.Options | None = None, batch: int = 1):
        self.L = _lib.lib()
        self.n, self.m, self.batch = int(n), int(m), int(batch)
        self.nnzj, self.nnzh = len(jrow), len(hrow)
        self.opts = options or default_options()
        jr, jc, hr, hc = (np.ascontiguousarray(a, dtype=np.int64) for a in (jrow, jcol, hrow, hcol))
        h = C.c_void_p()
        rc = self.L.sqphip_create(C.byref(h), n, m, num_linear, len(jr), _l(jr), _l(jc), len(hr), _l(hr),
                                  _l(hc), _d(_f(xL)), _d(_f(xU)), _d(_f(gL)), _d(_f(gU)),
                                  C.byref(self.opts), batch)
        if rc != 0:
            raise SqpHipError(f"sqphip_create failed with code {rc}")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.sqphip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            msg = self.L.sqphip_last_error(self.h)
            raise SqpHipError(f"libsqphip error {rc}: {msg.decode() if msg else ''}")

    # ---- sub-problem seat
    def qp_solve(self, mode, x_k, delta, mu, df, E, jval, hval):
        p = np.zeros(self.n); lam = np.zeros(self.m)
        mu_u = np.zeros(self.n); mu_l = np.zeros(self.n); slack = np.zeros(2 * self.m)
        st = C.c_int32()
        self._ck(self.L.sqphip_qp_solve(self.h, mode, _d(_f(x_k)), float(delta), float(mu), _d(_f(df)),
                                        _d(_f(E)), _d(_f(jval)),
                                        _d(_f(hval)) if hval is not None and len(hval) else None,
                                        _d(p), _d(lam), _d(mu_u), _d(mu_l), _d(slack), C.byref(st)))
        it, nf = C.c_int32(), C.c_int32()
        self.L.sqphip_qp_stats(self.h, C.byref(it), C.byref(nf))
        rule, err = C.c_int32(), C.c_double()
        self.L.sqphip_qp_termination(self.h, C.byref(rule), C.byref(err))
        return dict(p=p, lam=lam, mult_x_U=mu_u, mult_x_L=mu_l, slack=slack, status=st.value,
                    ipm_iters=it.value, n_factor=nf.value, term_rule=rule.value, scaled_error=err.value)

    # ---- the seat for many host models at once (sqphip_*_batch): request k runs on instance inst[k]
    def _insts(self, inst):
        a = np.ascontiguousarray(inst, dtype=np.int32)
        if a.ndim != 1 or len(a) == 0:
            raise ValueError("inst must be a non-empty list of instance numbers")
        return a

    @staticmethod
    def _rows(name, rows, count, width):
        """[count][width] float64, contiguous, from a sequence of `count` vectors; None stays None.  Ragged or mis-sized
        input is refused here, before the library sees a pointer."""
        if rows is None:
            return None
        rows = list(rows) if not isinstance(rows, np.ndarray) else rows
        if len(rows) != count:
            raise ValueError(f"{name}: {len(rows)} rows for {count} requests")
        for k, r in enumerate(rows):
            if r is None or np.ndim(r) != 1 or len(r) != width:
                raise ValueError(f"{name}[{k}]: expected a vector of length {width}")
        return np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(count, width))

    @staticmethod
    def _scalars(name, v, count):
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (count,)) if np.ndim(v) == 0 else v,
                                 dtype=np.float64)
        if a.shape != (count,):
            raise ValueError(f"{name}: expected {count} values")
        return a

    def qp_solve_batch(self, inst, mode, x_k, delta, mu, df, E, jval, hval):
        """`sqphip_qp_solve_batch`: one call for len(inst) sub-problems; returns the dicts of qp_solve in request order."""
        ins = self._insts(inst); cnt = len(ins)
        md = np.ascontiguousarray(mode, dtype=np.int32)
        if md.shape != (cnt,):
            raise ValueError(f"mode: expected {cnt} values")
        dl, pen = self._scalars("delta", delta, cnt), self._scalars("mu", mu, cnt)
        xk = self._rows("x_k", x_k, cnt, self.n); c = self._rows("df", df, cnt, self.n); b = self._rows("E", E, cnt, self.m)
        jv = self._rows("jval", jval, cnt, self.nnzj)
        hv = self._rows("hval", hval, cnt, self.nnzh) if hval is not None and self.nnzh and all(h is not None for h in hval) else None
        if hval is not None and self.nnzh and hv is None and any(h is not None for h in hval):
            raise ValueError("hval: given for some requests only")
        p = np.zeros((cnt, self.n)); lam = np.zeros((cnt, self.m)); mu_u = np.zeros((cnt, self.n)); mu_l = np.zeros((cnt, self.n))
        slack = np.zeros((cnt, 2 * self.m)); st = np.zeros(cnt, dtype=np.int32)
        self._ck(self.L.sqphip_qp_solve_batch(self.h, cnt, _i(ins), _i(md), _d(xk), _d(dl), _d(pen), _d(c), _d(b), _d(jv), _d(hv),
                                              _d(p), _d(lam), _d(mu_u), _d(mu_l), _d(slack), _i(st)))
        stats = self.qp_stats_batch(ins)
        return [dict(p=p[k].copy(), lam=lam[k].copy(), mult_x_U=mu_u[k].copy(), mult_x_L=mu_l[k].copy(), slack=slack[k].copy(),
                     status=int(st[k]), **stats[k]) for k in range(cnt)]

    def qp_stats_batch(self, inst):
        """`sqphip_qp_stats_batch`: per listed instance the ipm_iters, n_factor, term_rule, scaled_error of its last sub-problem."""
        ins = self._insts(inst); cnt = len(ins)
        it = np.zeros(cnt, dtype=np.int32); nf = np.zeros(cnt, dtype=np.int32); rule = np.zeros(cnt, dtype=np.int32); err = np.zeros(cnt)
        self._ck(self.L.sqphip_qp_stats_batch(self.h, cnt, _i(ins), _i(it), _i(nf), _i(rule), _d(err)))
        return [dict(ipm_iters=int(it[k]), n_factor=int(nf[k]), term_rule=int(rule[k]), scaled_error=float(err[k])) for k in range(cnt)]

    def seat_peek(self, inst):
        """Test hook `sqphip_seat_peek`: the seat's output slots of one instance as the device holds them."""
        p = np.zeros(self.n); lam = np.zeros(self.m); mu_u = np.zeros(self.n); mu_l = np.zeros(self.n); slack = np.zeros(2 * self.m)
        st = C.c_int32()
        self._ck(self.L.sqphip_seat_peek(self.h, int(inst), _d(p), _d(lam), _d(mu_u), _d(mu_l), _d(slack), C.byref(st)))
        return dict(p=p, lam=lam, mult_x_U=mu_u, mult_x_L=mu_l, slack=slack, status=st.value)

    _PN = {1: 1, 2: 2, math.inf: 0, "inf": 0}

    def norm_violations_batch(self, inst, E, x, p=1):
        ins = self._insts(inst); cnt = len(ins); out = np.zeros(cnt)
        self._ck(self.L.sqphip_norm_violations_batch(self.h, cnt, _i(ins), _d(self._rows("E", E, cnt, self.m)),
                                                     _d(self._rows("x", x, cnt, self.n)), self._PN[p], _d(out)))
        return out

    def kt_residuals_batch(self, inst, df, lam, mult_x_U, mult_x_L, jval):
        ins = self._insts(inst); cnt = len(ins); out = np.zeros(cnt)
        self._ck(self.L.sqphip_kt_residuals_batch(self.h, cnt, _i(ins), _d(self._rows("df", df, cnt, self.n)),
                                                  _d(self._rows("lam", lam, cnt, self.m)),
                                                  _d(self._rows("mult_x_U", mult_x_U, cnt, self.n)),
                                                  _d(self._rows("mult_x_L", mult_x_L, cnt, self.n)),
                                                  _d(self._rows("jval", jval, cnt, self.nnzj)), _d(out)))
        return out

    def norm_complementarity_batch(self, inst, E, lam, p=math.inf):
        ins = self._insts(inst); cnt = len(ins); out = np.zeros(cnt)
        self._ck(self.L.sqphip_norm_complementarity_batch(self.h, cnt, _i(ins), _d(self._rows("E", E, cnt, self.m)),
                                                          _d(self._rows("lam", lam, cnt, self.m)), self._PN[p], _d(out)))
        return out

    def compute_phi_batch(self, inst, f_trial, E_trial, x_trial, mu, fr):
        ins = self._insts(inst); cnt = len(ins); out = np.zeros(cnt)
        self._ck(self.L.sqphip_compute_phi_batch(self.h, cnt, _i(ins), _d(self._scalars("f_trial", f_trial, cnt)),
                                                 _d(self._rows("E_trial", E_trial, cnt, self.m)),
                                                 _d(self._rows("x_trial", x_trial, cnt, self.n)),
                                                 _d(self._scalars("mu", mu, cnt)), int(fr), _d(out)))
        return out

    def compute_qmodel_batch(self, inst, x, p, df, E, jval, hval, mu, with_step):
        ins = self._insts(inst); cnt = len(ins); out = np.zeros(cnt)
        hv = self._rows("hval", hval, cnt, self.nnzh) if hval is not None and self.nnzh and all(h is not None for h in hval) else None
        self._ck(self.L.sqphip_compute_qmodel_batch(self.h, cnt, _i(ins), _d(self._rows("x", x, cnt, self.n)),
                                                    _d(self._rows("p", p, cnt, self.n)), _d(self._rows("df", df, cnt, self.n)),
                                                    _d(self._rows("E", E, cnt, self.m)), _d(self._rows("jval", jval, cnt, self.nnzj)),
                                                    _d(hv), _d(self._scalars("mu", mu, cnt)), int(with_step), _d(out)))
        return out

    def compute_derivative_full_batch(self, inst, df, p, E, mu, mu_vec=None, feasibility_restoration=False, slack=None):
        ins = self._insts(inst); cnt = len(ins); out = np.zeros(cnt)
        self._ck(self.L.sqphip_compute_derivative_full_batch(
            self.h, cnt, _i(ins), _d(self._rows("df", df, cnt, self.n)), _d(self._rows("p", p, cnt, self.n)),
            _d(self._rows("E", E, cnt, self.m)), _d(self._scalars("mu", mu, cnt)), _d(self._rows("mu_vec", mu_vec, cnt, self.m)),
            int(feasibility_restoration), _d(self._rows("slack", slack, cnt, 2 * self.m)), _d(out)))
        return out

    def compute_derivative_full(self, df, p, E, mu, mu_vec=None, feasibility_restoration=False, slack=None):
        """compute_derivative(sqp) of sqp.jl:190-213 over merit.jl:13-17 (vector penalty, restoration branch)."""
        out = C.c_double()
        self._ck(self.L.sqphip_compute_derivative_full(self.h, _d(_f(df)), _d(_f(p)), _d(_f(E)), float(mu), _d(_f(mu_vec)),
                                                       int(feasibility_restoration), _d(_f(slack)), C.byref(out)))
        return out.value

    def compute_mu_rule(self, rule, it, rho, x, E, df, p, hval, lam, mu):
        """compute_mu_rule1! / 2! / 3! (sqp_line_search.jl:270-294) with the reductions on the device; returns mu."""
        mu = _f(mu).copy()
        self._ck(self.L.sqphip_compute_mu_rule_dev(self.h, int(rule), int(it), float(rho), _d(_f(x)), _d(_f(E)), _d(_f(df)),
                                                   _d(_f(p)), _d(_f(hval)) if hval is not None and len(hval) else None,
                                                   _d(_f(lam)), _d(mu)))
        return mu

    def acopf_armijo(self, inst, x, p, mu, phi0, D, eta=0.4, tau=0.9, min_alpha=1e-6, feasibility_restoration=False):
        """compute_alpha (sqp_line_search.jl:303-334) on the device: (alpha, is_valid, merit evaluations)."""
        al = C.c_double(); ok = C.c_int32(); ne = C.c_int32()
        self._ck(self.L.sqphip_acopf_armijo(self.h, inst, _d(_f(x)), _d(_f(p)), float(mu), float(phi0), float(D), float(eta),
                                            float(tau), float(min_alpha), int(feasibility_restoration), C.byref(al),
                                            C.byref(ok), C.byref(ne)))
        return al.value, bool(ok.value), ne.value

    def mf_solve_test(self, inst, jval, hval, Dd, sigp, hd, rtype, hsc, dw, rhs):
        """Kernel-level hook of the multifrontal path: (sol_fused, sol_standalone, dinv_by_unknown)."""
        rhs = _f(rhs); a = np.zeros_like(rhs); b = np.zeros_like(rhs); dv = np.zeros_like(rhs)
        rt = np.ascontiguousarray(rtype, dtype=np.int32)
        self._ck(self.L.sqphip_mf_solve_test(self.h, inst, _d(_f(jval)), _d(_f(hval)), _d(_f(Dd)), _d(_f(sigp)),
                                             _d(_f(hd)), _i(rt), float(hsc), float(dw), _d(rhs), _d(a), _d(b), _d(dv)))
        return a, b, dv

    def mf_batch_test(self, active, jval, hval, Dd, sigp, hd, rtype, hsc, dw, dw_last, fac_attempt, rhs):
        """Batched kernel-level hook of the multifrontal path (`sqphip_mf_batch_test`); per-instance inputs stacked as
        [B, ...].  Returns a dict: fused, standalone, dinv0, dinv1 ([B, nu]), decision ([B, 5]: outcome 0 idle / 1 another
        shift / 2 passed / 3 given up, sel, n_factor, fac_attempt, speculates: derived on the host from the inputs), dw ([B])."""
        rhs = _f(rhs); B = rhs.shape[0]
        out = {k: np.zeros_like(rhs) for k in ("fused", "standalone", "dinv0", "dinv1")}
        dec = np.zeros((B, 5), dtype=np.int32); dwo = np.zeros(B)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        act, rt, fa = i32(active), i32(rtype), i32(fac_attempt)
        self._ck(self.L.sqphip_mf_batch_test(self.h, _i(act), _d(_f(jval)), _d(_f(hval)), _d(_f(Dd)), _d(_f(sigp)), _d(_f(hd)),
                                             _i(rt), _d(_f(hsc)), _d(_f(dw)), _d(_f(dw_last)), _i(fa), _d(rhs),
                                             _d(out["fused"]), _d(out["standalone"]), _d(out["dinv0"]), _d(out["dinv1"]),
                                             _i(dec), _d(dwo)))
        out["decision"] = dec; out["dw"] = dwo
        return out

    def mf_values_test(self, active, jval, hval, Dd, sigp, hd, rtype, hsc, dw, dw_last, fac_attempt, sentinel=-7.5):
        """The values launch of a sweep on its own (`sqphip_mf_values_test`); inputs stacked as for `mf_batch_test`.  Returns
        (vals0, vals1), each [B, nnzK]: the assembled values of both candidate shifts, `sentinel` where nothing was written."""
        nk = C.c_int64()
        self._ck(self.L.sqphip_mf_values_test(self.h, *([None] * 11), 0.0, None, None, C.byref(nk)))
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        act, rt, fa = i32(active), i32(rtype), i32(fac_attempt)
        v0 = np.zeros((len(act), nk.value)); v1 = np.zeros_like(v0)
        self._ck(self.L.sqphip_mf_values_test(self.h, _i(act), _d(_f(jval)), _d(_f(hval)), _d(_f(Dd)), _d(_f(sigp)), _d(_f(hd)),
                                              _i(rt), _d(_f(hsc)), _d(_f(dw)), _d(_f(dw_last)), _i(fa), float(sentinel),
                                              _d(v0), _d(v1), C.byref(nk)))
        return v0, v1

    def kkt_dense_test(self, active, jval, hval, Dd, sigp, hd, rtype, hsc, dw, dw_last, fac_attempt, rhs, Fpad, nu,
                       sentinel=-7.5):
        """Kernel-level hook of the dense path (`sqphip_kkt_dense_test`); per-instance inputs stacked as [B, ...], rhs
        [B, n + m].  Fpad, nu: as `kkt_order_info` reports them for the context's structure and options.  Returns a dict:
        K [B, Fpad, Fpad] (K[b][r, c]: row r, column c of the matrix as assembled, factorised order), xv [B, Fpad],
        xv_mismatch (entries on which the two loaders of the working vector differ), sol / dinv [B, nu] (unknown order),
        dinv_pad [B, Fpad], decision [B, 4] (outcome 0 idle / 1 another shift / 2 passed / 3 given up, sel, n_factor,
        fac_attempt), dw [B]."""
        rhs = _f(rhs); B = rhs.shape[0]
        K = np.zeros((B, Fpad, Fpad)); xv = np.zeros((B, Fpad)); dpad = np.zeros((B, Fpad))
        sol = np.zeros((B, nu)); dinv = np.zeros((B, nu))
        dec = np.zeros((B, 4), dtype=np.int32); dwo = np.zeros(B); mis = C.c_int32(-1)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        act, rt, fa = i32(active), i32(rtype), i32(fac_attempt)
        self._ck(self.L.sqphip_kkt_dense_test(self.h, _i(act), _d(_f(jval)), _d(_f(hval)), _d(_f(Dd)), _d(_f(sigp)), _d(_f(hd)),
                                              _i(rt), _d(_f(hsc)), _d(_f(dw)), _d(_f(dw_last)), _i(fa), _d(rhs), float(sentinel),
                                              _d(K), _d(xv), C.byref(mis), _d(sol), _d(dinv), _d(dpad), _i(dec), _d(dwo)))
        # the device holds the matrix column-major: K[b][c, r] as read; hand out row-major views
        return {"K": K.transpose(0, 2, 1), "xv": xv, "xv_mismatch": int(mis.value), "sol": sol, "dinv": dinv,
                "dinv_pad": dpad, "decision": dec, "dw": dwo}

    SOLVE_VECTOR_SENTINEL = -7.5          # SQPHIP_SOLVE_VECTOR_SENTINEL (include/sqphip_test_hooks.h)

    def solve_vector_test(self, active, jval, Dd, rtype, rhs):
        """The working vector of the solves by both routines (`sqphip_solve_vector_test`), on a sparse or a dense context;
        per-instance inputs stacked as [B, ...], rhs [B, n + m].  Returns (xv_plain, xv_terms, mismatch): the vector by the
        column walk and by the entry-parallel terms, each [B, Fpad] (Fpad: the order of the factorised matrix padded to 64)
        with SOLVE_VECTOR_SENTINEL where nothing was written, and the number of entries whose bits differ.  Raises
        SqpHipError (state) where the context runs without the LDS stage."""
        rhs = _f(rhs); B = rhs.shape[0]
        Fpad = (self.counters()["kkt_order"] + 63) // 64 * 64
        xa = np.zeros((B, Fpad)); xb = np.zeros((B, Fpad)); mis = C.c_int32(-1)
        act = np.ascontiguousarray(active, dtype=np.int32); rt = np.ascontiguousarray(rtype, dtype=np.int32)
        self._ck(self.L.sqphip_solve_vector_test(self.h, _i(act), _d(_f(jval)), _d(_f(Dd)), _i(rt), _d(rhs), _d(xa), _d(xb),
                                                 C.byref(mis)))
        return xa, xb, int(mis.value)

    def mf_census(self):
        """Launch census of the multifrontal path (`sqphip_mf_census`): {kernel instantiation: launches enqueued}."""
        nk = C.c_int32()
        self._ck(self.L.sqphip_mf_census(self.h, None, None, 0, C.byref(nk)))
        cnt = np.zeros(nk.value, dtype=np.int64); names = C.create_string_buffer(64 * nk.value)
        self._ck(self.L.sqphip_mf_census(self.h, _l(cnt), names, nk.value, C.byref(nk)))
        return {names.raw[64 * k:64 * (k + 1)].split(b"\0")[0].decode(): int(cnt[k]) for k in range(nk.value)}

    def trans_inline_groups(self):
        """Sweeps, summed over the instance groups, that launched the three transition kernels in line
        (`sqphip_trans_inline_groups`); with the transitions riding in the post launch: the first sweep of every run only."""
        out = C.c_int64()
        self._ck(self.L.sqphip_trans_inline_groups(self.h, C.byref(out)))
        return int(out.value)

    # ---- merit path
    def norm_violations(self, E, x, p=1):
        out = C.c_double()
        pn = {1: 1, 2: 2, math.inf: 0, "inf": 0}[p]
        self._ck(self.L.sqphip_norm_violations(self.h, _d(_f(E)), _d(_f(x)), pn, C.byref(out)))
        return out.value

    def kt_residuals(self, df, lam, mult_x_U, mult_x_L, jval):
        out = C.c_double()
        self._ck(self.L.sqphip_kt_residuals(self.h, _d(_f(df)), _d(_f(lam)), _d(_f(mult_x_U)),
                                            _d(_f(mult_x_L)), _d(_f(jval)), C.byref(out)))
        return out.value

    def norm_complementarity(self, E, lam, p=math.inf):
        out = C.c_double()
        pn = {1: 1, 2: 2, math.inf: 0, "inf": 0}[p]
        self._ck(self.L.sqphip_norm_complementarity(self.h, _d(_f(E)), _d(_f(lam)), pn, C.byref(out)))
        return out.value

    def compute_phi(self, f_trial, E_trial, x_trial, mu, fr):
        out = C.c_double()
        self._ck(self.L.sqphip_compute_phi(self.h, float(f_trial), _d(_f(E_trial)), _d(_f(x_trial)),
                                           float(mu), int(fr), C.byref(out)))
        return out.value

    def compute_qmodel(self, x, p, df, E, jval, hval, mu, with_step):
        out = C.c_double()
        self._ck(self.L.sqphip_compute_qmodel(self.h, _d(_f(x)), _d(_f(p)), _d(_f(df)), _d(_f(E)),
                                              _d(_f(jval)),
                                              _d(_f(hval)) if hval is not None and len(hval) else None,
                                              float(mu), int(with_step), C.byref(out)))
        return out.value

    def compute_derivative(self, df, p, E, mu):
        out = C.c_double()
        self._ck(self.L.sqphip_compute_derivative(self.h, _d(_f(df)), _d(_f(p)), _d(_f(E)), float(mu),
                                                  C.byref(out)))
        return out.value

    def tr_update(self, ared, pred, delta, pnorm, delta_max=1e8):
        acc = C.c_int32(); dn = C.c_double()
        self._ck(self.L.sqphip_tr_update(float(ared), float(pred), float(delta), float(pnorm),
                                         float(delta_max), float(self.opts.tol_direction),
                                         C.byref(acc), C.byref(dn)))
        return bool(acc.value), dn.value

    # ---- ACOPF batch
    def acopf_attach(self, net, lay):
        keep = [np.ascontiguousarray(a, dtype=np.int32) for a in
                (net.f_bus, net.t_bus, net.gen_bus, lay.bal_ptr, lay.bal_colP, lay.bal_colQ)]
        coef = _f(lay.bal_coef)
        form = getattr(lay, "form", "polar")
        if form == "acwr":
            bp = [np.ascontiguousarray(a, dtype=np.int32) for a in (lay.bp_i, lay.bp_j, lay.br_bp)]
            self._ck(self.L.sqphip_acopf_attach_acwr(self.h, net.nb, net.ng, net.nl, *[_i(a) for a in keep], _d(coef),
                                                     int(net.ref_bus), len(bp[0]), *[_i(a) for a in bp], _d(_f(lay.br_sig)),
                                                     _d(_f(lay.bp_tmin)), _d(_f(lay.bp_tmax))))
        else:
            attach = self.L.sqphip_acopf_attach_acr if form == "acr" else self.L.sqphip_acopf_attach
            self._ck(attach(self.h, net.nb, net.ng, net.nl, *[_i(a) for a in keep], _d(coef), int(net.ref_bus)))
        if len(lay.dc_loss1):
            self._ck(self.L.sqphip_acopf_set_dclines(self.h, len(lay.dc_loss1), _d(_f(lay.dc_loss1))))
        if len(lay.sh_bus):
            sb = np.ascontiguousarray(lay.sh_bus, dtype=np.int32)
            self._ck(self.L.sqphip_acopf_set_shunts(self.h, len(sb), _i(sb), _d(_f(lay.sh_gs)), _d(_f(lay.sh_bs))))

    def set_bounds(self, inst, lay):
        """Per-instance variable / row bounds (anything with xL, xU, gL, gU attributes)."""
        self._ck(self.L.sqphip_set_bounds(self.h, inst, _d(_f(lay.xL)), _d(_f(lay.xU)), _d(_f(lay.gL)),
                                          _d(_f(lay.gU))))

    def acopf_set_instance(self, inst, net, lay, x0=None):
        ohm = _f(net.branch_coeffs().ravel())                 # [nl][12], row-major
        self._ck(self.L.sqphip_set_bounds(self.h, inst, _d(_f(lay.xL)), _d(_f(lay.xU)), _d(_f(lay.gL)),
                                          _d(_f(lay.gU))))
        self._ck(self.L.sqphip_acopf_set_instance(self.h, inst, _d(ohm), _d(_f(net.c2)),
                                                  _d(_f(net.c1)), _d(_f(lay.x0 if x0 is None else x0))))

    # ---- the synthetic dense-Hessian NLP (dense_synth.py; csrc/acopf_dev.hpp dense_eval)
    def dense_attach(self, nlp):
        self._ck(self.L.sqphip_dense_attach(self.h, _d(_f(nlp.Q.ravel())), _d(_f(nlp.A.ravel())), float(nlp.kappa)))

    def dense_set_instance(self, inst, nlp, lay, x0=None):
        self._ck(self.L.sqphip_set_bounds(self.h, inst, _d(_f(lay.xL)), _d(_f(lay.xU)), _d(_f(lay.gL)), _d(_f(lay.gU))))
        self._ck(self.L.sqphip_dense_set_instance(self.h, inst, _d(_f(nlp.c)), _d(_f(lay.x0 if x0 is None else x0))))

    # ---- a general sparse QCQP (qcqp.py; csrc/qcqp_dev.hpp qcqp_eval)
    def qcqp_attach(self, q):
        """Structure of the batch and the values every instance starts with (sqphip_qcqp_attach)."""
        t = [np.ascontiguousarray(a, dtype=np.int64) for a in (q.q0r, q.q0c, q.ar, q.ac, q.qi, q.qr, q.qc)]
        v = [_f(a) for a in (q.q0v, q.av, q.qv, q.c, q.g0)]
        self._ck(self.L.sqphip_qcqp_attach(self.h, len(v[0]), _l(t[0]), _l(t[1]), _d(v[0]), len(v[1]), _l(t[2]), _l(t[3]),
                                           _d(v[1]), len(v[2]), _l(t[4]), _l(t[5]), _l(t[6]), _d(v[2]), _d(v[3]), _d(v[4]),
                                           float(q.f0)))

    def qcqp_set_instance(self, inst, q=None, x0=None, **values):
        """Per-instance values (sqphip_qcqp_set_instance).  With a Qcqp q: its bounds, every value and its start; keywords
        f0, c, q0v, g0, av, qv override single parts, and what is given neither way is kept."""
        if q is not None:
            self.set_bounds(inst, q)
            values = {**{k: getattr(q, k) for k in ("f0", "c", "q0v", "g0", "av", "qv")}, **values}
            x0 = q.x0 if x0 is None else x0
        bad = set(values) - {"f0", "c", "q0v", "g0", "av", "qv"}
        if bad:
            raise TypeError(f"qcqp_set_instance: unknown values {sorted(bad)}")
        arr = [None if values.get(k) is None else _f(np.atleast_1d(values[k])) for k in ("f0", "c", "q0v", "g0", "av", "qv")]
        self._ck(self.L.sqphip_qcqp_set_instance(self.h, inst, *[_d(a) for a in arr], _d(_f(x0))))

    # ---- a sparse factorable NLP (nlp_terms.py; csrc/nlp_dev.hpp nlp_eval)
    def nlp_add_block(self, b) -> int:
        """One dense data block of the objective (sqphip_nlp_add_block; b: nlp_terms.NlpBlock); before the first sqp_reset,
        sqp_run or nlp_stream_begin.  Returns its number.  An nlp_terms.NlpSoftmaxBlock goes through
        sqphip_nlp_add_softmax_block, an nlp_terms.NlpRowBlock (several outputs, constraint rows) through
        sqphip_nlp_add_row_block, an nlp_terms.NlpCoxBlock through sqphip_nlp_add_cox_block, an nlp_terms.NlpLseBlock
        (log-sum-exp rows) through sqphip_nlp_add_lse_block, an nlp_terms.NlpNormBlock (Euclidean norms) through
        sqphip_nlp_add_norm_block."""
        from .nlp_terms import NlpCoxBlock, NlpLseBlock, NlpNormBlock, NlpRowBlock, NlpSoftmaxBlock
        def i32(a):
            return _i(np.ascontiguousarray(a, dtype=np.int32))

        def i64(a):
            return _l(np.ascontiguousarray(a, dtype=np.int64).ravel())

        # the arguments of a call between the handle and shift, weight, the block number (N, d; cols, A: pointers)
        def scalar(N, d, cols, A):
            return (int(b.kind), int(b.exp), float(b.par), N, d, cols, A)

        def rows(N, d, cols, A):
            r = np.ascontiguousarray(b.rows, dtype=np.int64)
            return scalar(N, d, cols, A) + (len(r), _l(r))

        def softmax(N, d, cols, A):
            return (N, d, int(b.K), int(bool(b.pinned)), cols, A, i32(b.labels))

        def cox(N, d, cols, A):
            return (N, d, cols, A, i32(b.risk), _d(_f(b.event)))

        def lse(N, d, cols, A):
            r = np.ascontiguousarray(b.rows, dtype=np.int64)
            return (N, d, cols, A, len(r), _l(r), i64(b.seg))

        symbol, args = "sqphip_nlp_add_block", scalar         # any other class
        # (a norm block has the argument list of a log-sum-exp block)
        for cls, sym, fn in ((NlpNormBlock, "sqphip_nlp_add_norm_block", lse), (NlpLseBlock, "sqphip_nlp_add_lse_block", lse), (NlpCoxBlock, "sqphip_nlp_add_cox_block", cox),
                             (NlpRowBlock, "sqphip_nlp_add_row_block", rows), (NlpSoftmaxBlock, "sqphip_nlp_add_softmax_block", softmax)):
            if isinstance(b, cls):
                symbol, args = sym, fn
                break
        if not hasattr(self.L, symbol):
            raise SqpHipError(f"libsqphip.so lacks {symbol}: rebuild it")
        A = _f(np.atleast_2d(b.A))
        out = C.c_int32(-1)
        self._ck(getattr(self.L, symbol)(self.h, *args(A.shape[0], A.shape[1], i64(b.cols), _d(A)),
                                         _d(None if b.shift is None else _f(b.shift).ravel()),
                                         _d(None if b.weight is None else _f(b.weight).ravel()), C.byref(out)))
        return out.value

    @staticmethod
    def _nlp_block_data(who, p, values):
        """[(block, weight or None, shift or None)] of p's blocks and of the keywords weight / shift, which override: an array
        for block 0, or a list or dict of arrays by block (None: keep).  The keywords leave `values`.  The weights of a block
        with R outputs are [R, N] and travel flattened."""
        per = {}
        for k, b in enumerate(getattr(p, "blocks", None) or []):
            per[k] = [b.weight, b.shift]
        for pos, key in enumerate(("weight", "shift")):
            v = values.pop(key, None)
            if v is None:
                continue
            if isinstance(v, dict):
                items = v.items()
            elif isinstance(v, (list, tuple)) and (len(v) == 0 or v[0] is None or np.ndim(v[0]) > 0):
                items = enumerate(v)              # (a [R, N] array is an ndarray, not a list: it is block 0's)
            else:
                items = [(0, v)]
            for k, a in items:
                if a is not None:
                    per.setdefault(int(k), [None, None])[pos] = a
        return [(k, None if w is None else _f(np.atleast_1d(w)).ravel(), None if s is None else _f(np.atleast_1d(s)).ravel())
                for k, (w, s) in sorted(per.items()) if w is not None or s is not None]

    def nlp_set_instance_block(self, inst, blk, weight=None, shift=None):
        """weight / shift of block blk of one instance (sqphip_nlp_set_instance_block); None: keep.  A block with R outputs
        takes [R, N] weights."""
        self._ck(self.L.sqphip_nlp_set_instance_block(self.h, int(inst), int(blk), _d(None if weight is None else _f(weight).ravel()),
                                                      _d(None if shift is None else _f(shift).ravel())))

    def nlp_stream_set_block(self, scen, blk, weight=None, shift=None):
        """weight / shift of block blk of one scenario of the queue (sqphip_nlp_stream_set_block), after nlp_stream_set."""
        self._ck(self.L.sqphip_nlp_stream_set_block(self.h, int(scen), int(blk), _d(None if weight is None else _f(weight).ravel()),
                                                    _d(None if shift is None else _f(shift).ravel())))

    def nlp_attach(self, p, general=None, instance_data=False):
        """Structure of the batch and the values every instance starts with; p: nlp_terms.NlpTerms.  A p with argument arrays
        (affine multi-variable factors) goes through sqphip_nlp_attach_affine, any other through sqphip_nlp_attach; a p
        made for more -- p.general, which make_nlp_terms sets for a variable shared by two factors of a term, a kind above
        LOG or a real exponent (nlp_terms.needs_general); fpar set -- through sqphip_nlp_attach_general.  A model of the
        older calls stays on them, so they refuse what they always refused.  general = True / False overrides the choice
        (a model of the old class files the same bits through the new call).
        instance_data = True goes through sqphip_nlp_attach_data: the class of the general call, with shifts, coefficients
        and real exponents owned by the instance (the block f0 | g0 | c | b | a | p).  p's data starts every instance;
        nlp_set_instance(inst, q) and nlp_stream_set(scen, q) then also send q's fshift, acoef and fpar, and q must have
        p's structure.
        p's dense data blocks (p.blocks, nlp_terms.NlpBlock) follow whichever attach it was, through nlp_add_block in their
        order: their weights and shifts start every instance."""
        self._nlp_attach_terms(p, general, instance_data)
        for b in getattr(p, "blocks", None) or []:
            self.nlp_add_block(b)

    def _nlp_attach_terms(self, p, general, instance_data):
        # (sqphip_nlp_attach_data, _general, _affine or sqphip_nlp_attach: the choice nlp_attach documents)
        from .nlp_terms import nlp_terms_args
        if instance_data:
            if not hasattr(self.L, "sqphip_nlp_attach_data"):
                raise SqpHipError("libsqphip.so lacks sqphip_nlp_attach_data: rebuild it")
            general = True
        if general is None:
            general = bool(getattr(p, "general", False)) or getattr(p, "fpar", None) is not None
        if general:
            if not hasattr(self.L, "sqphip_nlp_attach_general"):
                raise SqpHipError("libsqphip.so lacks sqphip_nlp_attach_general: rebuild it")
            aptr, avar, acoef = nlp_terms_args(p)
            t = [np.ascontiguousarray(a, dtype=np.int64) for a in (p.trow, p.tptr, aptr, avar)]
            k = [np.ascontiguousarray(a, dtype=np.int32) for a in (p.fkind, p.fexp)]
            v = [_f(a) for a in (p.tcoef, acoef, p.fshift, p.g0)]
            par = None if getattr(p, "fpar", None) is None else _f(p.fpar)
            fn = self.L.sqphip_nlp_attach_data if instance_data else self.L.sqphip_nlp_attach_general
            self._ck(fn(self.h, len(t[0]), _l(t[0]), _d(v[0]), _l(t[1]), _l(t[2]), _l(t[3]), _d(v[1]),
                        _i(k[0]), _i(k[1]), _d(par), _d(v[2]), _d(v[3]), float(p.f0)))
            if instance_data:
                self._nlp_structure = self._nlp_structure_of(p)
            return
        if getattr(p, "aptr", None) is not None:
            t = [np.ascontiguousarray(a, dtype=np.int64) for a in (p.trow, p.tptr, p.aptr, p.avar)]
            k = [np.ascontiguousarray(a, dtype=np.int32) for a in (p.fkind, p.fexp)]
            v = [_f(a) for a in (p.tcoef, p.acoef, p.fshift, p.g0)]
            self._ck(self.L.sqphip_nlp_attach_affine(self.h, len(t[0]), _l(t[0]), _d(v[0]), _l(t[1]), _l(t[2]), _l(t[3]), _d(v[1]),
                                                     _i(k[0]), _i(k[1]), _d(v[2]), _d(v[3]), float(p.f0)))
            return
        t = [np.ascontiguousarray(a, dtype=np.int64) for a in (p.trow, p.tptr, p.fvar)]
        k = [np.ascontiguousarray(a, dtype=np.int32) for a in (p.fkind, p.fexp)]
        v = [_f(a) for a in (p.tcoef, p.fscale, p.fshift, p.g0)]
        self._ck(self.L.sqphip_nlp_attach(self.h, len(t[0]), _l(t[0]), _d(v[0]), _l(t[1]), _l(t[2]), _i(k[0]), _i(k[1]),
                                          _d(v[1]), _d(v[2]), _d(v[3]), float(p.f0)))

    _NLP_DATA = ("fshift", "acoef", "fpar")

    @staticmethod
    def _nlp_structure_of(p):
        """what the instances of a context of nlp_attach(instance_data=True) share: trow, tptr, aptr, avar, fkind, fexp"""
        from .nlp_terms import nlp_terms_args
        aptr, avar, _ = nlp_terms_args(p)
        return [np.asarray(a).astype(np.int64) for a in (p.trow, p.tptr, aptr, avar, p.fkind, p.fexp)]

    def _nlp_data_of(self, who, p, values):
        """(values without the data keywords, [fshift, acoef, fpar] or None): the data parts of p and of the keywords on a
        context of nlp_attach(instance_data=True); the keywords are refused on any other context."""
        from .nlp_terms import nlp_terms_args
        struct = getattr(self, "_nlp_structure", None)
        data = {k: values.pop(k) for k in self._NLP_DATA if k in values}
        if struct is None:
            if data:
                raise TypeError(f"{who}: {sorted(data)} need a context of nlp_attach(instance_data=True)")
            return values, None
        if p is not None:
            mine = self._nlp_structure_of(p)
            for name, a, b in zip(("trow", "tptr", "aptr", "avar", "fkind", "fexp"), struct, mine):
                if a.shape != b.shape or not np.array_equal(a, b):
                    raise SqpHipError(f"{who}: the structure of the model ({name}) differs from the attached one")
            data = {"fshift": p.fshift, "acoef": nlp_terms_args(p)[2], "fpar": getattr(p, "fpar", None), **data}
        return values, [None if data.get(k) is None else _f(np.atleast_1d(data[k])) for k in self._NLP_DATA]

    def nlp_set_instance(self, inst, p=None, x0=None, **values):
        """Per-instance values (sqphip_nlp_set_instance).  With an NlpTerms p: its bounds, every value and its start; keywords
        f0, g0, tcoef override single parts, and what is given neither way is kept.  On a context of
        nlp_attach(instance_data=True) p's fshift, acoef and fpar go along (sqphip_nlp_set_instance_data; p must have the
        attached structure) and the keywords fshift, acoef, fpar override single parts."""
        values = dict(values)
        blocks = self._nlp_block_data("nlp_set_instance", p, values)
        values, data = self._nlp_data_of("nlp_set_instance", p, values)
        if p is not None:
            self.set_bounds(inst, p)
            values = {**{k: getattr(p, k) for k in ("f0", "g0", "tcoef")}, **values}
            x0 = p.x0 if x0 is None else x0
        bad = set(values) - {"f0", "g0", "tcoef"}
        if bad:
            raise TypeError(f"nlp_set_instance: unknown values {sorted(bad)}")
        arr = [None if values.get(k) is None else _f(np.atleast_1d(values[k])) for k in ("f0", "g0", "tcoef")]
        self._ck(self.L.sqphip_nlp_set_instance(self.h, inst, *[_d(a) for a in arr], _d(_f(x0))))
        if data is not None and any(a is not None for a in data):
            self._ck(self.L.sqphip_nlp_set_instance_data(self.h, inst, *[_d(a) for a in data]))
        for k, w, sh in blocks:
            self.nlp_set_instance_block(inst, k, w, sh)

    def acopf_eval(self, inst, x, sigma=1.0, lam=None):
        f = C.c_double(); grad = np.zeros(self.n); g = np.zeros(self.m)
        jv = np.zeros(self.nnzj); hv = np.zeros(self.nnzh) if lam is not None else None
        self._ck(self.L.sqphip_acopf_eval(self.h, inst, _d(_f(x)), float(sigma), _d(_f(lam)), C.byref(f),
                                          _d(grad), _d(g), _d(jv), _d(hv)))
        return dict(f=f.value, grad=grad, g=g, jval=jv, hval=hv)

    def sqp_reset(self):
        self._ck(self.L.sqphip_sqp_reset(self.h))

    def sqp_run(self, max_outer=0):
        self._ck(self.L.sqphip_sqp_run(self.h, int(max_outer)))

    def sqp_get(self, inst):
        x = np.zeros(self.n); g = np.zeros(self.m); mg = np.zeros(self.m)
        ml = np.zeros(self.n); mu = np.zeros(self.n)
        obj = C.c_double(); st = C.c_int32(); it = C.c_int32()
        self._ck(self.L.sqphip_sqp_get(self.h, inst, _d(x), _d(g), _d(mg), _d(ml), _d(mu), C.byref(obj),
                                       C.byref(st), C.byref(it)))
        return dict(x=x, g=g, mult_g=mg, mult_x_L=ml, mult_x_U=mu, obj_val=obj.value, status=st.value,
                    iter=it.value)

    def sqp_status(self):
        ret = np.zeros(self.batch, dtype=np.int32); it = np.zeros(self.batch, dtype=np.int32)
        done = np.zeros(self.batch, dtype=np.int32)
        self._ck(self.L.sqphip_sqp_status(self.h, _i(ret), _i(it), _i(done)))
        return ret, it, done

    def sqp_trace(self, inst, cap=4096):
        rows = np.zeros((cap, 12)); n = C.c_int32()
        self._ck(self.L.sqphip_sqp_trace(self.h, inst, _d(rows), cap, C.byref(n)))
        names = ("iter", "accepted", "fr", "sub_status", "ipm_iters", "f", "phi", "mu", "delta", "pnorm",
                 "prim_infeas", "dual_infeas")
        out = []
        for k in range(min(n.value, cap)):
            r = dict(zip(names, rows[k]))
            for key in names[:5]:
                r[key] = int(r[key])
            out.append(r)
        return out

    # ---- multi-GPU status gather (RCCL inside the library)
    @staticmethod
    def comm_available() -> bool:
        """librccl loads in this process (ask on every rank and agree before the collective comm_init)"""
        return bool(_lib.lib().sqphip_comm_available())

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = _lib.lib().sqphip_comm_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            raise SqpHipError(f"sqphip_comm_unique_id failed ({rc})")
        return buf.raw

    def comm_init(self, unique_id: bytes, world: int, rank: int):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._ck(self.L.sqphip_comm_init(self.h, C.cast(buf, C.c_void_p), int(world), int(rank)))

    def gather_status(self, total: int):
        ret = np.zeros(total, dtype=np.int32); it = np.zeros(total, dtype=np.int32); done = np.zeros(total, dtype=np.int32)
        self._ck(self.L.sqphip_gather_status(self.h, int(total), _i(ret), _i(it), _i(done)))
        return ret, it, done

    def comm_destroy(self):
        self._ck(self.L.sqphip_comm_destroy(self.h))

    def counters(self):
        c = _lib.Counters()
        self._ck(self.L.sqphip_get_counters(self.h, C.byref(c)))
        return {k: getattr(c, k) for k, _ in _lib.Counters._fields_}

    def mode_counters(self):
        """Work of the batched run since sqp_reset by sub-problem mode: {mode: (sub-problems, IPM iterations,
        factorisations)} for QP / FR / SOC / LP."""
        out = (C.c_int64 * 12)()
        self._ck(self.L.sqphip_get_mode_counters(self.h, out))
        return {name: (out[3 * k], out[3 * k + 1], out[3 * k + 2]) for k, name in enumerate(("QP", "FR", "SOC", "LP"))}

    def sqp_work(self):
        """Per instance: (sub-problems, IPM iterations, factorisations) since sqp_reset, three int64 arrays."""
        out = [np.zeros(self.batch, dtype=np.int64) for _ in range(3)]
        self._ck(self.L.sqphip_sqp_work(self.h, *[a.ctypes.data_as(C.POINTER(C.c_int64)) for a in out]))
        return tuple(out)

    def sqp_qp_log(self, inst):
        """The last (up to 64) sub-problems of an instance: list of (mode, MOI status, IPM iterations, factorisations)."""
        rows = np.zeros((64, 4), dtype=np.int32); n = C.c_int32()
        self._ck(self.L.sqphip_sqp_qp_log(self.h, inst, _i(rows), 64, C.byref(n)))
        return [tuple(int(v) for v in rows[k]) for k in range(n.value)]

    def sqp_qp_log_term(self, inst):
        """For the rows of sqp_qp_log: (final scaled optimality error, rule that ended the interior-point run: 0 tolerance,
        1 / 2 / 3 acceptable-termination rules, -1 not converged)."""
        err = np.zeros(64); rule = np.zeros(64, dtype=np.int32); n = C.c_int32()
        self._ck(self.L.sqphip_sqp_qp_log_term(self.h, inst, _d(err), _i(rule), 64, C.byref(n)))
        return [(float(err[k]), int(rule[k])) for k in range(n.value)]

    def termination_counters(self):
        """Sub-problems of the batched run since sqp_reset ended by (tolerance, rule 1, rule 2, rule 3)."""
        out = (C.c_int64 * 4)()
        self._ck(self.L.sqphip_get_termination_counters(self.h, out))
        return tuple(int(v) for v in out)

    def sqp_last_request(self, inst):
        """The sub-problem request an instance of the batched run worked on last (arguments of QpHip / sqphip_qp_solve)."""
        mode = C.c_int32(); delta = C.c_double(); mu = C.c_double()
        xk = np.zeros(self.n); c = np.zeros(self.n); b = np.zeros(self.m); jc = np.zeros(self.nnzj); hc = np.zeros(self.nnzh)
        self._ck(self.L.sqphip_sqp_last_request(self.h, inst, C.byref(mode), C.byref(delta), C.byref(mu), _d(xk), _d(c),
                                                _d(b), _d(jc), _d(hc)))
        return dict(mode=mode.value, delta=delta.value, mu_pen=mu.value, x_k=xk, c=c, b=b, jac_coo=jc, hess_coo=hc)

    # ---- scenario queue (more scenarios than slots)
    def stream_begin(self, n_scenarios):
        self._ck(self.L.sqphip_sqp_stream_begin(self.h, int(n_scenarios)))

    def stream_set(self, scen, net, lay, x0=None):
        self._ck(self.L.sqphip_sqp_stream_set(self.h, int(scen), _d(_f(lay.xL)), _d(_f(lay.xU)), _d(_f(lay.gL)), _d(_f(lay.gU)),
                                              _d(_f(net.branch_coeffs().ravel())), _d(_f(net.c2)), _d(_f(net.c1)),
                                              _d(_f(lay.x0 if x0 is None else x0))))

    def stream_run(self):
        self._ck(self.L.sqphip_sqp_stream_run(self.h))

    # ... shared between ranks: this rank's part of the queue as an explicit id list
    def stream_assign(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        self._ck(self.L.sqphip_sqp_stream_assign(self.h, len(a), _i(a)))

    def stream_append(self, ids):
        a = np.ascontiguousarray(ids, dtype=np.int32)
        self._ck(self.L.sqphip_sqp_stream_append(self.h, len(a), _i(a)))

    def stream_release(self, n):
        """take up to n unstarted ids off the tail of this rank's queue"""
        out = np.zeros(max(1, int(n)), dtype=np.int32); k = C.c_int32()
        self._ck(self.L.sqphip_sqp_stream_release(self.h, int(n), _i(out), C.byref(k)))
        return out[:k.value].copy()

    def stream_run_some(self, max_outer):
        """every slot performs up to max_outer more outer iterations; returns (unstarted ids of this rank, slots still running)"""
        u, a = C.c_int32(), C.c_int32()
        self._ck(self.L.sqphip_sqp_stream_run_some(self.h, int(max_outer), C.byref(u), C.byref(a)))
        return u.value, a.value

    def stream_get(self, scen):
        x = np.zeros(self.n); obj = C.c_double(); st = C.c_int32(); it = C.c_int32()
        self._ck(self.L.sqphip_sqp_stream_get(self.h, int(scen), _d(x), C.byref(obj), C.byref(st), C.byref(it)))
        return dict(x=x, obj_val=obj.value, status=st.value, iter=it.value)

    # ... on a QCQP context (qcqp_attach): stream_run / _assign / _append / _release / _run_some / stream_get are shared
    def qcqp_stream_begin(self, n_scenarios, keep_multipliers=False):
        """Tables for n_scenarios (sqphip_qcqp_stream_begin); keep_multipliers: stream_get_full returns g and the multipliers."""
        self._ck(self.L.sqphip_qcqp_stream_begin(self.h, int(n_scenarios), int(bool(keep_multipliers))))

    def qcqp_stream_set(self, scen, q=None, x0=None, **values):
        """One scenario (sqphip_qcqp_stream_set), with the conventions of qcqp_set_instance.  With a Qcqp q: its bounds, every
        value and its start; keywords f0, c, q0v, g0, av, qv override single parts and xL, xU, gL, gU single bounds.  A value
        given neither way is the one of qcqp_attach, a bound given neither way the one the context was created with."""
        names, bnames = ("f0", "c", "q0v", "g0", "av", "qv"), ("xL", "xU", "gL", "gU")
        if q is not None:
            values = {**{k: getattr(q, k) for k in names + bnames}, **values}
            x0 = q.x0 if x0 is None else x0
        bad = set(values) - set(names + bnames)
        if bad:
            raise TypeError(f"qcqp_stream_set: unknown values {sorted(bad)}")
        arr = [None if values.get(k) is None else _f(np.atleast_1d(values[k])) for k in bnames + names]
        self._ck(self.L.sqphip_qcqp_stream_set(self.h, int(scen), *[_d(a) for a in arr], _d(_f(x0))))

    # ... on a factorable-NLP context (nlp_attach): the same calls are shared
    def nlp_stream_begin(self, n_scenarios, keep_multipliers=False):
        """Tables for n_scenarios (sqphip_nlp_stream_begin); keep_multipliers: stream_get_full returns g and the multipliers."""
        self._ck(self.L.sqphip_nlp_stream_begin(self.h, int(n_scenarios), int(bool(keep_multipliers))))

    def nlp_stream_set(self, scen, p=None, x0=None, **values):
        """One scenario (sqphip_nlp_stream_set), with the conventions of qcqp_stream_set.  With an NlpTerms p: its bounds, every
        value and its start; keywords f0, g0, tcoef override single parts and xL, xU, gL, gU single bounds.  A value given
        neither way is the one of nlp_attach, a bound given neither way the one the context was created with.  On a context of
        nlp_attach(instance_data=True) p's fshift, acoef and fpar follow through sqphip_nlp_stream_set_data (p must have the
        attached structure); the keywords fshift, acoef, fpar override single parts, and a part given neither way is the
        attach's."""
        names, bnames = ("f0", "g0", "tcoef"), ("xL", "xU", "gL", "gU")
        values = dict(values)
        blocks = self._nlp_block_data("nlp_stream_set", p, values)
        values, data = self._nlp_data_of("nlp_stream_set", p, values)
        if p is not None:
            values = {**{k: getattr(p, k) for k in names + bnames}, **values}
            x0 = p.x0 if x0 is None else x0
        bad = set(values) - set(names + bnames)
        if bad:
            raise TypeError(f"nlp_stream_set: unknown values {sorted(bad)}")
        arr = [None if values.get(k) is None else _f(np.atleast_1d(values[k])) for k in bnames + names]
        self._ck(self.L.sqphip_nlp_stream_set(self.h, int(scen), *[_d(a) for a in arr], _d(_f(x0))))
        if data is not None and any(a is not None for a in data):
            self._ck(self.L.sqphip_nlp_stream_set_data(self.h, int(scen), *[_d(a) for a in data]))
        for k, w, sh in blocks:
            self.nlp_stream_set_block(scen, k, w, sh)

    def stream_get_full(self, scen):
        """The dict of sqp_get for a scenario of a queue begun with keep_multipliers (sqphip_sqp_stream_get_full)."""
        x = np.zeros(self.n); g = np.zeros(self.m); mg = np.zeros(self.m)
        ml = np.zeros(self.n); mu = np.zeros(self.n)
        obj = C.c_double(); st = C.c_int32(); it = C.c_int32()
        self._ck(self.L.sqphip_sqp_stream_get_full(self.h, int(scen), _d(x), _d(g), _d(mg), _d(ml), _d(mu), C.byref(obj),
                                                   C.byref(st), C.byref(it)))
        return dict(x=x, g=g, mult_g=mg, mult_x_L=ml, mult_x_U=mu, obj_val=obj.value, status=st.value,
                    iter=it.value)

    def reset_counters(self):
        self._ck(self.L.sqphip_reset_counters(self.h))

    KERNEL_CLASSES = ("values", "fronts_low", "fronts_top", "solve_top", "solve_levels", "post", "transitions")

    def kernel_times(self):
        """{class: (seconds of kernel time, launch groups timed)} since reset_counters (set_timing(2) collects them)."""
        sec = np.zeros(7); grp = np.zeros(7, dtype=np.int64)
        self._ck(self.L.sqphip_get_kernel_times(self.h, _d(sec), grp.ctypes.data_as(C.POINTER(C.c_int64)), 7))
        return {k: (float(sec[i]), int(grp[i])) for i, k in enumerate(self.KERNEL_CLASSES)}

    def set_timing(self, on: bool):
        self._ck(self.L.sqphip_set_timing(self.h, int(on)))


# ------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class QpData:
    """subproblem.jl:12-23.  Q / A are carried as COO values in the structure order of the Model
    (what eval_h / eval_jac_g fill); the library merges duplicates and mirrors the Hessian."""
    Q: np.ndarray | None
    c: np.ndarray
    A: np.ndarray
    b: np.ndarray
    c_lb: np.ndarray
    c_ub: np.ndarray
    v_lb: np.ndarray
    v_ub: np.ndarray
    num_linear_constraints: int


class QpHip:
    """`AbstractSubOptimizer` backed by libsqphip; method names and 6-tuple returns follow QpJuMP."""

    def __init__(self, ctx: Context, data: QpData | None = None):
        self.ctx = ctx
        self.data = data

    def create_model(self, delta):          # subproblem_JuMP.jl:36-125: nothing to build, the ctx is the model
        return None

    def _solve(self, mode, x_k, delta, mu=1.0):
        dta = self.data
        r = self.ctx.qp_solve(mode, x_k, delta, mu, dta.c, dta.b, dta.A, dta.Q)
        return r["p"], r["lam"], r["mult_x_U"], r["mult_x_L"], r["slack"], r["status"]

    def sub_optimize(self, x_k, delta):
        return self._solve(MODE_QP, x_k, delta)

    def sub_optimize_FR(self, x_k, delta):
        return self._solve(MODE_FR, x_k, delta)

    def sub_optimize_L1QP(self, x_k, delta, mu):
        return self._solve(MODE_L1QP, x_k, delta, mu)

    def sub_optimize_infeas(self, x_k, delta):
        p, _, _, _, slack, st = self._solve(MODE_INFEAS, x_k, delta)
        return p, (float(slack.sum()) if st in _OK else math.inf)

    def sub_optimize_lp(self, x_k):
        p, lam, mu_u, mu_l, _, st = self._solve(MODE_LP, x_k, math.inf)
        return p, lam, mu_u, mu_l, st

    # ---- many models at once: lists of QpData (one per request) on the instances `inst` of the context
    def _solve_batch(self, inst, mode, datas, x_k, delta, mu=1.0):
        cnt = len(datas)
        hv = None if any(d.Q is None for d in datas) else [d.Q for d in datas]
        rs = self.ctx.qp_solve_batch(inst, [mode] * cnt, x_k, delta, mu, [d.c for d in datas], [d.b for d in datas],
                                     [d.A for d in datas], hv)
        return [(r["p"], r["lam"], r["mult_x_U"], r["mult_x_L"], r["slack"], r["status"]) for r in rs]

    def sub_optimize_batch(self, inst, datas, x_k, delta):
        return self._solve_batch(inst, MODE_QP, datas, x_k, delta)

    def sub_optimize_FR_batch(self, inst, datas, x_k, delta):
        return self._solve_batch(inst, MODE_FR, datas, x_k, delta)

    def sub_optimize_lp_batch(self, inst, datas, x_k):
        return [(p, lam, mu_u, mu_l, st) for p, lam, mu_u, mu_l, _, st in
                self._solve_batch(inst, MODE_LP, datas, x_k, math.inf)]
