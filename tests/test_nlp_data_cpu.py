"""Per-instance data of a factorable NLP without a GPU (sqphip_nlp_attach_data; sqpsolver.jl_amd/nlp_terms.py
nlp_data_scenario, logistic_folds; tests/nlp_data_cases.py): the invariants of the scenario generator, the folds, the
reference on a perturbed instance against finite differences, the three prototypes in the header, the ctypes table and the
Julia shim, and the oracle's convergence on every instance the GPU tests run (tests/test_gpu_nlp_data.py)."""
import inspect
import itertools
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import oracle as O                                        # noqa: E402
from sqpsolver_jl_amd import _lib                                     # noqa: E402
from sqpsolver_jl_amd.nlp_terms import (POWR, cobb_douglas_model, logistic_fold_indices, logistic_folds, logistic_model,   # noqa: E402
                                        nlp_affine_synth, nlp_data_scenario, nlp_terms_args, nlp_terms_layout, nlp_terms_rows,
                                        nlp_terms_synth)
from nlp_general_ref import QUEUE_NOISE, SQP_KW, NlpGeneralRef, OracleGeneralTerms   # noqa: E402
from nlp_data_cases import (BATCH_SCENARIOS, DATA_SEED, QUEUE_DATA_SCENARIOS, block_count, consumers_case, data_differs,   # noqa: E402
                            data_model, data_scenarios, edge_model, folds_case, same_structure, wide_model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sqphip_nlp_attach_data", "sqphip_nlp_set_instance_data", "sqphip_nlp_stream_set_data")


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max()))


def test_the_entry_points_are_declared_exported_and_refuse_a_null_handle():
    L = _lib.lib()
    assert all(s in _lib.EXPORTS and hasattr(L, s) for s in NEW)
    assert L.sqphip_nlp_attach_data(None, 0, None, None, None, None, None, None, None, None, None, None, None, 0.0) == -1
    assert L.sqphip_nlp_set_instance_data(None, 0, None, None, None) == -1
    assert L.sqphip_nlp_stream_set_data(None, 0, None, None, None) == -1
    import sqpsolver_jl_amd as pkg
    assert "sqphip_nlp_attach_data" in inspect.getsource(pkg.Context.nlp_attach)
    assert "instance_data" in inspect.signature(pkg.Context.nlp_attach).parameters


def test_header_ctypes_and_julia_prototypes_agree():
    import ctypes as C
    attach = ["ctx", "i64", "i64*", "f64*", "i64*", "i64*", "i64*", "f64*", "i32*", "i32*", "f64*", "f64*", "f64*", "f64"]
    data = ["ctx", "i32", "f64*", "f64*", "f64*"]
    want = dict(zip(NEW, (attach, data, data)))
    names = dict(zip(NEW, (["ctx", "nterms", "trow", "tcoef", "tptr", "aptr", "avar", "acoef", "fkind", "fexp", "fpar", "fshift", "g0", "f0"],
                           ["ctx", "inst", "fshift", "acoef", "fpar"], ["ctx", "scenario", "fshift", "acoef", "fpar"])))
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sqphip.h")).read(), flags=re.S)
    ckind = lambda a: ("ctx" if "sqphip_ctx" in a else
                       {"int64_t": "i64", "int32_t": "i32", "double": "f64"}[re.search(r"int64_t|int32_t|double", a).group(0)] + ("*" if "*" in a else ""))
    table = {C.c_void_p: "ctx", C.c_int64: "i64", C.c_int32: "i32", C.c_double: "f64", C.POINTER(C.c_int64): "i64*",
             C.POINTER(C.c_int32): "i32*", C.POINTER(C.c_double): "f64*"}
    jkind = {"Ptr{Cvoid}": "ctx", "Int64": "i64", "Int32": "i32", "Cdouble": "f64", "Ptr{Int64}": "i64*", "Ptr{Int32}": "i32*",
             "Ptr{Cdouble}": "f64*"}
    jl = re.sub(r"#[^\n]*", "", open(os.path.join(ROOT, "julia", "SqpHip.jl")).read())
    general = re.search(r"\bint\s+sqphip_nlp_attach_general\s*\(([^;]*?)\)\s*;", hdr, flags=re.S).group(1).split(",")
    for fn in NEW:
        args = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % fn, hdr, flags=re.S).group(1).split(",")
        assert [ckind(a) for a in args] == want[fn], fn
        assert [re.findall(r"\w+", a)[-1] for a in args] == names[fn], fn
        assert [table[t] for t in getattr(_lib.lib(), fn).argtypes] == want[fn], fn
        ret, argt = re.search(r"ccall\(\(:%s, LIBSQPHIP\),\s*(\w+),\s*\((.*?)\)\s*,\s*ctx" % fn, jl, flags=re.S).groups()
        assert ret == "Cint" and [jkind[a] for a in re.findall(r"Ptr\{\w+\}|\w+", argt)] == want[fn], fn
        assert "hip_" + fn[len("sqphip_"):] + "(" in jl
    # the argument list of the general call
    assert [ckind(a) for a in general] == attach and [re.findall(r"\w+", a)[-1] for a in general] == names[NEW[0]]


@pytest.mark.parametrize("model", ["synth", "edge", "one_argument", "affine"])
def test_data_scenario_keeps_structure_linear_rows_row_values_and_domain(model):
    p = dict(synth=lambda: data_model()[0], edge=lambda: edge_model()[0], one_argument=lambda: nlp_terms_synth(24, 14, seed=5),
             affine=lambda: nlp_affine_synth(24, 14, seed=1))[model]()
    assert nlp_data_scenario(p, 0, 3) is p
    aptr, avar, acoef = nlp_terms_args(p)
    lin_fac = np.flatnonzero(np.isin(np.repeat(p.trow, np.diff(p.tptr)), np.arange(1, p.num_linear + 1)))
    assert model == "edge" or len(lin_fac) > 0
    R0 = NlpGeneralRef(p)
    for noise in (0.05, QUEUE_NOISE):
        for seed in range(1, 6):
            q = nlp_data_scenario(p, 2, seed, noise)
            assert same_structure(p, q) and (q.aptr is None) == (p.aptr is None)
            assert np.array_equal(q.tcoef, p.tcoef) and q.f0 == p.f0 and np.array_equal(q.x0, p.x0)
            assert all(np.array_equal(getattr(q, k), getattr(p, k)) for k in ("xL", "xU", "gL", "gU"))
            qa = nlp_terms_args(q)[2]
            assert np.array_equal(q.fshift[lin_fac], p.fshift[lin_fac]) and np.array_equal(qa[aptr[lin_fac]], acoef[aptr[lin_fac]])
            assert np.array_equal(q.fscale, qa[aptr[:-1]])                     # fscale: the first argument of every factor
            assert data_differs(p, q) > 0.5 * noise
            assert np.abs(nlp_terms_rows(q, q.x0) - nlp_terms_rows(p, p.x0)).max() <= 1e-12
            R = NlpGeneralRef(q)
            assert np.abs(R.g(q.x0) - R0.g(p.x0)).max() <= 1e-12
            assert R.domain_margin(q.x0) > 0 and R.domain_margin(q.x0) >= 0.5 * R0.domain_margin(p.x0) - 1e-12
            if p.fpar is not None:
                k = p.fkind == POWR
                assert np.all(np.isfinite(q.fpar)) and np.all(q.fpar[k] != 0.0) and np.array_equal(q.fpar[~k], p.fpar[~k])
    # other scenarios and other seeds are other data
    qs = [nlp_data_scenario(p, s, 1) for s in (1, 2)] + [nlp_data_scenario(p, 1, 2)]
    assert min(data_differs(a, b) for a, b in itertools.combinations(qs, 2)) > 1e-3


def test_the_box_margin_of_the_generated_models_survives_the_noise():
    """LOG, SQRT, POWR and negative powers of the generated models are positive on the whole box; the scenarios keep at least
    half of that margin, so the device tests may evaluate anywhere inside the box."""
    for p in (data_model()[0], wide_model()[0]):
        aptr, avar, acoef = nlp_terms_args(p)
        need = np.isin(p.fkind, (4, 5, POWR)) | ((p.fkind == 0) & (p.fexp < 0))
        fa = np.repeat(np.arange(len(p.fkind)), np.diff(aptr))

        def box_min(q):
            a = nlp_terms_args(q)[2]
            return np.bincount(fa, np.where(a >= 0, a * q.xL[avar - 1], a * q.xU[avar - 1]), len(q.fkind)) + q.fshift
        m0 = box_min(p)[need]
        assert m0.min() > 0.09
        for q in data_scenarios(p, (1, 2, 3, 4, 5), QUEUE_NOISE) + data_scenarios(p):
            assert np.all(box_min(q)[need] >= 0.5 * m0 - 1e-12)


def test_logistic_folds_share_one_structure_and_validate_on_disjoint_parts():
    X, y, reg, folds, idx = folds_case(4)
    N = len(y)
    assert len(folds) == 4 and N % 4 == 2
    val = [set(v.tolist()) for _, v in idx]
    assert all(len(v) == N // 4 for v in val) and not any(a & b for a, b in itertools.combinations(val, 2))
    assert set().union(*val) == set(range(4 * (N // 4)))                  # the remainder is dropped
    for (tr, v), f in zip(idx, folds):
        assert set(tr.tolist()) | set(v.tolist()) == set(range(16)) and not set(tr.tolist()) & set(v.tolist())
        assert same_structure(folds[0], f) and len(tr) == 12
        one = logistic_model(X[tr], y[tr], reg)
        assert np.array_equal(f.acoef, one.acoef) and np.array_equal(f.tcoef, one.tcoef)
        assert np.array_equal(f.acoef[:len(tr) * X.shape[1]].reshape(len(tr), -1), X[tr])
    assert min(data_differs(a, b) for a, b in itertools.combinations(folds, 2)) > 1e-3
    assert [len(t) for t, _ in logistic_fold_indices(10, 3)] == [6, 6, 6]
    assert len(logistic_folds(X, y, reg, 3)) == 3
    alphas, prices, wealth, models = consumers_case()
    assert all(same_structure(models[0], m) for m in models) and "one context" in " ".join(cobb_douglas_model.__doc__.split())


def _dense_jac(R, lay, x):
    J = np.zeros((lay.m, lay.n)); J[lay.jrow - 1, lay.jcol - 1] = R.jac(x, lay.jrow, lay.jcol)
    return J


def test_reference_on_a_perturbed_instance_matches_finite_differences():
    """the method of tests/test_nlp_general_cpu.py: central differences with h = 1e-6"""
    rng = np.random.default_rng(0)
    for p, lay in (data_model(), edge_model()):
        q = nlp_data_scenario(p, 3, DATA_SEED, QUEUE_NOISE)
        R = NlpGeneralRef(q)
        x = rng.uniform(0.6, 1.5, q.n); lam = rng.standard_normal(q.m)
        assert R.domain_margin(x) > 0
        h, sigma, E = 1e-6, 0.7, np.eye(q.n)
        fd_grad = np.array([(R.f(x + h * E[j]) - R.f(x - h * E[j])) / (2 * h) for j in range(q.n)])
        assert rel(R.grad(x), fd_grad) < 1e-8
        fd_J = np.stack([(R.g(x + h * E[j]) - R.g(x - h * E[j])) / (2 * h) for j in range(q.n)], axis=1)
        assert rel(_dense_jac(R, lay, x), fd_J) < 1e-8
        Lg = lambda z: sigma * R.grad(z) + _dense_jac(R, lay, z).T @ lam
        fd_H = np.stack([(Lg(x + h * E[j]) - Lg(x - h * E[j])) / (2 * h) for j in range(q.n)], axis=1)
        H = np.zeros((q.n, q.n))
        np.add.at(H, (lay.hrow - 1, lay.hcol - 1), R.hess(x, sigma, lam, lay.hrow, lay.hcol))
        assert rel(np.tril(fd_H), H) < 1e-7
        # the data is what moved: the same point through the unperturbed model differs
        assert rel(NlpGeneralRef(p).grad(x), R.grad(x)) > 1e-3


def test_block_counts_of_the_evaluator_cases_cover_both_parities():
    assert block_count(data_model()[0]) % 2 == 0 and block_count(edge_model()[0]) % 2 == 1
    assert len(wide_model()[0].fkind) > 1024


@pytest.mark.parametrize("kkt_mode", [2, 1])
def test_the_oracle_converges_on_every_instance_of_the_gpu_tests(kkt_mode):
    p, lay = data_model()
    lin = dict(kkt_mode=2) if kkt_mode == 2 else dict(kkt_mode=1, kkt_tile_order=1)
    try:
        for q in data_scenarios(p, BATCH_SCENARIOS) + data_scenarios(p, QUEUE_DATA_SCENARIOS, QUEUE_NOISE) + data_scenarios(p, (1, 2, 3)):
            ro = O.sqp_solve(OracleGeneralTerms(q, lay), O.default_options(**lin, **SQP_KW))
            assert ro["status"] == 0 and 2 <= ro["iter"] < SQP_KW["max_iter"]
    finally:
        O.set_kkt_order(None)
