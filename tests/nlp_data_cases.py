"""Cases of the per-instance data tests (sqphip_nlp_attach_data; tests/test_gpu_nlp_data.py runs them on the device,
tests/test_nlp_data_cpu.py vouches for them without one): models whose instances differ in the shifts, argument
coefficients and real exponents of their factors, each instance with its own NlpTerms and therefore its own reference
(tests/nlp_general_ref.py NlpGeneralRef / OracleGeneralTerms).

    data_model         nlp_general_synth(24, 14): an even block count
    edge_model         general_edge_model(): an odd block count, the padding double in use
    wide_model         more factors than one stride of the thread loops (1024)
    data_scenarios     nlp_data_scenario instances of a model
    block_count        1 + m + nterms + nfac + nargs (+ nfac with a POWR factor): the doubles of an instance before padding
    folds_case         a dataset and its k = 4 logistic training folds
    consumers_case     four Cobb-Douglas consumers with their own elasticities"""
from __future__ import annotations

import numpy as np

from nlp_general_ref import general_edge_model
from sqpsolver_jl_amd.nlp_terms import (cobb_douglas_model, logistic_fold_indices, logistic_folds, nlp_data_scenario,
                                        nlp_general_synth, nlp_terms_args, nlp_terms_layout)

DATA_SEED = 1
BATCH_SCENARIOS = (1, 2, 3, 4)                 # every slot with data of its own, none the attach's
QUEUE_DATA_SCENARIOS = tuple(range(6))
STRUCTURE = ("trow", "tptr", "fvar", "fkind", "fexp")


def data_model():
    p = nlp_general_synth(24, 14, seed=DATA_SEED)
    return p, nlp_terms_layout(p)


def edge_model():
    return general_edge_model()


def wide_model():
    p = nlp_general_synth(260, 200, seed=2)
    return p, nlp_terms_layout(p)


def data_scenarios(p, which=BATCH_SCENARIOS, noise=0.05):
    return [nlp_data_scenario(p, s, DATA_SEED, noise) for s in which]


def block_count(p) -> int:
    nfac, nargs = len(p.fkind), len(nlp_terms_args(p)[1])
    return 1 + p.m + len(p.trow) + nfac + nargs + (nfac if p.fpar is not None else 0)


def same_structure(p, q) -> bool:
    a, b = nlp_terms_args(p), nlp_terms_args(q)
    return (all(np.array_equal(getattr(p, k), getattr(q, k)) for k in STRUCTURE)
            and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def data_differs(p, q) -> float:
    """largest difference in the data of the factors (shifts, coefficients, real exponents)"""
    d = max(np.abs(p.fshift - q.fshift).max(), np.abs(nlp_terms_args(p)[2] - nlp_terms_args(q)[2]).max())
    return float(max(d, np.abs(p.fpar - q.fpar).max()) if p.fpar is not None else d)


def folds_case(k: int = 4):
    """(X, y, reg, folds, index pairs): 18 points with two features and an intercept; 18 % 4 = 2 points are dropped"""
    rng = np.random.default_rng(11)
    N = 18
    X = np.c_[np.ones(N), rng.standard_normal((N, 2))]
    y = (X @ np.array([0.3, 1.0, -0.7]) + 0.8 * rng.standard_normal(N) > 0).astype(float)
    reg = 0.5
    return X, y, reg, logistic_folds(X, y, reg, k), logistic_fold_indices(N, k)


def consumers_case():
    """(alphas [4][3], prices, wealth, models)"""
    alphas = np.array([[0.2, 0.3, 0.4], [0.5, 0.2, 0.1], [0.1, 0.1, 0.6], [0.3, 0.3, 0.3]])
    prices, wealth = np.array([1.0, 2.0, 0.5]), 10.0
    return alphas, prices, wealth, [cobb_douglas_model(a, prices, wealth) for a in alphas]
