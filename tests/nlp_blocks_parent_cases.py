"""The evaluations behind tests/golden/nlp_*_parent_bits.npz: every entry of the EDGE_CASES of the five families of dense data
blocks (scalar, several outputs, softmax, Cox, log-sum-exp) and their two-block companion models, at the x, sigma, lam at which
tests/test_gpu_nlp_block.py, _rowblock, _softmax, _cox and _lse evaluate them.  tests/golden/make_nlp_blocks_parent_bits.py
records them from a library, tests/test_gpu_nlp_blocks_parent_bits.py holds the tree's library to the records bit for bit.

What the shapes cover of the code the families share (nlp_blocks_dev.hpp): an N that is no multiple of 4 and an N above 1024 (one
thread stride) in every family; a Hessian of 1..15, 16, 17..31 and more than 32 columns (one tile, the tile edge, three tiles,
and with 117 or 128 columns more than 16 tiles on 16 waves) in every family; for the softmax block a tile that straddles a class
boundary ((5, 17, 2, 0)) and a tile whose rows and columns share no class ((64, 8, 16, 0)); for the log-sum-exp block R = 1, 2, 6
and 17 outputs.  The EDGE_CASES leave one hole, a softmax block of exactly 16 columns: SOFTMAX_EXTRA."""
import numpy as np

import nlp_block_ref as B
import nlp_cox_ref as X
import nlp_lse_ref as L
import nlp_rowblock_ref as R
import nlp_softmax_ref as S

FAMILIES = ("block", "rowblock", "softmax", "cox", "lse")
KEYS = ("f", "grad", "g", "jval", "hval")
SOFTMAX_EXTRA = (6, 8, 2, 0)                    # Kf d = 16: one full tile with the class boundary in its middle


def _edge(model, point):
    """an edge model: three instances with their own weights and shifts, each evaluated at point(p, b) = (x, sigma, lam)"""
    def build():
        p, lay, inst = model()
        return p, lay, 3, [(b, dict(weight=w, shift=s)) for b, (w, s) in enumerate(inst)], [(b,) + tuple(point(p, b)) for b in range(3)]
    return build


def _pair(model, data, lam):
    """a two-block model: instance 0 as attached, instance 1 with data(rng) = (weight, shift) by block; both at one x, sigma = 1.3"""
    def build():
        p, lay = model()
        rng = np.random.default_rng(2)
        kw = data(rng)
        x = rng.uniform(-1.0, 1.0, p.n)
        return p, lay, 2, [(1, kw)], [(b, x, 1.3, np.array(lam, dtype=float)) for b in range(2)]
    return build


def _two(rng, kw, ks, wshape=22):
    """the other data of instance 1 of a two-block model: weights of block kw, then shifts of the 37-point block ks"""
    w = rng.uniform(0.0, 1.0, wshape)
    return dict(weight={kw: w}, shift={ks: 0.1 * rng.standard_normal(37)})


def _rng_point(N, d, lam):
    return lambda p, b: (np.random.default_rng(N + d).uniform(0.6, 1.4, p.n), 0.7, lam)


def _rows_point(N, d, lam):
    return lambda p, b: (np.random.default_rng(N + d).uniform(0.6, 1.4, p.n), 0.0 if b == 2 else 0.7, lam)


def case_list(family):
    """[(name, build)]; build() -> (p, lay, batch, [(instance, keywords of nlp_set_instance)], [(instance, x, sigma, lam)])"""
    out = []
    if family == "block":
        for c in B.EDGE_CASES:
            out.append(("N%d-d%d-kind%d-e%d" % c, _edge(lambda c=c: B.edge_model(*c), _rng_point(c[0], c[1], np.array([0.8])))))
        out.append(("two-blocks", _pair(B.two_block_model, lambda rng: _two(rng, 1, 0), [])))
    elif family == "rowblock":
        for c in R.EDGE_CASES:
            out.append(("N%d-d%d-R%d-kind%d-e%d" % (c[0], c[1], len(c[2]), c[3], c[4]),
                        _edge(lambda c=c: R.edge_row_model(*c), _rows_point(c[0], c[1], R.EDGE_LAM))))
        out.append(("overlap", _pair(R.overlap_model, lambda rng: _two(rng, 1, 0, (2, 22)), [0.3, -0.6])))
    elif family == "softmax":
        for c, big in [(c, False) for c in S.EDGE_CASES] + [(S.BIG_LOGITS, True), (SOFTMAX_EXTRA, False)]:
            out.append(("N%d-d%d-K%d-pinned%d" % c + ("-big" if big else ""),
                        _edge(lambda c=c, big=big: S.edge_model(*c, big=big), lambda p, b, c=c: S.edge_point(p, c[0], c[1]))))
        for first in (False, True):
            ks = 0 if first else 1
            out.append(("mixed-softmax-first%d" % first, _pair(lambda first=first: S.mixed_model(first), lambda rng, ks=ks: _two(rng, ks, 1 - ks), [])))
    elif family == "cox":
        for c in X.EDGE_CASES:
            out.append((X.IDS[X.EDGE_CASES.index(c)], _edge(lambda c=c: X.edge_model(*c), lambda p, b, c=c: X.edge_point(p, c[0], c[1]))))
        for first in (False, True):
            kc = 0 if first else 1
            out.append(("mixed-cox-first%d" % first, _pair(lambda first=first: X.mixed_model(first), lambda rng, kc=kc: _two(rng, kc, 1 - kc), [])))
    elif family == "lse":
        for c in L.EDGE_CASES:
            out.append((L.IDS[L.EDGE_CASES.index(c)],
                        _edge(lambda c=c: L.edge_lse_model(*c), lambda p, b, c=c: (L.edge_point(p, c[0], c[1]), 0.0 if b == 2 else 0.7, L.EDGE_LAM))))

        def lse_data(rng, k):
            w1, s1 = rng.uniform(0.0, 1.0, 22), 0.1 * rng.standard_normal(22)
            w1[[0, 10]] = 1.0
            return dict(weight={k: w1}, shift={k: s1})
        for first in (False, True):
            out.append(("overlap-lse-first%d" % first, _pair(lambda first=first: L.overlap_model(first),
                        lambda rng, k=0 if first else 1: lse_data(rng, k), [0.3, -0.6])))
    else:
        raise ValueError(family)
    assert len({n for n, _ in out}) == len(out), family
    return out


def golden_path(here, family):
    return "%s/golden/nlp_%s_parent_bits.npz" % (here, family)


def run_case(pkg, build):
    """[(instance, acopf_eval's outputs, the outputs of the same call without the Hessian pointer)] of one case on the GPU"""
    import ctypes as C
    dp = C.POINTER(C.c_double)
    p, lay, batch, sets, evals = build()
    ctx = pkg.Context(lay.n, lay.m, lay.num_linear, lay.jrow, lay.jcol, lay.hrow, lay.hcol, lay.xL, lay.xU, lay.gL, lay.gU,
                      pkg.default_options(), batch=batch)
    ctx.nlp_attach(p)
    for b, kw in sets:
        ctx.nlp_set_instance(b, p, **kw)
    out = []
    for b, x, sigma, lam in evals:
        ev = ctx.acopf_eval(b, x, sigma, lam)
        xx, ll = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(lam, dtype=np.float64)
        f = C.c_double()
        no = dict(grad=np.zeros(ctx.n), g=np.zeros(ctx.m), jval=np.zeros(ctx.nnzj))
        ctx._ck(ctx.L.sqphip_acopf_eval(ctx.h, b, xx.ctypes.data_as(dp), float(sigma), ll.ctypes.data_as(dp), C.byref(f),
                                        no["grad"].ctypes.data_as(dp), no["g"].ctypes.data_as(dp), no["jval"].ctypes.data_as(dp), None))
        no["f"] = f.value
        out.append((b, ev, no))
    ctx.close()
    return out
