"""The host-side model compilers (csrc/model_plans.cpp: build_qcqp_plan, build_nlp_plan, nlp_data_check, nlp_block_columns)
without a GPU and without the library: tests/plan_smoke.cpp is compiled once per session together with model_plans.cpp
under the address and undefined-behaviour sanitizers and run as a child process on model files written here.

Accepted models: the row pointers are non-decreasing and end at the entry counts, every value, variable, row, term and
argument index is in range, the entries of one owner stand in term order, the stride is even and covers the values, and
the entry counts are those the term lists give by the rules of qcqp_dev.hpp / nlp_dev.hpp (counted here, in Python).
Rejected models: the message, byte for byte."""
from __future__ import annotations

import dataclasses
import os
import subprocess

import numpy as np
import pytest

import qcqp_cases as QC
from sqpsolver_jl_amd.nlp_terms import (COS, EXP, LOG, POW, POWR, SIN, cobb_douglas_model, make_nlp_terms, nlp_affine_synth,
                                        nlp_general_synth, nlp_terms_args, nlp_terms_layout, nlp_terms_synth)
from sqpsolver_jl_amd.qcqp import make_qcqp, qcqp_layout, qcqp_synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOATS = {"base", "fab", "acoef", "aw", "fpar"}
JMISS = " needs a Jacobian entry that the structure of sqphip_create lacks"
HMISS = " needs a Hessian entry that the structure of sqphip_create lacks"
ARG = (1 << 28) - 1


@pytest.fixture(scope="session")
def prog(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_smoke") / "plan_smoke"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                           "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "plan_smoke.cpp"),
                           os.path.join(ROOT, "sqpsolver.jl_amd", "csrc", "model_plans.cpp")])
    return str(exe)


_count = [0]


def run(prog, tmp_path, model, who, **arrays):
    """Writes the model file, runs the program; {name: int or float array | message}"""
    _count[0] += 1
    path = tmp_path / f"model{_count[0]}.txt"
    with open(path, "w") as fh:
        fh.write(f"model {model}\nwho {who}\n")
        for k, v in arrays.items():
            if v is None:
                fh.write(f"{k} -1\n")
                continue
            v = np.atleast_1d(np.asarray(v))
            tok = [float(x).hex() for x in v] if v.dtype.kind == "f" else [str(int(x)) for x in v]
            fh.write(" ".join([k, str(len(tok))] + tok) + "\n")
    r = subprocess.run([prog, str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]            # (a sanitizer report ends the program with one)
    out = {}
    for ln in r.stdout.splitlines():
        name, _, rest = ln.partition(" ")
        if name in ("err", "check"):
            out[name] = rest
            continue
        tok = rest.split()[1:]
        out[name] = np.array([float.fromhex(t) for t in tok]) if name in FLOATS else np.array([int(t) for t in tok], dtype=np.int64)
    return out


def structure(lay):
    return dict(n=lay.n, m=lay.m, nlin=lay.num_linear, jrow=lay.jrow, jcol=lay.jcol, hrow=lay.hrow, hcol=lay.hcol)


def segments(out, sizes):
    """The four CSR row pointers of the packed array, checked: where they start, non-decreasing, from 0 to the entry count"""
    ptr, starts = out["ptr"], [0, int(out["f_ptr"][0]), int(out["j_ptr"][0]), int(out["h_ptr"][0])]
    assert starts == list(np.cumsum([0] + [s + 1 for s in sizes[:3]])) and len(ptr) == sum(s + 1 for s in sizes)
    segs = [ptr[a:a + s + 1] for a, s in zip(starts, sizes)]
    for s in segs:
        assert s[0] == 0 and (np.diff(s) >= 0).all()
    return segs


def entries(out, name, width, seg):
    """The entries of a plan [count][width]; an empty plan keeps one padding entry"""
    e = out[name].reshape(-1, width)
    assert len(e) == max(int(seg[-1]), 1)
    return e[:int(seg[-1])]


def in_term_order(seg, key):
    for a, b in zip(seg[:-1], seg[1:]):
        assert (np.diff(key[a:b]) >= 0).all()


def owners(seg):
    return np.repeat(np.arange(len(seg) - 1), np.diff(seg))


# ------------------------------------------------------------------------------------------------ the QCQP builder
def qcqp_arrays(q, lay):
    return dict(structure(lay), nnzQ0=len(q.q0v), q0r=q.q0r, q0c=q.q0c, q0v=q.q0v, nnzA=len(q.av), ar=q.ar, ac=q.ac, av=q.av,
                nnzQ=len(q.qv), qi=q.qi, qr=q.qr, qc=q.qc, qv=q.qv, c=q.c, g0=q.g0, f0=float(q.f0))


def run_qcqp(prog, tmp_path, q, lay, **over):
    return run(prog, tmp_path, "qcqp", "sqphip_qcqp_attach", **{**qcqp_arrays(q, lay), **over})


def check_qcqp_plan(q, lay, out):
    assert out["rc"][0] == 0, out.get("err")
    n, m, nnzJ, nnzH = lay.n, lay.m, len(lay.jrow), len(lay.hrow)
    nq0, na, nq = len(q.q0v), len(q.av), len(q.qv)
    off = out["off"]
    assert list(off) == [0, 1, 1 + n, 1 + n + nq0, 1 + n + nq0 + m, 1 + n + nq0 + m + na, QC.nvalues(q)]
    nvals, nv = int(off[6]), int(out["nv"][0])
    assert nv % 2 == 0 and nvals <= nv <= nvals + 1 and len(out["base"]) == nv
    assert np.array_equal(out["base"][:nvals], np.concatenate([[q.f0], q.c, q.q0v, q.g0, q.av, q.qv])) and not out["base"][nvals:].any()
    assert (out["n"][0], out["m"][0], out["nq0"][0]) == (n, m, nq0)
    g, f, j, h = segments(out, [m, n, nnzJ, nnzH])
    # the counts, from the term lists: a Q term is one row entry; a Q0 term feeds the gradient of both its variables, a Q term
    # the Jacobian slots of both (a diagonal one: once); every Q0 and Q term has one Hessian entry (none without a structure)
    assert g[-1] == na + nq
    assert f[-1] == int(np.sum(np.where(q.q0r == q.q0c, 1, 2)))
    assert j[-1] == na + int(np.sum(np.where(q.qr == q.qc, 1, 2)))
    assert h[-1] == (nq0 + nq if nnzH else 0)
    ge, fe, je, he = entries(out, "ge", 4, g), entries(out, "fe", 2, f), entries(out, "je", 2, j), entries(out, "he", 2, h)
    for e in (ge, fe, je, he):
        assert ((e[:, 0] >= 0) & (e[:, 0] < nvals)).all()
    assert ((ge[:, 1] >= 0) & (ge[:, 1] < n) & (ge[:, 2] >= -1) & (ge[:, 2] < n) & (ge[:, 3] == 0)).all()
    assert ((fe[:, 1] >= 0) & (fe[:, 1] < n)).all() and ((je[:, 1] >= -1) & (je[:, 1] < n)).all()
    assert ((he[:, 1] >= -1) & (he[:, 1] < m)).all()
    for seg, e in ((g, ge), (f, fe), (j, je), (h, he)):
        in_term_order(seg, e[:, 0])                     # (the value index grows with the term: Q0, then A, then Q)
    # who owns what: a row entry its term's row; a Jacobian entry a slot of its term's row; an A value a linear entry
    row_of = np.concatenate([np.full(1 + n + nq0 + m, -1), q.ar - 1, q.qi - 1])
    assert np.array_equal(row_of[ge[:, 0]], owners(g)) and np.array_equal(row_of[je[:, 0]], lay.jrow[owners(j)] - 1)
    assert ((ge[:, 2] < 0) == (ge[:, 0] < off[5])).all() and ((je[:, 1] < 0) == (je[:, 0] < off[5])).all()
    assert ((fe[:, 0] >= off[2]) & (fe[:, 0] < off[3])).all() and (he[:, 0] >= off[2]).all()
    assert ((he[:, 1] < 0) == (he[:, 0] < off[3])).all() and np.array_equal(row_of[he[:, 0]], he[:, 1])
    q0 = out["q0"].reshape(-1, 2)
    assert len(q0) == max(nq0, 1)
    assert np.array_equal(q0[:nq0], np.c_[np.maximum(q.q0r, q.q0c) - 1, np.minimum(q.q0r, q.q0c) - 1].reshape(-1, 2))


@pytest.mark.parametrize("name", QC.CASE_NAMES)
def test_qcqp_plan_of_the_edge_and_stride_models(prog, tmp_path, name):
    cs = QC.case(name)
    for q in cs.qs:
        check_qcqp_plan(q, cs.lay, run_qcqp(prog, tmp_path, q, cs.lay))


def test_qcqp_edge_model_duplicates_and_empty_rows(prog, tmp_path):
    """What the edge model is about, on the plan itself: later copies of a duplicated COO slot and the slots no term needs get
    no entries, row 2 and variable 12 neither, the long row holds its 320 terms in term order."""
    cs = QC.case("edge-full")
    q, lay = cs.qs[0], cs.lay
    out = run_qcqp(prog, tmp_path, q, lay)
    g, f, j, h = segments(out, [lay.m, lay.n, len(lay.jrow), len(lay.hrow)])
    first = {}
    for k, key in enumerate(zip(lay.jrow.tolist(), lay.jcol.tolist())):
        if key in first or key == (7, 10):
            assert j[k + 1] == j[k], key
        first.setdefault(key, k)
    assert len(first) < len(lay.jrow)
    k54 = [k for k, key in enumerate(zip(lay.hrow.tolist(), lay.hcol.tolist())) if key == (5, 4)]
    on54 = lambda r, c: int(((np.maximum(r, c) == 5) & (np.minimum(r, c) == 4)).sum())      # Q0, the fan and some of the long row
    fed = on54(q.q0r, q.q0c) + on54(q.qr, q.qc)
    assert len(k54) == 2 and h[k54[0] + 1] - h[k54[0]] == fed > QC.EDGE_FAN and h[k54[1] + 1] == h[k54[1]]
    assert g[2] == g[1] and f[12] == f[11]
    assert g[QC.EDGE_LONG] - g[QC.EDGE_LONG - 1] == 100 + 220


def small_qcqp():
    q = make_qcqp(3, 2, 1, Q0=([1, 3], [1, 1], [2.0, 0.5]), A=([1, 2], [1, 2], [1.0, 1.0]), Q=([2], [2], [3], [1.0]))
    return q, qcqp_layout(q)


def drop(lay, which, r, c):
    rows, cols = (lay.jrow, lay.jcol) if which == "j" else (lay.hrow, lay.hcol)
    keep = ~((rows == r) & (cols == c))
    assert keep.sum() == len(rows) - 1
    return dataclasses.replace(lay, **{which + "row": rows[keep], which + "col": cols[keep]})


def test_qcqp_without_a_hessian_structure_and_with_no_terms(prog, tmp_path):
    q, lay = small_qcqp()
    noh = dataclasses.replace(lay, hrow=lay.hrow[:0], hcol=lay.hcol[:0])
    check_qcqp_plan(q, noh, run_qcqp(prog, tmp_path, q, noh))
    empty = make_qcqp(3, 2, 1)
    check_qcqp_plan(empty, noh, run_qcqp(prog, tmp_path, empty, noh, c=None, g0=None))


def test_qcqp_refusals_by_message(prog, tmp_path):
    q, lay = small_qcqp()
    who = "sqphip_qcqp_attach: "

    def msg(q=q, lay=lay, **over):
        out = run_qcqp(prog, tmp_path, q, lay, **over)
        assert out["rc"][0] == -1
        return out["err"]
    assert msg(lay=drop(lay, "j", 2, 3)) == who + "Q term 1 (2, 2, 3)" + JMISS
    assert msg(lay=drop(lay, "j", 1, 1)) == who + "A term 1 (1, 1)" + JMISS
    assert msg(lay=drop(lay, "h", 3, 1)) == who + "Q0 term 2 (3, 1)" + HMISS
    assert msg(lay=drop(lay, "h", 3, 2)) == who + "Q term 1 (2, 2, 3)" + HMISS
    assert msg(q=dataclasses.replace(q, ac=np.array([1, 4]))) == who + "A term 2 (2, 4): index out of range"
    assert msg(q=dataclasses.replace(q, qi=np.array([3]))) == who + "Q term 1 (3, 2, 3): index out of range"
    assert msg(q=dataclasses.replace(q, q0r=np.array([1, 0]))) == who + "Q0 term 2 (0, 1): index out of range"
    assert msg(lay=dataclasses.replace(lay, num_linear=2)) == who + "Q term 1 (2, 2, 3): a quadratic term in row 2, one of the num_linear = 2 linear rows"
    assert msg(nnzA=-1) == who + "negative term count"
    assert msg(qv=None) == who + "null term array"


def test_qcqp_refusals_of_the_device_tests(prog, tmp_path):
    """The models and the words of tests/test_gpu_qcqp.py test_misuse_is_refused_with_a_message"""
    q = qcqp_synth(16, 10, seed=2)
    lay = qcqp_layout(q)

    def words(q, lay, w):
        out = run_qcqp(prog, tmp_path, q, lay)
        assert out["rc"][0] == -1 and out["err"].startswith("sqphip_qcqp_attach: ") and all(x in out["err"] for x in w), out["err"]
    words(q, drop(lay, "j", q.qi[0], q.qr[0]), ["Q term 1", "Jacobian", "lacks"])
    words(q, dataclasses.replace(lay, hrow=lay.hrow[1:], hcol=lay.hcol[1:]), ["Hessian", "lacks"])
    words(q, dataclasses.replace(lay, num_linear=int(q.qi.min())), ["Q term 1", "linear rows"])
    bad = dataclasses.replace(q, ac=q.ac.copy()); bad.ac[2] = q.n + 1
    words(bad, lay, ["A term 3", "out of range"])
    check_qcqp_plan(q, lay, run_qcqp(prog, tmp_path, q, lay))


# ------------------------------------------------------------------------------------------------ the NLP builder
FLAVOURS = {"terms": ("sqphip_nlp_attach", 0, LOG, 1, 0), "affine": ("sqphip_nlp_attach_affine", 1, LOG, 1, 0),
            "general": ("sqphip_nlp_attach_general", 1, POWR, 0, 0), "data": ("sqphip_nlp_attach_data", 1, POWR, 0, 1)}


def run_nlp(prog, tmp_path, p, lay, flavour, **over):
    who, affine, last, distinct, data = FLAVOURS[flavour]
    aptr, avar, acoef = (None, p.fvar, p.fscale) if flavour == "terms" else nlp_terms_args(p)
    a = dict(structure(lay), affine=affine, last_kind=last, distinct=distinct, data=data, nterms=len(p.trow), trow=p.trow,
             tcoef=p.tcoef, tptr=p.tptr, aptr=aptr, avar=avar, acoef=acoef, fkind=p.fkind, fexp=p.fexp,
             fpar=p.fpar if affine and last == POWR else None, fshift=p.fshift, g0=p.g0, f0=float(p.f0))
    return run(prog, tmp_path, "nlp", who, **{**a, **over})


def check_nlp_plan(p, lay, out, flavour):
    assert out["rc"][0] == 0, out.get("err")
    n, m, nnzJ, nnzH = lay.n, lay.m, len(lay.jrow), len(lay.hrow)
    aptr, avar, acoef = nlp_terms_args(p)
    nterms, nfac, nargs = len(p.trow), len(p.fkind), len(avar)
    data, powr = flavour == "data", bool((p.fkind == POWR).any())
    sc = lambda k: int(out[k][0])
    assert (sc("n"), sc("m"), sc("nterms"), sc("nfac"), sc("nargs"), sc("data")) == (n, m, nterms, nfac, nargs, int(data))
    ob = 1 + m + nterms
    nvals = ob + (nfac + nargs + (nfac if powr else 0) if data else 0)
    assert (sc("ob"), sc("oa"), sc("op"), sc("end")) == (ob, ob + nfac, ob + nfac + nargs if powr else -1, nvals)
    nv = sc("nv")
    assert nv % 2 == 0 and nvals <= nv <= nvals + 1 and len(out["base"]) == nv and sc("ws") == 3 * nfac
    want = [[p.f0], p.g0, p.tcoef] + ([p.fshift, acoef] + ([p.fpar] if powr else []) if data else [])
    assert np.array_equal(out["base"][:nvals], np.concatenate(want)) and not out["base"][nvals:].any()
    assert np.array_equal(out["tptr"], p.tptr) and np.array_equal(out["aptr"], aptr) and np.array_equal(out["kind"], p.fkind)
    assert np.array_equal(out["avar"][:nargs], avar - 1) and np.array_equal(out["acoef"][:nargs], acoef)
    one = np.diff(aptr) == 1
    assert np.array_equal(out["fvar"][:nfac], np.where(one, avar[aptr[:-1]] - 1, -1)) and sc("multi") == int((~one).any())
    e = np.where(p.fkind == POW, p.fexp, 1)
    assert np.array_equal(out["fke"][:nfac], p.fkind + 16 * (e + 32))
    assert np.array_equal(out["lin_terms"], np.flatnonzero((p.trow >= 1) & (p.trow <= p.num_linear)))
    obj = np.flatnonzero(p.trow == 0)
    assert sc("nobj") == len(obj) and np.array_equal(out["ot"][:len(obj)], obj) and len(out["ot"]) == max(len(obj), 1)
    g, f, j, h = segments(out, [m, n, nnzJ, nnzH])
    # the counts, from the term lists: a term of a row is one row entry; every argument of a term one gradient or Jacobian
    # entry; the Hessian holds one entry per unordered pair of (factor, argument) couples of a term -- a couple with itself
    # and two couples of one factor only when the factor is curved (not POW with e = 1) -- and both ordered pairs where two
    # couples of different factors sit on one variable
    targs = [range(aptr[p.tptr[t]], aptr[p.tptr[t + 1]]) for t in range(nterms)]
    fac_of = np.repeat(np.arange(nfac), np.diff(aptr))
    curved = ~((p.fkind == POW) & (p.fexp == 1))
    nh = 0
    for t in range(nterms):
        for b in targs[t]:
            for a in range(targs[t][0], b + 1):
                if fac_of[a] == fac_of[b] and not curved[fac_of[b]]:
                    continue
                nh += 2 if (a != b and avar[a] == avar[b]) else 1
    assert g[-1] == int((p.trow > 0).sum())
    assert f[-1] == sum(len(targs[t]) for t in obj) and j[-1] == nargs - f[-1]
    assert h[-1] == (nh if nnzH else 0)
    ge, fe, je, he = entries(out, "ge", 1, g), entries(out, "fe", 2, f), entries(out, "je", 2, j), entries(out, "he", 4, h)
    for seg, e in ((g, ge), (f, fe), (j, je), (h, he)):
        assert ((e[:, 0] >= 0) & (e[:, 0] < nterms)).all()
        in_term_order(seg, e[:, 0])
    assert np.array_equal(p.trow[ge[:, 0]] - 1, owners(g))

    def couple(t, ent):
        """the argument a plan entry names; its factor bits must be the argument's factor within the term"""
        arg, kf = ent & ARG, ent >> 28
        assert ((arg >= 0) & (arg < nargs)).all() and np.array_equal(fac_of[arg], p.tptr[t] + kf)
        return arg
    assert np.array_equal(avar[couple(fe[:, 0], fe[:, 1])] - 1, owners(f)) and (p.trow[fe[:, 0]] == 0).all()
    ja = couple(je[:, 0], je[:, 1])
    assert np.array_equal(lay.jrow[owners(j)], p.trow[je[:, 0]]) and np.array_equal(lay.jcol[owners(j)], avar[ja])
    ha, hb = couple(he[:, 0], he[:, 1]), couple(he[:, 0], he[:, 2])
    assert np.array_equal(he[:, 3], p.trow[he[:, 0]] - 1) and ((he[:, 3] >= -1) & (he[:, 3] < m)).all()
    ho = owners(h)
    assert np.array_equal(lay.hrow[ho], np.maximum(avar[ha], avar[hb])) and np.array_equal(lay.hcol[ho], np.minimum(avar[ha], avar[hb]))


NLP_MODELS = {"terms": lambda: nlp_terms_synth(16, 10, seed=2), "affine": lambda: nlp_affine_synth(16, 10, seed=2),
              "general": lambda: nlp_general_synth(16, 10, seed=2),
              "data": lambda: cobb_douglas_model([0.2, 0.3, 0.4], [1.0, 2.0, 0.5], 10.0)}


@pytest.mark.parametrize("flavour", list(NLP_MODELS))
def test_nlp_plan_of_every_attach_flavour(prog, tmp_path, flavour):
    p = NLP_MODELS[flavour]()
    lay = nlp_terms_layout(p)
    check_nlp_plan(p, lay, run_nlp(prog, tmp_path, p, lay, flavour), flavour)
    if flavour in ("terms", "affine"):                   # a model of the older calls files the same plan through the general one
        a, b = run_nlp(prog, tmp_path, p, lay, flavour), run_nlp(prog, tmp_path, p, lay, "general")
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    noh = dataclasses.replace(lay, hrow=lay.hrow[:0], hcol=lay.hcol[:0])
    check_nlp_plan(p, noh, run_nlp(prog, tmp_path, p, noh, flavour), flavour)


def test_nlp_data_checks_of_an_instance(prog, tmp_path):
    """nlp_data_check on the plan of four consumers' model: the words of tests/test_gpu_nlp_data.py and the whole messages"""
    p = cobb_douglas_model([0.2, 0.3, 0.4], [1.0, 2.0, 0.5], 10.0)
    lay = nlp_terms_layout(p)
    who = "sqphip_nlp_set_instance_data"
    _, _, acoef = nlp_terms_args(p)

    def chk(flavour="data", **k):
        out = run_nlp(prog, tmp_path, p, lay, flavour, check=1, **{"chk_" + n: k.get(n) for n in ("fshift", "acoef", "fpar")})
        assert out["rc"][0] == 0
        return out["check"].replace("sqphip_nlp_attach_" + flavour, who)      # (the program checks under the attach's name)
    assert chk() == "" and chk(fshift=p.fshift, acoef=acoef, fpar=p.fpar) == ""
    par = p.fpar.copy(); par[1] = 0.0
    assert chk(fpar=par) == who + ": term 1 factor 2: real exponent 0.000000 (finite and not 0)"
    lin = who + ": term 2 factor 1: the term is in one of the num_linear = 1 linear rows: coefficient 1 and shift 0 only"
    ac = acoef.copy(); ac[3] = 2.0
    assert chk(acoef=ac) == lin
    sh = p.fshift.copy(); sh[3] = 0.1
    assert chk(fshift=sh) == lin
    assert chk("general") == who + ": the data of this context is shared by the batch (attach with sqphip_nlp_attach_data)"


def small_nlp(**over):
    terms = [(0, 1.0, [(1, POW, 2)]), (1, 1.0, [(2, POW)]), (2, 2.0, [(1, SIN), (3, EXP)])]
    p = make_nlp_terms(3, 2, 1, terms)
    return p, nlp_terms_layout(p)


def test_nlp_refusals_by_message(prog, tmp_path):
    p, lay = small_nlp()
    who = "sqphip_nlp_attach: "
    check_nlp_plan(p, lay, run_nlp(prog, tmp_path, p, lay, "terms"), "terms")

    def msg(p=p, lay=lay, flavour="terms", **over):
        out = run_nlp(prog, tmp_path, p, lay, flavour, **over)
        assert out["rc"][0] == -1
        return out["err"]

    def put(name, k, v):
        a = getattr(p, name).copy(); a[k] = v
        return dataclasses.replace(p, **{name: a})
    assert msg(lay=drop(lay, "j", 2, 3)) == who + "term 3 factor 2: needs the Jacobian entry (2, 3) that the structure of sqphip_create lacks"
    assert msg(lay=drop(lay, "h", 3, 1)) == who + "term 3 factor 2: needs the Hessian entry (3, 1) that the structure of sqphip_create lacks"
    assert msg(p=put("fvar", 0, 4)) == who + "term 1 factor 1: variable 4 out of range"
    assert msg(p=put("fvar", 3, 0)) == who + "term 3 factor 2: variable 0 out of range"
    assert msg(p=put("trow", 2, 3)) == who + "term 3: row 3 out of range (0: objective, 1..2)"
    assert msg(lay=dataclasses.replace(lay, num_linear=2)) == who + ("term 3 factor 1: row 2 is one of the num_linear = 2 linear rows: "
                                                                    "a single POW factor with e = 1, a = 1, b = 0 only")
    assert msg(flavour="affine", lay=dataclasses.replace(lay, num_linear=2)) == (
        "sqphip_nlp_attach_affine: term 3 factor 1: row 2 is one of the num_linear = 2 linear rows: "
        "a single POW factor with e = 1, one argument with coefficient 1, shift 0 only")
    assert msg(p=put("fkind", 0, LOG + 1)) == who + "term 1 factor 1: unknown kind 5"
    assert msg(p=put("fexp", 0, 33)) == who + "term 1 factor 1: exponent 33 (1 <= |e| <= 32)"
    assert msg(p=put("fvar", 3, 1)) == who + "term 3 factor 2: variable 1 twice in one term (write x^2)"
    assert msg(tptr=None) == who + "null term array"
    nine = make_nlp_terms(9, 1, 0, [(1, 1.0, [(v, COS) for v in range(1, 10)])])
    assert msg(p=nine, lay=nlp_terms_layout(nine)) == who + "term 1: more than 8 factors"
    pw = make_nlp_terms(2, 1, 0, [(1, 1.0, [(1, POWR, 0.5), (2, POW)])])
    assert msg(p=pw, lay=nlp_terms_layout(pw), flavour="general", fpar=None) == (
        "sqphip_nlp_attach_general: term 1 factor 1: a POWR factor needs its real exponent: fpar is null")
    assert msg(p=pw, lay=nlp_terms_layout(pw), flavour="affine") == "sqphip_nlp_attach_affine: term 1 factor 1: unknown kind 10"


def test_nlp_refusals_of_the_device_tests(prog, tmp_path):
    """The model and the words of tests/test_gpu_nlp.py (the misuse test)"""
    p = nlp_terms_synth(16, 10, seed=2)
    lay = nlp_terms_layout(p)
    t = int(np.flatnonzero((p.trow > p.num_linear) & (np.diff(p.tptr) >= 2))[0])
    k, T = int(p.tptr[t]), f"term {t + 1}"
    for name, at, v, w in (("fvar", k, p.n + 1, [T, "factor 1", "out of range"]), ("trow", t, p.m + 1, [T, "out of range"]),
                           ("fvar", k, 0, [T, "out of range"])):
        a = getattr(p, name).copy(); a[at] = v
        out = run_nlp(prog, tmp_path, dataclasses.replace(p, **{name: a}), lay, "terms")
        assert out["rc"][0] == -1 and out["err"].startswith("sqphip_nlp_attach: ") and all(x in out["err"] for x in w), out["err"]


# ------------------------------------------------------------------------------------------------ the columns of a block
def test_block_columns_with_and_without_a_hessian_structure(prog, tmp_path):
    n, cols = 7, np.array([6, 2, 7, 1, 4])
    r, c = np.tril_indices(5)
    hrow, hcol = np.maximum(cols[r], cols[c]), np.minimum(cols[r], cols[c])
    order = np.random.default_rng(3).permutation(len(hrow))
    hrow, hcol = np.r_[hrow[order], 6, 3], np.r_[hcol[order], 6, 3]                 # a second copy of (6, 6); a slot no block needs
    out = run(prog, tmp_path, "block", "x", n=n, hrow=hrow, hcol=hcol, cols=cols)
    assert out["rc"][0] == 0 and np.array_equal(out["cv"], cols - 1)
    hs = out["hs"]
    assert len(hs) == 15 and np.array_equal(hs, np.argsort(order)) and hs[0] == int(np.flatnonzero(order == 0)[0])
    for k, (a, b) in enumerate(zip(r, c)):                                          # entry (a, b) at a (a + 1) / 2 + b
        assert k == a * (a + 1) // 2 + b and (hrow[hs[k]], hcol[hs[k]]) == (max(cols[a], cols[b]), min(cols[a], cols[b]))
    out = run(prog, tmp_path, "block", "x", n=n, hrow=hrow[:0], hcol=hcol[:0], cols=cols)
    assert out["rc"][0] == 0 and np.array_equal(out["cv"], cols - 1) and np.array_equal(out["hs"], np.full(15, -1))
    keep = ~((hrow == 7) & (hcol == 2))
    out = run(prog, tmp_path, "block", "x", n=n, hrow=hrow[keep], hcol=hcol[keep], cols=cols)
    assert out["err"] == "entry (3, 2) needs the Hessian entry (7, 2) that the structure of sqphip_create lacks"
    # the words of tests/test_gpu_nlp_block.py and tests/test_gpu_nlp_softmax.py
    assert run(prog, tmp_path, "block", "x", n=6, hrow=hrow[:0], hcol=hcol[:0], cols=[2, 7, 5])["err"] == "column 2: variable 7 out of range"
    assert run(prog, tmp_path, "block", "x", n=7, hrow=hrow[:0], hcol=hcol[:0], cols=[2, 5, 2])["err"] == "column 3: variable 2 twice (columns 1 and 3)"
