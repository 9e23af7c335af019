// model_plans.cpp -- see model_plans.hpp
#include "model_plans.hpp"
#include "../../include/sqphip.h"
#include <algorithm>
#include <cmath>

namespace sqphip {

StructureSlots::StructureSlots(int64_t n_, int64_t nnzJ_, const int64_t *jrow, const int64_t *jcol, int64_t nnzH_,
                               const int64_t *hrow, const int64_t *hcol) : n(n_), nnzJ(nnzJ_), nnzH(nnzH_)
{
    for (int64_t k = nnzJ - 1; k >= 0; --k) jslot[(jrow[k] - 1) * n + (jcol[k] - 1)] = (int)k;
    for (int64_t k = nnzH - 1; k >= 0; --k) {
        const int64_t r = hrow[k] - 1, c = hcol[k] - 1;
        hslot[std::max(r, c) * n + std::min(r, c)] = (int)k;
    }
}

void csr_by_owner(int owners, const std::vector<int> &own, std::vector<int> &ptr, std::vector<int> &ord)
{
    ptr.assign(owners + 1, 0);
    for (int o : own) ptr[o + 1]++;
    for (int r = 0; r < owners; ++r) ptr[r + 1] += ptr[r];
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    ord.assign(own.size(), 0);
    for (size_t e = 0; e < own.size(); ++e) ord[fill[own[e]]++] = (int)e;
}

std::vector<int> pack_ptrs(const std::vector<int> &g, const std::vector<int> &f, const std::vector<int> &j, const std::vector<int> &h,
                           int &fp, int &jp, int &hp)
{
    std::vector<int> ptr(g);
    fp = (int)ptr.size(); ptr.insert(ptr.end(), f.begin(), f.end());
    jp = (int)ptr.size(); ptr.insert(ptr.end(), j.begin(), j.end());
    hp = (int)ptr.size(); ptr.insert(ptr.end(), h.begin(), h.end());
    return ptr;
}

namespace {

// the entries of a plan (w ints each, in production order) as CSR by owner, the entries of one owner kept in that order;
// an empty plan keeps one entry of zeros
std::vector<int> plan_csr(int owners, const std::vector<int> &own, const std::vector<int> &e, int w, std::vector<int> &ptr)
{
    std::vector<int> ord;
    csr_by_owner(owners, own, ptr, ord);
    std::vector<int> out(std::max<size_t>(ord.size(), 1) * w, 0);
    for (size_t k = 0; k < ord.size(); ++k) std::copy(e.begin() + (size_t)ord[k] * w, e.begin() + ((size_t)ord[k] + 1) * w, out.begin() + k * w);
    return out;
}

void push(std::vector<int> &v, std::initializer_list<int> e) { v.insert(v.end(), e); }

std::string qcqp_term(const char *kind, int64_t t, int64_t a, int64_t b, int64_t c = 0)
{
    std::string s = std::string(kind) + " term " + std::to_string(t) + " (" + std::to_string(a) + ", " + std::to_string(b);
    if (c) s += ", " + std::to_string(c);
    return s + ")";
}

std::string nlp_term(const char *who, int64_t t, int64_t k, const std::string &msg)
{
    return std::string(who) + ": term " + std::to_string(t + 1) + (k >= 0 ? " factor " + std::to_string(k + 1) : std::string()) + ": " + msg;
}

}  // namespace

int build_qcqp_plan(const StructureSlots &S, int64_t m, int64_t nlin, const char *who, int64_t nnzQ0, const int64_t *q0r,
                    const int64_t *q0c, const double *q0v, int64_t nnzA, const int64_t *ar, const int64_t *ac, const double *av,
                    int64_t nnzQ, const int64_t *qi, const int64_t *qr, const int64_t *qc, const double *qv, const double *c,
                    const double *g0, double f0, QcqpPlan &P, std::string &err)
{
    auto fail = [&](const std::string &msg) { err = std::string(who) + ": " + msg; return (int)SQPHIP_EINVAL; };
    if (nnzQ0 < 0 || nnzA < 0 || nnzQ < 0) return fail("negative term count");
    if ((nnzQ0 > 0 && (!q0r || !q0c || !q0v)) || (nnzA > 0 && (!ar || !ac || !av)) ||
        (nnzQ > 0 && (!qi || !qr || !qc || !qv))) return fail("null term array");
    const int64_t n = S.n, nnzH = S.nnzH;
    const std::string jmiss = " needs a Jacobian entry that the structure of sqphip_create lacks",
                      hmiss = " needs a Hessian entry that the structure of sqphip_create lacks";
    // values of an instance: f0 | c | Q0 | g0 | A | Q; the stride padded to even
    QcqpHost &Hh = P.host;
    long *off = Hh.off;
    off[0] = 0; off[1] = 1; off[2] = off[1] + n; off[3] = off[2] + nnzQ0; off[4] = off[3] + m; off[5] = off[4] + nnzA; off[6] = off[5] + nnzQ;
    Hh.nv = (off[6] + 1) & ~1L;
    if (Hh.nv > INT32_MAX) return fail("too many values per instance");
    const int off_q0 = (int)off[2], off_a = (int)off[4], off_q = (int)off[5];
    std::vector<int> g_own, g_e, f_own, f_e, j_own, j_e, h_own, h_e;
    for (int64_t t = 0; t < nnzQ0; ++t) {
        const int64_t r = q0r[t] - 1, cc = q0c[t] - 1;
        if (r < 0 || r >= n || cc < 0 || cc >= n) return fail(qcqp_term("Q0", t + 1, q0r[t], q0c[t]) + ": index out of range");
        const int hs = S.hfind(r, cc);
        if (nnzH > 0 && hs < 0) return fail(qcqp_term("Q0", t + 1, q0r[t], q0c[t]) + hmiss);
        const int v = off_q0 + (int)t;
        f_own.push_back((int)r); push(f_e, {v, (int)cc});
        if (r != cc) { f_own.push_back((int)cc); push(f_e, {v, (int)r}); }
        if (hs >= 0) { h_own.push_back(hs); push(h_e, {v, -1}); }
    }
    for (int64_t t = 0; t < nnzA; ++t) {
        const int64_t i = ar[t] - 1, j = ac[t] - 1;
        if (i < 0 || i >= m || j < 0 || j >= n) return fail(qcqp_term("A", t + 1, ar[t], ac[t]) + ": index out of range");
        const int js = S.jfind(i, j);
        if (js < 0) return fail(qcqp_term("A", t + 1, ar[t], ac[t]) + jmiss);
        const int v = off_a + (int)t;
        g_own.push_back((int)i); push(g_e, {v, (int)j, -1, 0});      // (value, variable, second variable or -1: linear, 0)
        j_own.push_back(js); push(j_e, {v, -1});
    }
    for (int64_t t = 0; t < nnzQ; ++t) {
        const int64_t i = qi[t] - 1, r = qr[t] - 1, cc = qc[t] - 1;
        const std::string what = qcqp_term("Q", t + 1, qi[t], qr[t], qc[t]);
        if (i < 0 || i >= m || r < 0 || r >= n || cc < 0 || cc >= n) return fail(what + ": index out of range");
        if (i < nlin) return fail(what + ": a quadratic term in row " + std::to_string(i + 1) +
                                  ", one of the num_linear = " + std::to_string(nlin) + " linear rows");
        const int jr = S.jfind(i, r), jc = S.jfind(i, cc), hs = S.hfind(r, cc);
        if (jr < 0 || jc < 0) return fail(what + jmiss);
        if (nnzH > 0 && hs < 0) return fail(what + hmiss);
        const int v = off_q + (int)t;
        g_own.push_back((int)i); push(g_e, {v, (int)r, (int)cc, 0});
        j_own.push_back(jr); push(j_e, {v, (int)cc});
        if (r != cc) { j_own.push_back(jc); push(j_e, {v, (int)r}); }
        if (hs >= 0) { h_own.push_back(hs); push(h_e, {v, (int)i}); }
    }
    std::vector<int> g_ptr, f_ptr, j_ptr, h_ptr;
    P.ge = plan_csr((int)m, g_own, g_e, 4, g_ptr);
    if (g_own.empty()) P.ge[2] = -1;
    P.fe = plan_csr((int)n, f_own, f_e, 2, f_ptr);
    P.je = plan_csr((int)S.nnzJ, j_own, j_e, 2, j_ptr);
    P.he = plan_csr((int)nnzH, h_own, h_e, 2, h_ptr);
    P.ptr = pack_ptrs(g_ptr, f_ptr, j_ptr, h_ptr, P.f_ptr, P.j_ptr, P.h_ptr);
    P.n = (int)n; P.m = (int)m; P.nq0 = (int)nnzQ0;
    P.q0.assign(2 * (size_t)std::max<int64_t>(nnzQ0, 1), 0);     // the Q0 terms, 0-based, folded into the lower triangle
    for (int64_t t = 0; t < nnzQ0; ++t) { P.q0[2 * t] = (int)std::max(q0r[t], q0c[t]) - 1; P.q0[2 * t + 1] = (int)std::min(q0r[t], q0c[t]) - 1; }
    std::vector<double> &val0 = Hh.base;
    val0.assign(Hh.nv, 0.0);
    val0[0] = f0;
    if (c) std::copy(c, c + n, val0.begin() + off[1]);
    if (nnzQ0) std::copy(q0v, q0v + nnzQ0, val0.begin() + off[2]);
    if (g0) std::copy(g0, g0 + m, val0.begin() + off[3]);
    if (nnzA) std::copy(av, av + nnzA, val0.begin() + off[4]);
    if (nnzQ) std::copy(qv, qv + nnzQ, val0.begin() + off[5]);
    return SQPHIP_OK;
}

int build_nlp_plan(const StructureSlots &S, int64_t m, int64_t nlin, const char *who, const NlpOptions &O, int64_t nterms,
                   const int64_t *trow, const double *tcoef, const int64_t *tptr, const int64_t *aptr, const int64_t *avar,
                   const double *acoef, const int32_t *fkind, const int32_t *fexp, const double *fpar, const double *fshift,
                   const double *g0, double f0, NlpPlan &P, std::string &err)
{
    const bool affine = O.affine;
    auto fail = [&](const char *msg) { err = std::string(who) + ": " + msg; return (int)SQPHIP_EINVAL; };
    auto tfail = [&](int64_t t, int64_t k, const std::string &msg) { err = nlp_term(who, t, k, msg); return (int)SQPHIP_EINVAL; };
    if (affine && !aptr) return fail("null aptr");
    if (nterms < 0) return fail("negative term count");
    if (!tptr || (nterms > 0 && (!trow || !tcoef))) return fail("null term array");
    if (tptr[0] != 0) return fail("tptr[0] must be 0");
    for (int64_t t = 0; t < nterms; ++t)
        if (tptr[t + 1] < tptr[t]) return tfail(t, -1, "tptr decreases");
    const int64_t nfac = tptr[nterms];
    if (nfac > 0 && (!avar || !fkind || !fexp)) return fail("null factor array");
    if (nfac > (1 << 28) || nterms > (1 << 28)) return fail("too many terms");
    if (affine) {
        if (aptr[0] != 0) return fail("aptr[0] must be 0");
        for (int64_t t = 0; t < nterms; ++t)
            for (int64_t k = tptr[t]; k < tptr[t + 1]; ++k) {
                if (aptr[k + 1] < aptr[k]) return tfail(t, k - tptr[t], "aptr decreases");
                if (aptr[k + 1] == aptr[k]) return tfail(t, k - tptr[t], "no arguments");
                if (aptr[k + 1] - aptr[k] > 8) return tfail(t, k - tptr[t], "more than 8 arguments");
            }
    }
    const int64_t nargs = affine ? aptr[nfac] : nfac;
    if (nargs > (1 << 28)) return fail("too many arguments");
    auto a0 = [&](int64_t k) { return affine ? aptr[k] : k; };
    const int64_t n = S.n, nnzH = S.nnzH;
    NlpHost &Hh = P.host;
    std::vector<int> g_own, g_t, f_own, f_e, j_own, j_e, h_own, h_e;
    std::vector<int> &fke = P.fke, &fv = P.fvar, &ap = Hh.aptr, &av = P.avar, &ot = P.ot;
    std::vector<double> &fab = P.fab, &ac = P.acoef, &aw = P.aw, &fpw = P.fpar;
    // A one-argument factor keeps its coefficient in pass 1 (fab, chain factors folded into phi', phi'') and weight 1.0 in the
    // plans; a factor of several arguments stores kappa', kappa'' and its arguments weigh a_v (nlp_dev.hpp).
    fke.assign((size_t)std::max<int64_t>(nfac, 1), 0); fv.assign(fke.size(), 0);
    fab.assign(2 * fke.size(), 0.0);
    for (size_t k = 0; k < fke.size(); ++k) fab[2 * k] = 1.0;
    ap.assign((size_t)nfac + 1, 0); av.assign((size_t)std::max<int64_t>(nargs, 1), 0);
    ac.assign(av.size(), 1.0); aw.assign(av.size(), 1.0); fpw.assign(fke.size(), 0.0);
    ot.clear(); Hh.lin_terms.clear();
    bool multi = false, powr = false;
    for (int64_t t = 0; t < nterms; ++t) {
        const int64_t i = trow[t], k0 = tptr[t], k1 = tptr[t + 1];
        if (i < 0 || i > m) return tfail(t, -1, "row " + std::to_string(i) + " out of range (0: objective, 1.." + std::to_string(m) + ")");
        if (k1 == k0) return tfail(t, -1, "no factors (a constant belongs in f0 / g0)");
        if (k1 - k0 > 8) return tfail(t, -1, "more than 8 factors");
        bool plain[8];
        for (int64_t k = k0; k < k1; ++k) {
            const int64_t kf = k - k0, j0 = a0(k), j1 = a0(k + 1);
            const double b = fshift ? fshift[k] : 0.0;
            for (int64_t j = j0; j < j1; ++j)
                if (avar[j] < 1 || avar[j] > n) return tfail(t, kf, "variable " + std::to_string(avar[j]) + " out of range");
            if (fkind[k] < NLP_POW || fkind[k] > O.last_kind) return tfail(t, kf, "unknown kind " + std::to_string(fkind[k]));
            if (fkind[k] == NLP_POWR) {
                if (!fpar) return tfail(t, kf, "a POWR factor needs its real exponent: fpar is null");
                if (!std::isfinite(fpar[k]) || fpar[k] == 0.0)
                    return tfail(t, kf, "real exponent " + std::to_string(fpar[k]) + " (finite and not 0)");
                fpw[k] = fpar[k];
                powr = true;
            }
            const int e = fkind[k] == NLP_POW ? fexp[k] : 1;
            if (e == 0 || e > 32 || e < -32) return tfail(t, kf, "exponent " + std::to_string(e) + " (1 <= |e| <= 32)");
            for (int64_t j = j0; j < j1; ++j) {
                for (int64_t j2 = j0; j2 < j; ++j2)
                    if (avar[j2] == avar[j]) return tfail(t, kf, "variable " + std::to_string(avar[j]) + " twice in one factor (add the coefficients)");
                for (int64_t j2 = a0(k0); O.distinct && j2 < j0; ++j2)
                    if (avar[j2] == avar[j]) return tfail(t, kf, "variable " + std::to_string(avar[j]) + " twice in one term (write x^2)");
            }
            plain[kf] = fkind[k] == NLP_POW && e == 1;
            const bool one = j1 - j0 == 1;
            multi = multi || !one;
            const double a = one && acoef ? acoef[j0] : 1.0;
            if (i >= 1 && i <= nlin && !(k1 - k0 == 1 && one && plain[kf] && a == 1.0 && b == 0.0))
                return tfail(t, kf, "row " + std::to_string(i) + " is one of the num_linear = " + std::to_string(nlin) +
                                    (affine ? " linear rows: a single POW factor with e = 1, one argument with coefficient 1, shift 0 only"
                                            : " linear rows: a single POW factor with e = 1, a = 1, b = 0 only"));
            fv[k] = one ? (int)avar[j0] - 1 : -1; fke[k] = fkind[k] + (e + 32) * (1 << NLP_KIND_BITS); fab[2 * k] = a; fab[2 * k + 1] = b;
            ap[k] = (int)j0; ap[k + 1] = (int)j1;
            for (int64_t j = j0; j < j1; ++j) {
                av[j] = (int)avar[j] - 1; ac[j] = acoef ? acoef[j] : 1.0; aw[j] = one ? 1.0 : ac[j];
            }
        }
        if (i >= 1 && i <= nlin) Hh.lin_terms.push_back((int)t);
        if (i == 0) ot.push_back((int)t); else { g_own.push_back((int)i - 1); g_t.push_back((int)t); }
        // a plan entry names an argument and, in the bits above 2^28, its factor within the term
        auto ent = [&](int64_t k, int64_t j) { return (int)(j | ((k - k0) << 28)); };
        for (int64_t k = k0; k < k1; ++k)
            for (int64_t j = a0(k); j < a0(k + 1); ++j) {
                if (i == 0) { f_own.push_back(av[j]); push(f_e, {(int)t, ent(k, j)}); continue; }
                const int js = S.jfind(i - 1, av[j]);
                if (js < 0) return tfail(t, k - k0, "needs the Jacobian entry (" + std::to_string(i) + ", " + std::to_string(avar[j]) +
                                                    ") that the structure of sqphip_create lacks");
                j_own.push_back(js); push(j_e, {(int)t, ent(k, j)});
            }
        if (nnzH > 0)
            for (int64_t k = k0; k < k1; ++k)
                for (int64_t j = a0(k); j < a0(k + 1); ++j)
                    for (int64_t k2 = k0; k2 <= k; ++k2) {
                        if (k2 == k && plain[k - k0]) continue;            // phi'' = 0
                        for (int64_t j2 = a0(k2); j2 < (k2 == k ? j + 1 : a0(k2 + 1)); ++j2) {
                            const int hs = S.hfind(av[j], av[j2]);
                            if (hs < 0) return tfail(t, k - k0, "needs the Hessian entry (" + std::to_string(std::max(avar[j], avar[j2])) + ", " +
                                                                std::to_string(std::min(avar[j], avar[j2])) + ") that the structure of sqphip_create lacks");
                            // two arguments on one variable (shared variables only: different factors): both ordered pairs count
                            for (int c = (j2 != j && av[j2] == av[j]) ? 2 : 1; c > 0; --c) {
                                h_own.push_back(hs); push(h_e, {(int)t, ent(k2, j2), ent(k, j), (int)i - 1});
                            }
                        }
                    }
    }
    // CSR by owner, the entries of one owner kept in production (term) order
    std::vector<int> g_ptr, f_ptr, j_ptr, h_ptr;
    P.ge = plan_csr((int)m, g_own, g_t, 1, g_ptr);
    P.fe = plan_csr((int)n, f_own, f_e, 2, f_ptr);
    P.je = plan_csr((int)S.nnzJ, j_own, j_e, 2, j_ptr);
    P.he = plan_csr((int)nnzH, h_own, h_e, 4, h_ptr);
    P.ptr = pack_ptrs(g_ptr, f_ptr, j_ptr, h_ptr, P.f_ptr, P.j_ptr, P.h_ptr);
    Hh.tptr.resize((size_t)nterms + 1);
    for (int64_t t = 0; t <= nterms; ++t) Hh.tptr[t] = (int)tptr[t];
    Hh.kind.assign(fkind, fkind + nfac);
    // values of an instance: f0 | g0 | c, the stride padded to even: every block is 16-byte aligned, as the QCQP blocks are;
    // data: f0 | g0 | c | b [nfac] | a [nargs] | p [nfac, with a POWR factor only]
    const long ob = 1 + (long)m + nterms, oa = ob + nfac, op = powr ? oa + nargs : -1;
    const long nvals = O.data ? oa + nargs + (powr ? nfac : 0) : ob, nv = (nvals + 1) & ~1L;
    if (nv > INT32_MAX) return fail("too many values per instance");
    std::vector<double> &val0 = Hh.base;
    val0.assign(nv, 0.0);
    val0[0] = f0;
    if (g0) std::copy(g0, g0 + m, val0.begin() + 1);
    if (nterms) std::copy(tcoef, tcoef + nterms, val0.begin() + 1 + m);
    if (O.data) {
        for (int64_t k = 0; k < nfac; ++k) val0[ob + k] = fab[2 * k + 1];
        std::copy(ac.begin(), ac.begin() + nargs, val0.begin() + oa);
        if (powr) std::copy(fpw.begin(), fpw.begin() + nfac, val0.begin() + op);
    }
    P.n = (int)n; P.m = (int)m; P.multi = multi ? 1 : 0;
    P.nobj = (int)ot.size();
    if (ot.empty()) ot.push_back(0);
    Hh.nv = nv; Hh.nfac = nfac; Hh.nterms = nterms; Hh.nargs = nargs;
    Hh.end = nvals; Hh.ws = 3 * nfac; Hh.blk.clear(); Hh.started = false;
    Hh.data = O.data; Hh.ob = ob; Hh.oa = oa; Hh.op = op;
    return SQPHIP_OK;
}

std::string nlp_data_check(const NlpHost &H, int64_t nlin, const char *who, const double *fshift, const double *acoef, const double *fpar)
{
    if (!H.data) return std::string(who) + ": the data of this context is shared by the batch (attach with sqphip_nlp_attach_data)";
    if (fpar && H.op < 0) return std::string(who) + ": fpar given, but the model has no POWR factor";
    if (fpar)
        for (long t = 0; t < H.nterms; ++t)
            for (int k = H.tptr[t]; k < H.tptr[t + 1]; ++k)
                if (H.kind[k] == NLP_POWR && (!std::isfinite(fpar[k]) || fpar[k] == 0.0))
                    return nlp_term(who, t, k - H.tptr[t], "real exponent " + std::to_string(fpar[k]) + " (finite and not 0)");
    for (int t : H.lin_terms) {
        const int k = H.tptr[t];              // (the attach made sure: one factor, one argument)
        if ((acoef && acoef[H.aptr[k]] != 1.0) || (fshift && fshift[k] != 0.0))
            return nlp_term(who, t, 0, "the term is in one of the num_linear = " + std::to_string(nlin) + " linear rows: coefficient 1 and shift 0 only");
    }
    return "";
}

std::string nlp_block_columns(const StructureSlots &S, int D, const int64_t *cols, std::vector<int> &cv, std::vector<int> &hs)
{
    for (int j = 0; j < D; ++j) {
        if (cols[j] < 1 || cols[j] > S.n) return "column " + std::to_string(j + 1) + ": variable " + std::to_string(cols[j]) + " out of range";
        for (int j2 = 0; j2 < j; ++j2)
            if (cols[j2] == cols[j]) return "column " + std::to_string(j + 1) + ": variable " + std::to_string(cols[j]) + " twice (columns " +
                                            std::to_string(j2 + 1) + " and " + std::to_string(j + 1) + ")";
    }
    hs.assign((size_t)D * (D + 1) / 2, -1); cv.resize(D);
    for (int j = 0; j < D; ++j) cv[j] = (int)cols[j] - 1;
    for (int r = 0; S.nnzH > 0 && r < D; ++r)
        for (int c = 0; c <= r; ++c) {
            const int64_t vr = std::max(cv[r], cv[c]), vc = std::min(cv[r], cv[c]);
            if ((hs[(size_t)r * (r + 1) / 2 + c] = S.hfind(vr, vc)) < 0)
                return "entry (" + std::to_string(r + 1) + ", " + std::to_string(c + 1) + ") needs the Hessian entry (" + std::to_string(vr + 1) +
                       ", " + std::to_string(vc + 1) + ") that the structure of sqphip_create lacks";
        }
    return "";
}

std::string nlp_block_rows(const StructureSlots &S, int64_t m, int64_t nlin, int R, const int64_t *rows, const std::vector<int> &cv,
                           int *row, std::vector<int> &js)
{
    const int d = (int)cv.size();
    js.assign((size_t)R * d, -1);
    for (int r = 0; r < R; ++r) {
        const std::string out = "output " + std::to_string(r + 1) + ": row " + std::to_string(rows[r]);
        if (rows[r] < 0 || rows[r] > m) return out + " outside 0.." + std::to_string(m);
        for (int r2 = 0; r2 < r; ++r2)
            if (rows[r2] == rows[r]) return out + " twice (outputs " + std::to_string(r2 + 1) + " and " + std::to_string(r + 1) + ")";
        if (rows[r] >= 1 && rows[r] <= nlin) return out + " is one of the num_linear = " + std::to_string(nlin) + " linear rows";
        row[r] = (int)rows[r];
        for (int j = 0; rows[r] >= 1 && j < d; ++j)
            if ((js[(size_t)r * d + j] = S.jfind(rows[r] - 1, cv[j])) < 0)
                return out + ", column " + std::to_string(j + 1) + " needs the Jacobian entry (" + std::to_string(rows[r]) + ", " +
                       std::to_string(cv[j] + 1) + ") that the structure of sqphip_create lacks";
    }
    return "";
}

std::string nlp_block_targets(const StructureSlots &S, int64_t m, int64_t nlin, int R, const int64_t *rows, const std::vector<int> &cv,
                              NlpBlockTargets &T)
{
    const int d = (int)cv.size();
    T.tgt.assign((size_t)R, -1); T.trow.clear(); T.js.clear();
    std::vector<int> seen((size_t)m + 1, -1);       // target of a row, once it has appeared
    // (the opening of a complaint, built on the failing paths only)
    auto out = [&](int r) { return "output " + std::to_string(r + 1) + ": row " + std::to_string(rows[r]); };
    for (int r = 0; r < R; ++r) {
        if (rows[r] < 0 || rows[r] > m) return out(r) + " outside 0.." + std::to_string(m);
        if (rows[r] >= 1 && rows[r] <= nlin) return out(r) + " is one of the num_linear = " + std::to_string(nlin) + " linear rows";
        int &t = seen[(size_t)rows[r]];
        if (t < 0) {
            t = (int)T.trow.size();
            T.trow.push_back((int)rows[r]);
            T.js.resize(T.js.size() + (size_t)d, -1);
            for (int j = 0; rows[r] >= 1 && j < d; ++j)
                if ((T.js[(size_t)t * d + j] = S.jfind(rows[r] - 1, cv[j])) < 0)
                    return out(r) + ", column " + std::to_string(j + 1) + " needs the Jacobian entry (" + std::to_string(rows[r]) + ", " +
                           std::to_string(cv[j] + 1) + ") that the structure of sqphip_create lacks";
        }
        T.tgt[r] = t;
    }
    // the outputs by target: a counting sort, which keeps them in rising order
    const int nt = (int)T.trow.size();
    T.tptr.assign((size_t)nt + 1, 0);
    for (int r = 0; r < R; ++r) ++T.tptr[(size_t)T.tgt[r] + 1];
    for (int t = 0; t < nt; ++t) T.tptr[(size_t)t + 1] += T.tptr[t];
    T.tout.assign((size_t)R, 0);
    std::vector<int> at(T.tptr.begin(), T.tptr.end() - 1);
    for (int r = 0; r < R; ++r) T.tout[(size_t)at[T.tgt[r]]++] = r;
    return "";
}

}  // namespace sqphip
