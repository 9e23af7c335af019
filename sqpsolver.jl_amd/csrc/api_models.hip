// api_models.hip -- the model side of the extern "C" boundary (include/sqphip.h): the attach and set-instance calls of the
// ACOPF forms, the dense NLP, the general QCQP and the factorable NLP with its data blocks, and the scenario queue of the
// QCQP and NLP contexts.  api.hip holds the rest of the boundary.
#include "api_util.hpp"
#include "qcqp_dev.hpp"
#include "nlp_dev.hpp"
#include <algorithm>
#include <cmath>

using namespace sqphip;

// ---- ACOPF evaluator + batched SQP -----------------------------------------------------------------
// structure counts of the two layouts (acopf_synth.py acopf_layout / acr_layout) without shunts
static int acopf_nnzj(int acr, int nb, int ng, int nl, int ndc)
{
    const int nbal = 2 * nl + ng + 2 * ndc;
    return acr ? 1 + 2 * nbal + 4 * nb + 24 * nl + 2 * ndc : 32 * nl + 2 * ng + 1 + 6 * ndc;
}
static int acopf_nnzh(int acr, int nb, int ng, int nl) { return acr ? ng + 28 * nl + 4 * nb : ng + 44 * nl; }
// ... and of the W-space layout (acwr_layout): the shunt entries are part of the structure
static int acwr_n(int nb, int nbp, int ng, int nl) { return 3 * nb + 2 * nbp + 2 * ng + 4 * nl; }
static int acwr_m(int nb, int nbp, int nl) { return 1 + 3 * nb + 4 * nbp + 6 * nl; }
static int acwr_nnzj(int nb, int nbp, int ng, int nl, int ndc)
{
    const int nbal = 2 * nl + ng + 2 * ndc;
    return 1 + 2 * nbal + 2 * nb + 4 * nbp + 16 * nl + 3 * nb + 10 * nbp + 4 * nl + 2 * ndc;
}
static int acwr_nnzh(int nb, int nbp, int ng, int nl) { return ng + 4 * nl + 2 * nb + 4 * nbp; }

// what the three forms check of the topology arrays ...
static bool acopf_topology_ok(const DV &d, int nb, int nl, int nbal, const int32_t *f_bus, const int32_t *t_bus, const int32_t *bal_colP,
                              const int32_t *bal_colQ, int ref_bus)
{
    for (int l = 0; l < nl; ++l)
        if (f_bus[l] < 0 || f_bus[l] >= nb || t_bus[l] < 0 || t_bus[l] >= nb) return false;
    for (int k = 0; k < nbal; ++k)
        if (bal_colP[k] < 0 || bal_colP[k] >= d.n || bal_colQ[k] < 0 || bal_colQ[k] >= d.n) return false;
    return ref_bus >= 0 && ref_bus < nb;
}

// ... and upload: the topology, the HVDC loss factors (zeros: sqphip_acopf_set_dclines overrides), the instances' tables
static void acopf_upload(Ctx &C, int nb, int ng, int nl, int ndc, int ref_bus, const int32_t *f_bus, const int32_t *t_bus,
                         const int32_t *gen_bus, const int32_t *bal_ptr, const int32_t *bal_colP, const int32_t *bal_colQ,
                         const double *bal_coef)
{
    DV &d = C.d;
    const int nbal = bal_ptr[nb];
    d.nb = nb; d.ng = ng; d.nl = nl; d.ref_bus = ref_bus; d.ndc = ndc;
    d.dc_loss1 = C.upload(std::vector<double>(ndc > 0 ? ndc : 1, 0.0));
    d.f_bus = C.upload(std::vector<int>(f_bus, f_bus + nl));
    d.t_bus = C.upload(std::vector<int>(t_bus, t_bus + nl));
    d.gen_bus = C.upload(std::vector<int>(gen_bus, gen_bus + ng));
    d.bal_ptr = C.upload(std::vector<int>(bal_ptr, bal_ptr + nb + 1));
    d.bal_colP = C.upload(std::vector<int>(bal_colP, bal_colP + nbal));
    d.bal_colQ = C.upload(std::vector<int>(bal_colQ, bal_colQ + nbal));
    d.bal_coef = C.upload(std::vector<double>(bal_coef, bal_coef + nbal));
    d.br_ohm = C.dalloc<double>((size_t)d.B * nl * 12);
    d.c2 = C.dalloc<double>((size_t)d.B * ng); d.c1 = C.dalloc<double>((size_t)d.B * ng);
}

static int acopf_attach_impl(sqphip_ctx *h, int acr, int32_t nb, int32_t ng, int32_t nl, const int32_t *f_bus,
                             const int32_t *t_bus, const int32_t *gen_bus, const int32_t *bal_ptr,
                             const int32_t *bal_colP, const int32_t *bal_colQ, const double *bal_coef,
                             int32_t ref_bus)
{
    if (!h || nb <= 0 || ng <= 0 || nl <= 0) return SQPHIP_EINVAL;
    if (!f_bus || !t_bus || !gen_bus || !bal_ptr || !bal_colP || !bal_colQ || !bal_coef) return SQPHIP_EINVAL;
    Ctx &C0 = h->c;
    // HVDC lines add 4 variables, 1 row, 2 balance incidences (= 4 Jacobian entries) and 2 loss-row entries each
    const int n_ac = 2 * nb + 2 * ng + 4 * nl, m_ac = acr ? 1 + 4 * nb + 6 * nl : 1 + 2 * nb + 8 * nl;
    if (C0.d.n < n_ac || (C0.d.n - n_ac) % 4 != 0) return SQPHIP_EINVAL;
    const int ndc = (C0.d.n - n_ac) / 4;
    if (C0.d.m != m_ac + ndc) return SQPHIP_EINVAL;
    const int nbal = bal_ptr[nb];
    // (a structure with bus shunts has 2 (polar) / 4 (rectangular) more Jacobian and 1 / 2 more Hessian entries per
    // shunted bus at the end of the lists; sqphip_acopf_set_shunts checks the exact counts)
    const int extraJ = C0.d.nnzj_coo - acopf_nnzj(acr, nb, ng, nl, ndc), extraH = C0.d.nnzh_coo - acopf_nnzh(acr, nb, ng, nl);
    if (extraJ < 0 || extraJ != 2 * extraH || extraH > (acr ? 2 * nb : nb) || nbal != 2 * nl + ng + 2 * ndc) return SQPHIP_EINVAL;
    if (!acopf_topology_ok(C0.d, nb, nl, nbal, f_bus, t_bus, bal_colP, bal_colQ, ref_bus)) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        C.d.acr = acr; C.d.acwr = 0;
        acopf_upload(C, nb, ng, nl, ndc, ref_bus, f_bus, t_bus, gen_bus, bal_ptr, bal_colP, bal_colQ, bal_coef);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        C.evaluator_attached = true;
        make_lanes(C);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_acopf_attach(sqphip_ctx *h, int32_t nb, int32_t ng, int32_t nl, const int32_t *f_bus,
                                   const int32_t *t_bus, const int32_t *gen_bus, const int32_t *bal_ptr,
                                   const int32_t *bal_colP, const int32_t *bal_colQ, const double *bal_coef,
                                   int32_t ref_bus)
{
    return acopf_attach_impl(h, 0, nb, ng, nl, f_bus, t_bus, gen_bus, bal_ptr, bal_colP, bal_colQ, bal_coef, ref_bus);
}

extern "C" int sqphip_acopf_attach_acr(sqphip_ctx *h, int32_t nb, int32_t ng, int32_t nl, const int32_t *f_bus,
                                       const int32_t *t_bus, const int32_t *gen_bus, const int32_t *bal_ptr,
                                       const int32_t *bal_colP, const int32_t *bal_colQ, const double *bal_coef,
                                       int32_t ref_bus)
{
    return acopf_attach_impl(h, 1, nb, ng, nl, f_bus, t_bus, gen_bus, bal_ptr, bal_colP, bal_colQ, bal_coef, ref_bus);
}

extern "C" int sqphip_acopf_attach_acwr(sqphip_ctx *h, int32_t nb, int32_t ng, int32_t nl, const int32_t *f_bus,
                                        const int32_t *t_bus, const int32_t *gen_bus, const int32_t *bal_ptr,
                                        const int32_t *bal_colP, const int32_t *bal_colQ, const double *bal_coef,
                                        int32_t ref_bus, int32_t nbp, const int32_t *bp_i, const int32_t *bp_j,
                                        const int32_t *br_bp, const double *br_sig, const double *bp_tmin,
                                        const double *bp_tmax)
{
    if (!h || nb <= 0 || ng <= 0 || nl <= 0 || nbp <= 0 || nbp > nl) return SQPHIP_EINVAL;
    if (!f_bus || !t_bus || !gen_bus || !bal_ptr || !bal_colP || !bal_colQ || !bal_coef) return SQPHIP_EINVAL;
    if (!bp_i || !bp_j || !br_bp || !br_sig || !bp_tmin || !bp_tmax) return SQPHIP_EINVAL;
    Ctx &C0 = h->c;
    const int n_ac = acwr_n(nb, nbp, ng, nl);
    if (C0.d.n < n_ac || (C0.d.n - n_ac) % 4 != 0) return SQPHIP_EINVAL;
    const int ndc = (C0.d.n - n_ac) / 4;
    if (C0.d.m != acwr_m(nb, nbp, nl) + ndc) return SQPHIP_EINVAL;
    const int nbal = bal_ptr[nb];
    if (C0.d.nnzj_coo != acwr_nnzj(nb, nbp, ng, nl, ndc) || C0.d.nnzh_coo != acwr_nnzh(nb, nbp, ng, nl) ||
        nbal != 2 * nl + ng + 2 * ndc) return SQPHIP_EINVAL;
    for (int l = 0; l < nl; ++l)
        if (br_bp[l] < 0 || br_bp[l] >= nbp || !(br_sig[l] == 1.0 || br_sig[l] == -1.0)) return SQPHIP_EINVAL;
    for (int k = 0; k < nbp; ++k)
        if (bp_i[k] < 0 || bp_j[k] >= nb || bp_i[k] >= bp_j[k]) return SQPHIP_EINVAL;
    if (!acopf_topology_ok(C0.d, nb, nl, nbal, f_bus, t_bus, bal_colP, bal_colQ, ref_bus)) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        d.acr = 0; d.acwr = 1; d.nbp = nbp;
        acopf_upload(C, nb, ng, nl, ndc, ref_bus, f_bus, t_bus, gen_bus, bal_ptr, bal_colP, bal_colQ, bal_coef);
        d.bp_i = C.upload(std::vector<int>(bp_i, bp_i + nbp)); d.bp_j = C.upload(std::vector<int>(bp_j, bp_j + nbp));
        d.br_bp = C.upload(std::vector<int>(br_bp, br_bp + nl));
        d.br_sig = C.upload(std::vector<double>(br_sig, br_sig + nl));
        d.bp_tmin = C.upload(std::vector<double>(bp_tmin, bp_tmin + nbp));
        d.bp_tmax = C.upload(std::vector<double>(bp_tmax, bp_tmax + nbp));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        C.evaluator_attached = true;
        make_lanes(C);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_acopf_set_shunts(sqphip_ctx *h, int32_t nsh, const int32_t *sh_bus, const double *gs,
                                       const double *bs)
{
    if (acopf_only(h, "sqphip_acopf_set_shunts")) return SQPHIP_EINVAL;
    if (!h || !h->c.evaluator_attached || nsh < 0) return SQPHIP_EINVAL;
    Ctx &C0 = h->c;
    const int nl = C0.d.nl, ng = C0.d.ng, nb = C0.d.nb;
    const int acr = C0.d.acr;
    if (!C0.d.acwr) {                    // (the W-space structure carries the shunt entries of every bus already)
        if (C0.d.nnzj_coo != acopf_nnzj(acr, nb, ng, nl, C0.d.ndc) + (acr ? 4 : 2) * nsh ||
            C0.d.nnzh_coo != acopf_nnzh(acr, nb, ng, nl) + (acr ? 2 : 1) * nsh) return SQPHIP_EINVAL;
        if (nsh > 0 && C0.d.nlin != (acr ? 1 : 2 * nl + 1)) return SQPHIP_EINVAL; // balance rows must not be declared linear
    }
    std::vector<int> of(nb, -1);
    for (int s = 0; s < nsh; ++s) {
        if (sh_bus[s] < 0 || sh_bus[s] >= nb || of[sh_bus[s]] >= 0) return SQPHIP_EINVAL;
        of[sh_bus[s]] = s;
    }
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        d.nsh = nsh;
        d.sh_bus = C.upload(std::vector<int>(sh_bus, sh_bus + nsh));
        d.sh_of_bus = C.upload(of);
        d.sh_gs = C.upload(std::vector<double>(gs, gs + nsh));
        d.sh_bs = C.upload(std::vector<double>(bs, bs + nsh));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        make_lanes(C);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_acopf_set_dclines(sqphip_ctx *h, int32_t ndc, const double *loss1)
{
    if (acopf_only(h, "sqphip_acopf_set_dclines")) return SQPHIP_EINVAL;
    if (!h || !h->c.evaluator_attached || ndc != h->c.d.ndc || (ndc > 0 && !loss1)) return SQPHIP_EINVAL;
    if (ndc == 0) return SQPHIP_OK;
    return guarded(h, [&](Ctx &C) {
        C.d.dc_loss1 = C.upload(std::vector<double>(loss1, loss1 + ndc));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        make_lanes(C);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_acopf_set_instance(sqphip_ctx *h, int32_t inst, const double *ohm, const double *c2,
                                         const double *c1, const double *x0)
{
    if (acopf_only(h, "sqphip_acopf_set_instance")) return SQPHIP_EINVAL;
    if (!h || !h->c.evaluator_attached || inst < 0 || inst >= h->c.d.B) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        h2d(C, d.br_ohm + (size_t)inst * d.nl * 12, ohm, (size_t)d.nl * 12);
        h2d(C, d.c2 + (size_t)inst * d.ng, c2, d.ng); h2d(C, d.c1 + (size_t)inst * d.ng, c1, d.ng);
        h2d(C, d.x0 + (size_t)inst * d.n, x0, d.n);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

// ---- the synthetic dense-Hessian NLP (acopf_dev.hpp dense_eval): structure as sqpsolver.jl_amd/dense_synth.py lays it out
extern "C" int sqphip_dense_attach(sqphip_ctx *h, const double *Q, const double *A, double kappa)
{
    if (!h || !Q || !A || !(kappa >= 0.0)) return SQPHIP_EINVAL;
    Ctx &C0 = h->c;
    const long n = C0.d.n, m = C0.d.m;
    if (C0.d.nnzj_coo != m * n || C0.d.nnzh_coo != n * (n + 1) / 2 || C0.d.nlin != m) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        double *q = C.dalloc<double>((size_t)(n * n)), *a = C.dalloc<double>((size_t)(m * n));
        h2d(C, q, Q, (size_t)(n * n)); h2d(C, a, A, (size_t)(m * n));
        d.dnQ = q; d.dnA = a; d.dn_kappa = kappa;
        d.dnc = C.dalloc<double>((size_t)d.B * n);
        d.dense_nlp = 1;
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        C.evaluator_attached = true;           // (the batched run! has its device callbacks)
        make_lanes(C);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_dense_set_instance(sqphip_ctx *h, int32_t inst, const double *c, const double *x0)
{
    if (!h || !h->c.d.dense_nlp || inst < 0 || inst >= h->c.d.B || !c || !x0) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        h2d(C, d.dnc + (size_t)inst * d.n, c, d.n);
        h2d(C, d.x0 + (size_t)inst * d.n, x0, d.n);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

// ---- a general sparse QCQP (qcqp_dev.hpp qcqp_eval) and a sparse factorable NLP (nlp_dev.hpp nlp_eval).  An attach reads:
// null and state checks, the plan from the terms and the COO structures of sqphip_create (model_plans.cpp, host only), one
// upload that fills QcqpDev / NlpDev, the lanes.
static int no_evaluator_yet(sqphip_ctx *h, const char *who)
{
    if (!h->c.evaluator_attached) return SQPHIP_OK;
    h->c.err = std::string(who) + ": the context already has device callbacks (an earlier *_attach)";
    return SQPHIP_ESTATE;
}

static StructureSlots structure_slots(const Ctx &C)
{
    return StructureSlots(C.d.n, C.d.nnzj_coo, C.h_jrow.data(), C.h_jcol.data(), C.d.nnzh_coo, C.h_hrow.data(), C.h_hcol.data());
}

// the instances' blocks of values [B][nv] as an attach leaves them: val0 [nv] in every one (the set-instance calls overwrite)
static double *upload_blocks(Ctx &C, const std::vector<double> &val0)
{
    std::vector<double> all((size_t)C.d.B * val0.size());
    for (int b = 0; b < C.d.B; ++b) std::copy(val0.begin(), val0.end(), all.begin() + (size_t)b * val0.size());
    return C.upload(all);
}

// the two range messages of the set-instance and queue calls
static int instance_in_batch(sqphip_ctx *h, const std::string &who, int32_t inst)
{
    if (inst >= 0 && inst < h->c.d.B) return SQPHIP_OK;
    h->c.err = who + ": instance " + std::to_string(inst) + " is outside the batch of " + std::to_string(h->c.d.B);
    return SQPHIP_EINVAL;
}
static int scenario_in_queue(sqphip_ctx *h, const std::string &who, int32_t scen)
{
    if (scen >= 0 && scen < h->c.d.stream.M) return SQPHIP_OK;
    h->c.err = who + ": scenario " + std::to_string(scen) + " is outside the " + std::to_string(h->c.d.stream.M) + " of the queue";
    return SQPHIP_EINVAL;
}

extern "C" int sqphip_qcqp_attach(sqphip_ctx *h, int64_t nnzQ0, const int64_t *q0r, const int64_t *q0c, const double *q0v,
                                  int64_t nnzA, const int64_t *ar, const int64_t *ac, const double *av, int64_t nnzQ,
                                  const int64_t *qi, const int64_t *qr, const int64_t *qc, const double *qv,
                                  const double *c, const double *g0, double f0)
{
    const char *who = "sqphip_qcqp_attach";
    if (!h) return SQPHIP_EINVAL;
    if (int rc = no_evaluator_yet(h, who)) return rc;
    QcqpPlan L;
    if (int rc = build_qcqp_plan(structure_slots(h->c), h->c.d.m, h->c.d.nlin, who, nnzQ0, q0r, q0c, q0v, nnzA, ar, ac, av, nnzQ, qi, qr,
                                 qc, qv, c, g0, f0, L, h->c.err)) return rc;
    return guarded(h, [&](Ctx &C) {
        QcqpDev P = {};
        P.n = L.n; P.m = L.m; P.nv = (int)L.host.nv; P.nq0 = L.nq0;
        P.off_c = (int)L.host.off[1]; P.off_q0 = (int)L.host.off[2]; P.off_g0 = (int)L.host.off[3];
        P.f_ptr = L.f_ptr; P.j_ptr = L.j_ptr; P.h_ptr = L.h_ptr;
        P.ptr = C.upload(L.ptr); P.q0 = (const int2 *)C.upload(L.q0); P.ge = (const int4 *)C.upload(L.ge);
        P.fe = (const int2 *)C.upload(L.fe); P.je = (const int2 *)C.upload(L.je); P.he = (const int2 *)C.upload(L.he);
        QcqpDev *pd = (QcqpDev *)C.dalloc<char>(sizeof(QcqpDev));
        SQPHIP_HIP_OK(hipMemcpyAsync(pd, &P, sizeof(QcqpDev), hipMemcpyHostToDevice, C.stream));
        C.d.qcv = upload_blocks(C, L.host.base);
        C.d.qc = pd;
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        C.qc = std::move(L.host);
        C.evaluator_attached = true;       // (the batched run! has its device callbacks)
        make_lanes(C);
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_qcqp_set_instance(sqphip_ctx *h, int32_t inst, const double *f0, const double *c, const double *q0v,
                                        const double *g0, const double *av, const double *qv, const double *x0)
{
    if (h && !h->c.d.qc && h->c.evaluator_attached) {
        h->c.err = "sqphip_qcqp_set_instance: the context has no QCQP attached (sqphip_qcqp_attach)";
        return SQPHIP_EINVAL;
    }
    if (!h || !h->c.d.qc || inst < 0 || inst >= h->c.d.B) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        const long *o = C.qc.off;           // f0 | c | Q0 | g0 | A | Q | end
        double *v = d.qcv + (size_t)inst * C.qc.nv;
        const double *src[6] = {f0, c, q0v, g0, av, qv};
        for (int k = 0; k < 6; ++k) h2d(C, v + o[k], src[k], (size_t)(o[k + 1] - o[k]));
        h2d(C, d.x0 + (size_t)inst * d.n, x0, d.n);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

static int nlp_attach_impl(sqphip_ctx *h, const char *who, const NlpOptions &O, int64_t nterms, const int64_t *trow, const double *tcoef,
                           const int64_t *tptr, const int64_t *aptr, const int64_t *avar, const double *acoef, const int32_t *fkind,
                           const int32_t *fexp, const double *fpar, const double *fshift, const double *g0, double f0)
{
    if (!h) return SQPHIP_EINVAL;
    if (int rc = no_evaluator_yet(h, who)) return rc;
    StructureSlots S = structure_slots(h->c);
    NlpPlan L;
    if (int rc = build_nlp_plan(S, h->c.d.m, h->c.d.nlin, who, O, nterms, trow, tcoef, tptr, aptr, avar, acoef, fkind, fexp, fpar, fshift,
                                g0, f0, L, h->c.err)) return rc;
    L.host.slots = std::move(S);
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        const NlpHost &H = L.host;
        NlpDev P = {};
        P.n = L.n; P.m = L.m; P.nterms = (int)H.nterms; P.nfac = (int)H.nfac; P.nv = (int)H.nv; P.nobj = L.nobj;
        P.f_ptr = L.f_ptr; P.j_ptr = L.j_ptr; P.h_ptr = L.h_ptr;
        P.ptr = C.upload(L.ptr); P.tptr = C.upload(H.tptr); P.fvar = C.upload(L.fvar); P.fke = C.upload(L.fke);
        P.fab = (const double2 *)C.upload(L.fab);
        P.ot = C.upload(L.ot); P.ge = C.upload(L.ge); P.fe = (const int2 *)C.upload(L.fe); P.je = (const int2 *)C.upload(L.je);
        P.he = (const int4 *)C.upload(L.he);
        P.aptr = C.upload(H.aptr); P.avar = C.upload(L.avar); P.acoef = C.upload(L.acoef); P.aw = C.upload(L.aw); P.multi = L.multi;
        P.fpar = C.upload(L.fpar);
        P.data = H.data ? 1 : 0; P.ob = (int)H.ob; P.oa = (int)H.oa; P.op = (int)H.op;
        P.ws = (int)H.ws;
        NlpDev *pd = (NlpDev *)C.dalloc<char>(sizeof(NlpDev));
        SQPHIP_HIP_OK(hipMemcpyAsync(pd, &P, sizeof(NlpDev), hipMemcpyHostToDevice, C.stream));
        d.nlv = upload_blocks(C, H.base);
        d.nlw = C.dalloc<double>((size_t)d.B * (size_t)H.ws);
        d.nlp = pd;
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        C.nl = std::move(L.host);
        C.evaluator_attached = true;       // (the batched run! has its device callbacks)
        make_lanes(C);
        return SQPHIP_OK;
    });
}

// The four entry points (NlpOptions, model_plans.hpp): the two older calls are the general one with the menu check at LOG and
// the distinct-variables check switched on; sqphip_nlp_attach has no aptr, its fscale is the coefficient of the one argument.
extern "C" int sqphip_nlp_attach(sqphip_ctx *h, int64_t nterms, const int64_t *trow, const double *tcoef, const int64_t *tptr,
                                 const int64_t *fvar, const int32_t *fkind, const int32_t *fexp, const double *fscale,
                                 const double *fshift, const double *g0, double f0)
{
    return nlp_attach_impl(h, "sqphip_nlp_attach", {false, NLP_LOG, true, false}, nterms, trow, tcoef, tptr, nullptr, fvar, fscale, fkind, fexp, nullptr, fshift, g0, f0);
}

extern "C" int sqphip_nlp_attach_affine(sqphip_ctx *h, int64_t nterms, const int64_t *trow, const double *tcoef, const int64_t *tptr,
                                        const int64_t *aptr, const int64_t *avar, const double *acoef, const int32_t *fkind,
                                        const int32_t *fexp, const double *fshift, const double *g0, double f0)
{
    return nlp_attach_impl(h, "sqphip_nlp_attach_affine", {true, NLP_LOG, true, false}, nterms, trow, tcoef, tptr, aptr, avar, acoef, fkind, fexp, nullptr, fshift, g0, f0);
}

extern "C" int sqphip_nlp_attach_general(sqphip_ctx *h, int64_t nterms, const int64_t *trow, const double *tcoef, const int64_t *tptr,
                                         const int64_t *aptr, const int64_t *avar, const double *acoef, const int32_t *fkind,
                                         const int32_t *fexp, const double *fpar, const double *fshift, const double *g0, double f0)
{
    return nlp_attach_impl(h, "sqphip_nlp_attach_general", {true, NLP_POWR, false, false}, nterms, trow, tcoef, tptr, aptr, avar, acoef, fkind, fexp, fpar, fshift, g0, f0);
}

extern "C" int sqphip_nlp_attach_data(sqphip_ctx *h, int64_t nterms, const int64_t *trow, const double *tcoef, const int64_t *tptr,
                                      const int64_t *aptr, const int64_t *avar, const double *acoef, const int32_t *fkind,
                                      const int32_t *fexp, const double *fpar, const double *fshift, const double *g0, double f0)
{
    return nlp_attach_impl(h, "sqphip_nlp_attach_data", {true, NLP_POWR, false, true}, nterms, trow, tcoef, tptr, aptr, avar, acoef, fkind, fexp, fpar, fshift, g0, f0);
}

// nlp_data_check (model_plans.hpp) into the context's error
static int nlp_data_refused(sqphip_ctx *h, const char *who, const double *fshift, const double *acoef, const double *fpar)
{
    const std::string bad = nlp_data_check(h->c.nl, h->c.d.nlin, who, fshift, acoef, fpar);
    if (bad.empty()) return SQPHIP_OK;
    h->c.err = bad;
    return SQPHIP_EINVAL;
}

// ... and the upload of the parts given into the block v (of an instance or of a scenario of the queue)
static void nlp_data_upload(Ctx &C, double *v, const double *fshift, const double *acoef, const double *fpar)
{
    h2d(C, v + C.nl.ob, fshift, (size_t)C.nl.nfac); h2d(C, v + C.nl.oa, acoef, (size_t)C.nl.nargs);
    if (C.nl.op >= 0) h2d(C, v + C.nl.op, fpar, (size_t)C.nl.nfac);
}

extern "C" int sqphip_nlp_set_instance_data(sqphip_ctx *h, int32_t inst, const double *fshift, const double *acoef, const double *fpar)
{
    const char *who = "sqphip_nlp_set_instance_data";
    if (!h) return SQPHIP_EINVAL;
    if (int rc = nlp_data_refused(h, who, nullptr, nullptr, nullptr)) return rc;
    if (int rc = instance_in_batch(h, who, inst)) return rc;
    if (int rc = nlp_data_refused(h, who, fshift, acoef, fpar)) return rc;
    return guarded(h, [&](Ctx &C) {
        nlp_data_upload(C, C.d.nlv + (size_t)inst * C.nl.nv, fshift, acoef, fpar);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_nlp_set_instance(sqphip_ctx *h, int32_t inst, const double *f0, const double *g0, const double *tcoef,
                                       const double *x0)
{
    if (h && !h->c.d.nlp) {
        h->c.err = "sqphip_nlp_set_instance: the context has no factorable NLP attached (sqphip_nlp_attach)";
        return SQPHIP_EINVAL;
    }
    if (!h || inst < 0 || inst >= h->c.d.B) return SQPHIP_EINVAL;
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        double *v = d.nlv + (size_t)inst * C.nl.nv;           // f0 | g0 | c
        h2d(C, v, f0, 1); h2d(C, v + 1, g0, d.m); h2d(C, v + 1 + d.m, tcoef, (size_t)C.nl.nterms);
        h2d(C, d.x0 + (size_t)inst * d.n, x0, d.n);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

// ---- dense data blocks of a factorable NLP (nlp_blocks_dev.hpp, the six family headers, nlp_blocks_eval of nlp_dev.hpp)
// the state rules of the add calls; kb: the number of the block to be, blk: "who: block kb + 1" for the messages
static int nlp_block_begin(sqphip_ctx *h, const std::string &who, int &kb, std::string &blk)
{
    if (!h) return SQPHIP_EINVAL;
    Ctx &C0 = h->c;
    if (!C0.d.nlp) { C0.err = who + ": the context has no factorable NLP attached (sqphip_nlp_attach*)"; return SQPHIP_EINVAL; }
    if (C0.nl.started) {
        C0.err = who + ": the layout of the instances is final after sqphip_sqp_reset, sqphip_sqp_run or sqphip_nlp_stream_begin";
        return SQPHIP_ESTATE;
    }
    kb = (int)C0.nl.blk.size();
    blk = who + ": block " + std::to_string(kb + 1);
    if (kb >= NLP_MAX_BLOCKS) { C0.err = blk + ": a context takes at most " + std::to_string((int)NLP_MAX_BLOCKS) + " blocks"; return SQPHIP_EINVAL; }
    return SQPHIP_OK;
}

// Re-lays the instances' blocks of doubles behind what they hold with W [nW] | S [nS] of block kb (weight NULL: ones, shift
// NULL: zeros), uploads A [N][d] and its transpose, cv and hs, and files the block K (ke, par, K, Kf, y: the caller's; wsz:
// its doubles of workspace) in the context's NlpDev.
static int nlp_block_commit(sqphip_ctx *h, const std::string &blk, int kb, long N, int d, long nW, long nS, long wsz, const double *A,
                            const std::vector<int> &cv, const std::vector<int> &hs, const double *weight, const double *shift,
                            NlpBlkDev K, int32_t *blk_out)
{
    Ctx &C0 = h->c;
    const long ow = C0.nl.end, os = ow + nW, end = os + nS, nv = (end + 1) & ~1L;
    const long wz = C0.nl.ws + (kb == 0 ? TPB / 64 + 3 * TPB : 0), ws = wz + wsz;
    if (nv > INT32_MAX || ws > INT32_MAX) { C0.err = blk + ": too many values per instance"; return SQPHIP_EINVAL; }
    return guarded(h, [&](Ctx &C) {
        DV &dv = C.d;
        const long nv0 = C.nl.nv, B = dv.B;
        // re-lay the instances' blocks behind what they hold
        std::vector<double> old((size_t)B * nv0), all((size_t)B * nv, 0.0);
        d2h(C, old.data(), dv.nlv, old.size());
        NlpDev P;
        SQPHIP_HIP_OK(hipMemcpyAsync(&P, dv.nlp, sizeof(NlpDev), hipMemcpyDeviceToHost, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        auto fill = [&](double *v) {
            for (long i = 0; i < nW; ++i) v[ow + i] = weight ? weight[i] : 1.0;
            for (long i = 0; i < nS; ++i) v[os + i] = shift ? shift[i] : 0.0;
        };
        for (long b = 0; b < B; ++b) {
            std::copy(old.begin() + b * nv0, old.begin() + b * nv0 + C.nl.end, all.begin() + b * nv);
            fill(all.data() + b * nv);
        }
        C.nl.base.resize(nv, 0.0);
        std::fill(C.nl.base.begin() + C.nl.end, C.nl.base.end(), 0.0);
        fill(C.nl.base.data());
        std::vector<double> a(A, A + (size_t)N * d), at((size_t)N * d);
        for (long i = 0; i < N; ++i)
            for (int j = 0; j < d; ++j) at[(size_t)j * N + i] = a[(size_t)i * d + j];
        K.N = (int)N; K.d = d; K.ow = (int)ow; K.os = (int)os; K.wz = (int)wz;
        K.A = C.upload(a); K.At = C.upload(at); K.col = C.upload(cv); K.hs = C.upload(hs);
        P.blk[kb] = K;
        P.nblk = kb + 1; P.nv = (int)nv; P.ws = (int)ws;
        dv.nlv = C.upload(all);
        dv.nlw = C.dalloc<double>((size_t)B * (size_t)ws);
        SQPHIP_HIP_OK(hipMemcpyAsync(const_cast<NlpDev *>(dv.nlp), &P, sizeof(NlpDev), hipMemcpyHostToDevice, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        C.nl.nv = nv; C.nl.end = end; C.nl.ws = ws;
        C.nl.blk.push_back(NlpHost::Block{N, ow, os, nS, nW});
        make_lanes(C);
        if (blk_out) *blk_out = kb;
        return SQPHIP_OK;
    });
}

// The opening of an add call: the null handle and the state rules (begin), and the refusal "who: block k: msg" (fail)
struct NlpBlockAdd {
    sqphip_ctx *h;
    int kb = 0;
    std::string blk;
    int begin(const char *who) { return nlp_block_begin(h, who, kb, blk); }
    int fail(const std::string &msg) const { h->c.err = blk + ": " + msg; return (int)SQPHIP_EINVAL; }
};

// what every add call refuses of N points on d columns, of which it takes max_d at most (the softmax block, which has checked
// its own Kf d, passes d)
static std::string nlp_block_shape(int64_t N, int32_t d, int max_d)
{
    if (d < 1 || d > max_d) return "d = " + std::to_string(d) + " columns (1.." + std::to_string(max_d) + ")";
    if (N < 1) return "N = " + std::to_string(N) + " points (at least 1)";
    if (N > INT32_MAX / d) return "N d = " + std::to_string(N) + " x " + std::to_string(d) + " is too large (N d < 2^31)";
    return "";
}

// what sqphip_nlp_add_lse_block and sqphip_nlp_add_norm_block refuse of R outputs over consecutive segments of the N points
static std::string nlp_block_segments(int64_t N, int32_t d, int32_t R, const int64_t *rows, const int64_t *seg)
{
    if (R < 1 || R > N) return "R = " + std::to_string(R) + " outputs (1.." + std::to_string(N) + ")";
    if (R > INT32_MAX / d) return "R d = " + std::to_string(R) + " x " + std::to_string(d) + " is too large (R d < 2^31)";
    if (!rows || !seg) return "null rows or seg";
    if (seg[0] != 0) return "output 1: seg[0] = " + std::to_string(seg[0]) + " (the first segment starts at point 0)";
    for (int r = 0; r < R; ++r)
        if (seg[r + 1] <= seg[r])
            return "output " + std::to_string(r + 1) + ": the segment " + std::to_string(seg[r]) + ".." + std::to_string(seg[r + 1]) +
                   " is " + (seg[r + 1] == seg[r] ? "empty" : "decreasing");
    if (seg[R] != N) return "output " + std::to_string(R) + ": seg[R] = " + std::to_string(seg[R]) + " (the last segment ends at N = " + std::to_string(N) + ")";
    return "";
}

// what sqphip_nlp_add_block and sqphip_nlp_add_row_block refuse of the shape and the menu entry; e: the exponent in use
static std::string nlp_block_menu(int32_t kind, int32_t exp, double par, int64_t N, int32_t d, const int64_t *cols, const double *A, int &e)
{
    if (const std::string bad = nlp_block_shape(N, d, NLP_BLOCK_MAX_D); !bad.empty()) return bad;
    if (!cols || !A) return "null cols or A";
    if (kind < NLP_POW || kind > NLP_POWR) return "unknown kind " + std::to_string(kind);
    e = kind == NLP_POW ? exp : 1;
    if (kind == NLP_POW && e == 1) return "a plain linear block (POW, e = 1) belongs in the terms";
    if (e == 0 || e > 32 || e < -32) return "exponent " + std::to_string(e) + " (1 <= |e| <= 32)";
    if (kind == NLP_POWR && (!std::isfinite(par) || par == 0.0)) return "real exponent " + std::to_string(par) + " (finite and not 0)";
    return "";
}

extern "C" int sqphip_nlp_add_block(sqphip_ctx *h, int32_t kind, int32_t exp, double par, int64_t N, int32_t d, const int64_t *cols,
                                    const double *A, const double *shift, const double *weight, int32_t *blk_out)
{
    NlpBlockAdd call{h};
    if (int rc = call.begin("sqphip_nlp_add_block")) return rc;
    Ctx &C0 = h->c;
    int e;
    if (const std::string bad = nlp_block_menu(kind, exp, par, N, d, cols, A, e); !bad.empty()) return call.fail(bad);
    std::vector<int> hs, cv;
    if (const std::string bad = nlp_block_columns(C0.nl.slots, d, cols, cv, hs); !bad.empty()) return call.fail(bad);
    NlpBlkDev K = {};
    K.family = NLP_BLK_SCALAR;
    K.ke = kind + (e + 32) * (1 << NLP_KIND_BITS);
    K.par = kind == NLP_POWR ? par : 0.0;
    return nlp_block_commit(h, call.blk, call.kb, (long)N, d, (long)N, (long)N, nlp_block_ws(N).size, A, cv, hs, weight, shift, K, blk_out);
}

// a block with several outputs (nlp_rowblock_dev.hpp): the checks of sqphip_nlp_add_block, then the rows and their Jacobian slots
extern "C" int sqphip_nlp_add_row_block(sqphip_ctx *h, int32_t kind, int32_t exp, double par, int64_t N, int32_t d, const int64_t *cols,
                                        const double *A, int32_t R, const int64_t *rows, const double *shift, const double *weight,
                                        int32_t *blk_out)
{
    NlpBlockAdd call{h};
    if (int rc = call.begin("sqphip_nlp_add_row_block")) return rc;
    Ctx &C0 = h->c;
    int e;
    if (const std::string bad = nlp_block_menu(kind, exp, par, N, d, cols, A, e); !bad.empty()) return call.fail(bad);
    if (R < 1 || R > NLP_BLOCK_MAX_R) return call.fail("R = " + std::to_string(R) + " outputs (1.." + std::to_string((int)NLP_BLOCK_MAX_R) + ")");
    if (!rows) return call.fail("null rows");
    if (N > INT32_MAX / R) return call.fail("R N = " + std::to_string(R) + " x " + std::to_string(N) + " is too large (R N < 2^31)");
    std::vector<int> hs, cv;
    if (const std::string bad = nlp_block_columns(C0.nl.slots, d, cols, cv, hs); !bad.empty()) return call.fail(bad);
    NlpBlkDev K = {};
    std::vector<int> js;
    if (const std::string bad = nlp_block_rows(C0.nl.slots, C0.d.m, C0.d.nlin, R, rows, cv, K.row, js); !bad.empty()) return call.fail(bad);
    K.family = NLP_BLK_ROWS;
    K.ke = kind + (e + 32) * (1 << NLP_KIND_BITS);
    K.par = kind == NLP_POWR ? par : 0.0;
    K.R = R;
    const int rc = guarded(h, [&](Ctx &C) { K.js = C.upload(js); return SQPHIP_OK; });
    if (rc) return rc;
    return nlp_block_commit(h, call.blk, call.kb, (long)N, d, (long)R * N, (long)N, nlp_rowblock_ws(N).size, A, cv, hs, weight, shift, K, blk_out);
}

// a multinomial (softmax) block (nlp_softmax_dev.hpp)
extern "C" int sqphip_nlp_add_softmax_block(sqphip_ctx *h, int64_t N, int32_t d, int32_t K, int32_t pinned, const int64_t *cols,
                                            const double *A, const int32_t *labels, const double *shift, const double *weight,
                                            int32_t *blk_out)
{
    NlpBlockAdd call{h};
    if (int rc = call.begin("sqphip_nlp_add_softmax_block")) return rc;
    Ctx &C0 = h->c;
    if (K < 2 || K > NLP_SOFTMAX_MAX_K) return call.fail("K = " + std::to_string(K) + " classes (2.." + std::to_string((int)NLP_SOFTMAX_MAX_K) + ")");
    if (d < 1) return call.fail("d = " + std::to_string(d) + " features (at least 1)");
    const int Kf = pinned ? K - 1 : K;
    if ((long)Kf * d > NLP_BLOCK_MAX_D)
        return call.fail("Kf d = " + std::to_string(Kf) + " x " + std::to_string(d) + " columns (at most " + std::to_string((int)NLP_BLOCK_MAX_D) + ")");
    if (const std::string bad = nlp_block_shape(N, d, d); !bad.empty()) return call.fail(bad);
    if (!cols || !A || !labels) return call.fail("null cols, A or labels");
    for (int64_t i = 0; i < N; ++i)
        if (labels[i] < 0 || labels[i] >= K)
            return call.fail("point " + std::to_string(i + 1) + ": label " + std::to_string(labels[i]) + " outside 0.." + std::to_string(K - 1));
    std::vector<int> hs, cv;
    if (const std::string bad = nlp_block_columns(C0.nl.slots, Kf * d, cols, cv, hs); !bad.empty()) return call.fail(bad);
    NlpBlkDev Kb = {};
    Kb.family = NLP_BLK_SOFTMAX;
    Kb.K = K; Kb.Kf = Kf;
    const int rc = guarded(h, [&](Ctx &C) { Kb.y = C.upload(std::vector<int>(labels, labels + N)); return SQPHIP_OK; });
    if (rc) return rc;
    return nlp_block_commit(h, call.blk, call.kb, (long)N, d, (long)N, (long)Kf * N, nlp_softmax_ws(N, Kf).size, A, cv, hs, weight, shift, Kb, blk_out);
}

// a Cox partial-likelihood block (nlp_cox_dev.hpp): the shape checks of sqphip_nlp_add_block, then risk and event
extern "C" int sqphip_nlp_add_cox_block(sqphip_ctx *h, int64_t N, int32_t d, const int64_t *cols, const double *A, const int32_t *risk,
                                        const double *event, const double *shift, const double *weight, int32_t *blk_out)
{
    NlpBlockAdd call{h};
    if (int rc = call.begin("sqphip_nlp_add_cox_block")) return rc;
    Ctx &C0 = h->c;
    if (const std::string bad = nlp_block_shape(N, d, NLP_BLOCK_MAX_D); !bad.empty()) return call.fail(bad);
    if (!cols || !A || !risk || !event) return call.fail("null cols, A, risk or event");
    for (int64_t i = 0; i < N; ++i) {
        if (risk[i] < i + 1 || risk[i] > N)
            return call.fail("point " + std::to_string(i + 1) + ": risk " + std::to_string(risk[i]) + " outside " + std::to_string(i + 1) + ".." + std::to_string(N));
        if (i > 0 && risk[i] < risk[i - 1])
            return call.fail("point " + std::to_string(i + 1) + ": risk " + std::to_string(risk[i]) + " decreases from " + std::to_string(risk[i - 1]));
        if (!std::isfinite(event[i]) || event[i] < 0.0)
            return call.fail("point " + std::to_string(i + 1) + ": event " + std::to_string(event[i]) + " (finite and not negative)");
    }
    std::vector<int> hs, cv;
    if (const std::string bad = nlp_block_columns(C0.nl.slots, d, cols, cv, hs); !bad.empty()) return call.fail(bad);
    // first[j]: the first point whose risk set holds point j; risk is non-decreasing, so these points are i >= first[j]
    std::vector<int> fst((size_t)N);
    for (int64_t j = 0, i = 0; j < N; ++j) {
        while (risk[i] <= j) ++i;              // (risk[j] >= j + 1: i <= j)
        fst[j] = (int)i;
    }
    NlpBlkDev Kb = {};
    Kb.family = NLP_BLK_COX;
    const int rc = guarded(h, [&](Ctx &C) {
        Kb.risk = C.upload(std::vector<int>(risk, risk + N)); Kb.first = C.upload(fst);
        Kb.event = C.upload(std::vector<double>(event, event + N));
        return SQPHIP_OK;
    });
    if (rc) return rc;
    return nlp_block_commit(h, call.blk, call.kb, (long)N, d, (long)N, (long)N, nlp_cox_ws(N, d).size, A, cv, hs, weight, shift, Kb, blk_out);
}

// a log-sum-exp row block (nlp_lse_dev.hpp): the shape checks of sqphip_nlp_add_cox_block, then the segments, the rows and their
// Jacobian slots; rows, seg, the output of every point and the slots are uploaded, so R is not capped
extern "C" int sqphip_nlp_add_lse_block(sqphip_ctx *h, int64_t N, int32_t d, const int64_t *cols, const double *A, int32_t R,
                                        const int64_t *rows, const int64_t *seg, const double *shift, const double *weight,
                                        int32_t *blk_out)
{
    NlpBlockAdd call{h};
    if (int rc = call.begin("sqphip_nlp_add_lse_block")) return rc;
    Ctx &C0 = h->c;
    if (const std::string bad = nlp_block_shape(N, d, NLP_BLOCK_MAX_D); !bad.empty()) return call.fail(bad);
    if (!cols || !A) return call.fail("null cols or A");
    if (const std::string bad = nlp_block_segments(N, d, R, rows, seg); !bad.empty()) return call.fail(bad);
    std::vector<int> hs, cv;
    if (const std::string bad = nlp_block_columns(C0.nl.slots, d, cols, cv, hs); !bad.empty()) return call.fail(bad);
    std::vector<int> row((size_t)R), js;
    if (const std::string bad = nlp_block_rows(C0.nl.slots, C0.d.m, C0.d.nlin, R, rows, cv, row.data(), js); !bad.empty()) return call.fail(bad);
    std::vector<int> sg((size_t)R + 1), outp((size_t)N);
    for (int r = 0; r <= R; ++r) sg[r] = (int)seg[r];
    for (int r = 0; r < R; ++r)
        for (int i = sg[r]; i < sg[r + 1]; ++i) outp[i] = r;
    NlpBlkDev Kb = {};
    Kb.family = NLP_BLK_LSE;
    Kb.R = R;
    const int rc = guarded(h, [&](Ctx &C) {
        Kb.lrow = C.upload(row); Kb.seg = C.upload(sg); Kb.outp = C.upload(outp); Kb.js = C.upload(js);
        return SQPHIP_OK;
    });
    if (rc) return rc;
    return nlp_block_commit(h, call.blk, call.kb, (long)N, d, (long)N, (long)N, nlp_lse_ws(N, R, d).size, A, cv, hs, weight, shift, Kb, blk_out);
}

// a Euclidean-norm row block (nlp_norm_dev.hpp): the checks of sqphip_nlp_add_lse_block, but any number of outputs may share a target
// row (nlp_block_targets); the targets with their outputs and Jacobian slots and the lists of the short and the long outputs are uploaded
extern "C" int sqphip_nlp_add_norm_block(sqphip_ctx *h, int64_t N, int32_t d, const int64_t *cols, const double *A, int32_t R,
                                         const int64_t *rows, const int64_t *seg, const double *shift, const double *weight,
                                         int32_t *blk_out)
{
    NlpBlockAdd call{h};
    if (int rc = call.begin("sqphip_nlp_add_norm_block")) return rc;
    Ctx &C0 = h->c;
    if (const std::string bad = nlp_block_shape(N, d, NLP_BLOCK_MAX_D); !bad.empty()) return call.fail(bad);
    if (!cols || !A) return call.fail("null cols or A");
    if (const std::string bad = nlp_block_segments(N, d, R, rows, seg); !bad.empty()) return call.fail(bad);
    std::vector<int> hs, cv;
    if (const std::string bad = nlp_block_columns(C0.nl.slots, d, cols, cv, hs); !bad.empty()) return call.fail(bad);
    NlpBlockTargets T;
    if (const std::string bad = nlp_block_targets(C0.nl.slots, C0.d.m, C0.d.nlin, R, rows, cv, T); !bad.empty()) return call.fail(bad);
    std::vector<int> sg((size_t)R + 1), outp((size_t)N), shortl, longl;
    for (int r = 0; r <= R; ++r) sg[r] = (int)seg[r];
    for (int r = 0; r < R; ++r) {
        for (int i = sg[r]; i < sg[r + 1]; ++i) outp[i] = r;
        (sg[r + 1] - sg[r] <= NLP_NORM_SHORT ? shortl : longl).push_back(r);
    }
    NlpBlkDev Kb = {};
    Kb.family = NLP_BLK_NORM;
    Kb.R = R; Kb.T = (int)T.trow.size(); Kb.nshort = (int)shortl.size(); Kb.nlong = (int)longl.size();
    if (shortl.empty()) shortl.push_back(0);      // (never read: an upload is not empty)
    if (longl.empty()) longl.push_back(0);
    const int rc = guarded(h, [&](Ctx &C) {
        Kb.tgt = C.upload(T.tgt); Kb.trow = C.upload(T.trow); Kb.tptr = C.upload(T.tptr); Kb.tout = C.upload(T.tout); Kb.js = C.upload(T.js);
        Kb.seg = C.upload(sg); Kb.outp = C.upload(outp); Kb.shortl = C.upload(shortl); Kb.longl = C.upload(longl);
        return SQPHIP_OK;
    });
    if (rc) return rc;
    return nlp_block_commit(h, call.blk, call.kb, (long)N, d, (long)N, (long)N, nlp_norm_ws(N, R, d).size, A, cv, hs, weight, shift, Kb, blk_out);
}

// weight / shift of block blk into the block of values v (of an instance or of a scenario of the queue); NULL: kept
static int nlp_block_put(sqphip_ctx *h, double *v, int32_t blk, const double *weight, const double *shift)
{
    return guarded(h, [&](Ctx &C) {
        const NlpHost::Block &K = C.nl.blk[blk];
        h2d(C, v + K.ow, weight, (size_t)K.nW); h2d(C, v + K.os, shift, (size_t)K.nS);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

static int nlp_block_check(sqphip_ctx *h, const std::string &who, int32_t blk)
{
    Ctx &C = h->c;
    if (!C.d.nlp) { C.err = who + ": the context has no factorable NLP attached (sqphip_nlp_attach*)"; return SQPHIP_EINVAL; }
    if (blk < 0 || blk >= (int)C.nl.blk.size()) {
        C.err = who + ": block " + std::to_string(blk) + " is outside the " + std::to_string(C.nl.blk.size()) + " of the context (sqphip_nlp_add_block)";
        return SQPHIP_EINVAL;
    }
    return SQPHIP_OK;
}

extern "C" int sqphip_nlp_set_instance_block(sqphip_ctx *h, int32_t inst, int32_t blk, const double *weight, const double *shift)
{
    const std::string who = "sqphip_nlp_set_instance_block";
    if (!h) return SQPHIP_EINVAL;
    if (int rc = nlp_block_check(h, who, blk)) return rc;
    if (int rc = instance_in_batch(h, who, inst)) return rc;
    return nlp_block_put(h, h->c.d.nlv + (size_t)inst * h->c.nl.nv, blk, weight, shift);
}

extern "C" int sqphip_nlp_stream_set_block(sqphip_ctx *h, int32_t scen, int32_t blk, const double *weight, const double *shift)
{
    const std::string who = "sqphip_nlp_stream_set_block";
    if (!h) return SQPHIP_EINVAL;
    if (int rc = nlp_block_check(h, who, blk)) return rc;
    if (!h->c.d.stream.val) { h->c.err = who + ": no NLP queue (sqphip_nlp_stream_begin)"; return SQPHIP_EINVAL; }
    if (int rc = scenario_in_queue(h, who, scen)) return rc;
    return nlp_block_put(h, const_cast<double *>(h->c.d.stream.val) + (size_t)scen * h->c.nl.nv, blk, weight, shift);
}

// ---- the queue on a QCQP or factorable-NLP context: a scenario is one block of values in the layout of DV::qcv / DV::nlv, so
// that the loader of the stage kernel (sqp_dev.hpp, b_sqp_stream) is one streaming copy; _run / _run_some / _assign / _append /
// _release / _get are shared.  The tables of a queue of n_scenarios blocks of nv doubles (nv < 0: of the ohm / c2 / c1 tables
// of an ACOPF context, sqphip_sqp_stream_begin):
int sqphip::stream_begin(sqphip_ctx *h, int32_t n_scenarios, int32_t keep_multipliers, long nv)
{
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        StreamDev Q = {};
        const size_t M = (size_t)n_scenarios;
        Q.M = n_scenarios;
        Q.next = C.dalloc<int>(1); Q.slot_scen = C.dalloc<int>((size_t)d.B);
        Q.qend = C.dalloc<int>(1);
        {   // hand-out order: identity, all M scenarios (sqphip_sqp_stream_assign changes it)
            std::vector<int> ids(M);
            for (size_t k = 0; k < M; ++k) ids[k] = (int)k;
            Q.qids = C.upload(ids);
            SQPHIP_HIP_OK(hipMemcpyAsync(Q.qend, &Q.M, sizeof(int), hipMemcpyHostToDevice, C.stream));
        }
        C.stream_started = false;
        Q.xL = C.dalloc<double>(M * d.n); Q.xU = C.dalloc<double>(M * d.n); Q.x0 = C.dalloc<double>(M * d.n);
        Q.gL = C.dalloc<double>(M * d.m); Q.gU = C.dalloc<double>(M * d.m);
        if (nv >= 0) Q.val = C.dalloc<double>(M * (size_t)nv);
        else { Q.ohm = C.dalloc<double>(M * d.nl * 12); Q.c2 = C.dalloc<double>(M * d.ng); Q.c1 = C.dalloc<double>(M * d.ng); }
        Q.rx = C.dalloc<double>(M * d.n); Q.robj = C.dalloc<double>(M);
        Q.rstat = C.dalloc<int>(M); Q.riter = C.dalloc<int>(M);
        if (keep_multipliers) {
            Q.rE = C.dalloc<double>(M * d.m); Q.rlam = C.dalloc<double>(M * d.m);
            Q.rmxL = C.dalloc<double>(M * d.n); Q.rmxU = C.dalloc<double>(M * d.n);
        }
        // every slot starts as "queue exhausted" (-1): the stage kernel's queue step stays off until
        // sqphip_sqp_stream_run arms the slots (-2), so a plain sqp_reset / sqp_run between _begin and _stream_run
        // behaves as if no queue existed (dalloc zero-fills, and 0 is a valid scenario id)
        SQPHIP_HIP_OK(hipMemsetAsync(Q.slot_scen, 0xff, sizeof(int) * (size_t)d.B, C.stream));
        // riter = -1: "no result filed by this context" (sqphip_sqp_stream_get; reset by _stream_run and _stream_assign)
        SQPHIP_HIP_OK(hipMemsetAsync(Q.riter, 0xff, sizeof(int) * M, C.stream));
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        d.stream = Q;
        make_lanes(C);
        return SQPHIP_OK;
    });
}

// the checks of a scenario that both value queues share (fn: the entry point, for the message); NULL bounds become those
// of sqphip_create
static int value_stream_check(sqphip_ctx *h, const char *fn, int32_t scen, const double *&xL, const double *&xU,
                              const double *&gL, const double *&gU, const double *x0)
{
    const std::string f(fn);
    if (int rc = scenario_in_queue(h, f, scen)) return rc;
    if (!x0) { h->c.err = f + ": x0 is NULL (a scenario needs its start)"; return SQPHIP_EINVAL; }
    if (!xL) xL = h->c.h_xL.data();
    if (!xU) xU = h->c.h_xU.data();
    if (!gL) gL = h->c.h_gL.data();
    if (!gU) gU = h->c.h_gU.data();
    for (int i = 0; i < h->c.d.m; ++i) {
        if (gL[i] == -INFINITY && gU[i] == INFINITY) {
            h->c.err = f + ": row " + std::to_string(i) + " is unbounded on both sides";
            return SQPHIP_EINVAL;
        }
        if (h->c.d.condense && gL[i] == gU[i] && h->c.h_kpos[i] < 0) {
            h->c.err = f + ": row " + std::to_string(i) + " is an equality for this scenario but was not one when "
                       "the context was created (options.kkt_condense = 1 fixes the kept rows)";
            return SQPHIP_EINVAL;
        }
    }
    return SQPHIP_OK;
}

// ... and the upload: bounds, start and the block v of nv values
static int value_stream_upload(sqphip_ctx *h, int32_t scen, const double *xL, const double *xU, const double *gL,
                               const double *gU, const double *x0, const std::vector<double> &v)
{
    return guarded(h, [&](Ctx &C) {
        DV &d = C.d;
        const StreamDev &Q = d.stream;
        const size_t s = (size_t)scen;
        h2d(C, const_cast<double *>(Q.xL) + s * d.n, xL, d.n); h2d(C, const_cast<double *>(Q.xU) + s * d.n, xU, d.n);
        h2d(C, const_cast<double *>(Q.x0) + s * d.n, x0, d.n);
        h2d(C, const_cast<double *>(Q.gL) + s * d.m, gL, d.m); h2d(C, const_cast<double *>(Q.gU) + s * d.m, gU, d.m);
        h2d(C, const_cast<double *>(Q.val) + s * v.size(), v.data(), v.size());
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}

extern "C" int sqphip_qcqp_stream_begin(sqphip_ctx *h, int32_t n_scenarios, int32_t keep_multipliers)
{
    if (!h) return SQPHIP_EINVAL;
    if (!h->c.d.qc) { h->c.err = "sqphip_qcqp_stream_begin: the context has no QCQP attached (sqphip_qcqp_attach)"; return SQPHIP_EINVAL; }
    if (n_scenarios <= 0) { h->c.err = "sqphip_qcqp_stream_begin: n_scenarios must be positive"; return SQPHIP_EINVAL; }
    return stream_begin(h, n_scenarios, keep_multipliers, h->c.qc.nv);
}

extern "C" int sqphip_qcqp_stream_set(sqphip_ctx *h, int32_t scen, const double *xL, const double *xU, const double *gL,
                                      const double *gU, const double *f0, const double *c, const double *q0v,
                                      const double *g0, const double *av, const double *qv, const double *x0)
{
    if (!h) return SQPHIP_EINVAL;
    if (!h->c.d.qc || !h->c.d.stream.val) { h->c.err = "sqphip_qcqp_stream_set: no QCQP queue (sqphip_qcqp_stream_begin)"; return SQPHIP_EINVAL; }
    if (int rc = value_stream_check(h, "sqphip_qcqp_stream_set", scen, xL, xU, gL, gU, x0)) return rc;
    // the scenario's block: the values of the attach, overlaid with the parts given (f0 | c | Q0 | g0 | A | Q)
    std::vector<double> v(h->c.qc.base);
    const long *o = h->c.qc.off;
    const double *src[6] = {f0, c, q0v, g0, av, qv};
    for (int k = 0; k < 6; ++k) if (src[k]) std::copy(src[k], src[k] + (o[k + 1] - o[k]), v.begin() + o[k]);
    return value_stream_upload(h, scen, xL, xU, gL, gU, x0, v);
}

// ---- the queue on a factorable-NLP context: the same tables, the block in the layout of DV::nlv (f0 | g0 | c, on a context
// of sqphip_nlp_attach_data | b | a | p; padded to even)
extern "C" int sqphip_nlp_stream_begin(sqphip_ctx *h, int32_t n_scenarios, int32_t keep_multipliers)
{
    if (!h) return SQPHIP_EINVAL;
    if (!h->c.d.nlp) { h->c.err = "sqphip_nlp_stream_begin: the context has no factorable NLP attached (sqphip_nlp_attach)"; return SQPHIP_EINVAL; }
    if (n_scenarios <= 0) { h->c.err = "sqphip_nlp_stream_begin: n_scenarios must be positive"; return SQPHIP_EINVAL; }
    h->c.nl.started = true;
    return stream_begin(h, n_scenarios, keep_multipliers, h->c.nl.nv);
}

extern "C" int sqphip_nlp_stream_set(sqphip_ctx *h, int32_t scen, const double *xL, const double *xU, const double *gL,
                                     const double *gU, const double *f0, const double *g0, const double *tcoef,
                                     const double *x0)
{
    if (!h) return SQPHIP_EINVAL;
    if (!h->c.d.nlp || !h->c.d.stream.val) { h->c.err = "sqphip_nlp_stream_set: no NLP queue (sqphip_nlp_stream_begin)"; return SQPHIP_EINVAL; }
    if (int rc = value_stream_check(h, "sqphip_nlp_stream_set", scen, xL, xU, gL, gU, x0)) return rc;
    // the scenario's block: the values of the attach, overlaid with the parts given
    std::vector<double> v(h->c.nl.base);
    const long m = h->c.d.m;
    if (f0) v[0] = *f0;
    if (g0) std::copy(g0, g0 + m, v.begin() + 1);
    if (tcoef) std::copy(tcoef, tcoef + h->c.nl.nterms, v.begin() + 1 + m);
    return value_stream_upload(h, scen, xL, xU, gL, gU, x0, v);
}

extern "C" int sqphip_nlp_stream_set_data(sqphip_ctx *h, int32_t scen, const double *fshift, const double *acoef, const double *fpar)
{
    const char *who = "sqphip_nlp_stream_set_data";
    if (!h) return SQPHIP_EINVAL;
    if (int rc = nlp_data_refused(h, who, nullptr, nullptr, nullptr)) return rc;
    if (!h->c.d.stream.val) { h->c.err = std::string(who) + ": no NLP queue (sqphip_nlp_stream_begin)"; return SQPHIP_EINVAL; }
    if (int rc = scenario_in_queue(h, who, scen)) return rc;
    if (int rc = nlp_data_refused(h, who, fshift, acoef, fpar)) return rc;
    return guarded(h, [&](Ctx &C) {
        nlp_data_upload(C, const_cast<double *>(C.d.stream.val) + (size_t)scen * C.nl.nv, fshift, acoef, fpar);
        SQPHIP_HIP_OK(hipStreamSynchronize(C.stream));
        return SQPHIP_OK;
    });
}
