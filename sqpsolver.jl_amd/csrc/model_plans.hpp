// model_plans.hpp -- the host-side model compilers of sqphip_qcqp_attach and sqphip_nlp_attach*: index checks, structure
// lookups and the gather plans (CSR by owner, indices only) that qcqp_dev.hpp / nlp_dev.hpp evaluate.  Plain C++17 without
// any HIP header, so that it builds and runs without a device (tests/plan_smoke.cpp).  The device sums every output entry
// over its plan row in plan order: the order in which entries are produced here is part of the results' bits.
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

namespace sqphip {

// the menu of a factor (nlp_dev.hpp); fke = kind + 16 * (exponent + 32)
enum { NLP_POW = 0, NLP_SIN = 1, NLP_COS = 2, NLP_EXP = 3, NLP_LOG = 4,
       NLP_SQRT = 5, NLP_TANH = 6, NLP_ATAN = 7, NLP_SIGMOID = 8, NLP_SOFTPLUS = 9, NLP_POWR = 10 };
enum { NLP_KIND_BITS = 4, NLP_KIND_MASK = (1 << NLP_KIND_BITS) - 1 };

// first COO slot of every structural entry of sqphip_create (1-based arrays; later duplicates get no plan entries: they
// stay 0 and gather_csc sums them); -1: the structure lacks the entry.  The Hessian is looked up in either triangle.
struct StructureSlots {
    int64_t n = 0, nnzJ = 0, nnzH = 0;
    StructureSlots() {}
    StructureSlots(int64_t n, int64_t nnzJ, const int64_t *jrow, const int64_t *jcol, int64_t nnzH, const int64_t *hrow, const int64_t *hcol);
    int jfind(int64_t i, int64_t j) const { auto it = jslot.find(i * n + j); return it == jslot.end() ? -1 : it->second; }
    int hfind(int64_t r, int64_t c) const
    {
        auto it = hslot.find((r > c ? r : c) * n + (r > c ? c : r));
        return it == hslot.end() ? -1 : it->second;
    }
private:
    std::unordered_map<int64_t, int> jslot, hslot;
};

// owners of a plan's entries (in production order) -> CSR row pointers and the stable order of the entries by owner
void csr_by_owner(int owners, const std::vector<int> &own, std::vector<int> &ptr, std::vector<int> &ord);
// the row pointers of the row / variable / Jacobian / Hessian plans back to back; fp, jp, hp: where the last three start
std::vector<int> pack_ptrs(const std::vector<int> &g, const std::vector<int> &f, const std::vector<int> &j, const std::vector<int> &h,
                           int &fp, int &jp, int &hp);

// What a context keeps of an attached QCQP (empty, nv = 0: none).  Values of an instance: f0 | c | Q0 | g0 | A | Q.
struct QcqpHost {
    long nv = 0;                          // doubles per instance (DV::qcv; even: the blocks are 16-byte aligned, b_sqp_stream)
    long off[7] = {};                     // where the parts start: f0, c, Q0, g0, A, Q, end (= the doubles in use)
    std::vector<double> base;             // [nv] the values given to sqphip_qcqp_attach (NULL parts of a queue scenario)
};
// ... and what the attach uploads: the scalar fields of QcqpDev and its arrays; int2 / int4 entries flat, 2 / 4 ints each
struct QcqpPlan {
    int n, m, nq0, f_ptr, j_ptr, h_ptr;
    std::vector<int> ptr, q0, ge, fe, je, he;      // q0, fe, je, he: 2 per entry; ge: 4
    QcqpHost host;
};
// SQPHIP_OK, or SQPHIP_EINVAL with the message ("who: ...") in err
int build_qcqp_plan(const StructureSlots &S, int64_t m, int64_t nlin, const char *who, int64_t nnzQ0, const int64_t *q0r,
                    const int64_t *q0c, const double *q0v, int64_t nnzA, const int64_t *ar, const int64_t *ac, const double *av,
                    int64_t nnzQ, const int64_t *qi, const int64_t *qr, const int64_t *qc, const double *qv, const double *c,
                    const double *g0, double f0, QcqpPlan &P, std::string &err);

// What a context keeps of an attached factorable NLP (empty, nv = 0: none).  Values of an instance: f0 | g0 | c, with data
// | b [nfac] | a [nargs] | p [nfac, with a POWR factor only] at ob, oa, op (-1: no p), then W_k [N_k] | S_k [nS_k] of every
// dense data block (sqphip_nlp_add_block; nS: N, Kf N for a softmax block; nW: N, R N for a block with R outputs,
// sqphip_nlp_add_row_block), padded to even.
struct NlpHost {
    long nv = 0, nfac = 0, nterms = 0, nargs = 0;
    long end = 0, ws = 0;                 // doubles in use before the padding; doubles of workspace per instance (DV::nlw)
    bool data = false;                    // sqphip_nlp_attach_data
    long ob = 0, oa = 0, op = -1;
    std::vector<double> base;             // [nv] the values given to the attach (NULL parts of a queue scenario)
    std::vector<int> tptr, aptr, kind;    // [nterms + 1], [nfac + 1], [nfac]: what nlp_data_check needs of the structure
    std::vector<int> lin_terms;           // the terms of rows 1..num_linear
    struct Block { long N, ow, os, nS, nW; };
    std::vector<Block> blk;
    bool started = false;                 // a reset, run or queue has seen the layout, which is final from then on
    StructureSlots slots;                 // for the columns of the blocks
};
struct NlpPlan {
    int n, m, nobj, f_ptr, j_ptr, h_ptr, multi;
    std::vector<int> ptr, fvar, fke, ot, ge, fe, je, he, avar;    // fe, je: 2 per entry; he: 4
    std::vector<double> fab, acoef, aw, fpar;                      // fab: 2 per factor (a, b)
    NlpHost host;
};
// The four entry points differ in these.  !affine: aptr is null and factor k has the one argument avar[k] with coefficient
// acoef[k].  last_kind: the menu ends at LOG (sqphip_nlp_attach, _affine) or POWR.  distinct: the factors of a term sit on
// distinct variables (the two older calls).  data: b | a | p appended to every instance's block (NlpDev::data).
struct NlpOptions { bool affine; int last_kind; bool distinct, data; };
int build_nlp_plan(const StructureSlots &S, int64_t m, int64_t nlin, const char *who, const NlpOptions &O, int64_t nterms,
                   const int64_t *trow, const double *tcoef, const int64_t *tptr, const int64_t *aptr, const int64_t *avar,
                   const double *acoef, const int32_t *fkind, const int32_t *fexp, const double *fpar, const double *fshift,
                   const double *g0, double f0, NlpPlan &P, std::string &err);

// what sqphip_nlp_set_instance_data and sqphip_nlp_stream_set_data refuse of the data of one instance (NULL: kept, unchecked:
// what an instance holds has passed these checks).  Returns the complaint ("who: ..."), empty when there is none.
std::string nlp_data_check(const NlpHost &H, int64_t nlin, const char *who, const double *fshift, const double *acoef, const double *fpar);

// cols [D] 1-based, in range and distinct, to cv (0-based), and the COO slot of every lower entry (r, c) of a block's
// D x D Hessian to hs (-1 throughout when nnzH = 0).  Returns the complaint, empty when there is none.
std::string nlp_block_columns(const StructureSlots &S, int D, const int64_t *cols, std::vector<int> &cv, std::vector<int> &hs);

// rows [R] of a block with several outputs (0: the objective, i: row i, distinct, none of the rows 1..nlin) to row, and the
// Jacobian COO slot of every (rows[r], cv[j]) to js [R][d] (-1 for an output on row 0).  Returns the complaint, empty when
// there is none.
std::string nlp_block_rows(const StructureSlots &S, int64_t m, int64_t nlin, int R, const int64_t *rows, const std::vector<int> &cv,
                           int *row, std::vector<int> &js);

// rows [R] of a block whose outputs may share a target (0: the objective, i: row i, none of the rows 1..nlin; a row may be the
// target of any number of outputs): the distinct targets in order of first appearance to trow [T], the target of every output to
// tgt [R] (0 .. T - 1), the outputs of a target in rising order as a CSR list to tptr [T + 1] / tout [R], and the Jacobian COO
// slot of every (trow[t], cv[j]) to js [T][d] (-1 for the target row 0).  Linear in R.  Returns the complaint, empty when there is
// none.
struct NlpBlockTargets { std::vector<int> tgt, trow, tptr, tout, js; };
std::string nlp_block_targets(const StructureSlots &S, int64_t m, int64_t nlin, int R, const int64_t *rows, const std::vector<int> &cv,
                              NlpBlockTargets &T);

}  // namespace sqphip
