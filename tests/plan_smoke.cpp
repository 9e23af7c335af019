// plan_smoke.cpp -- the host-side model compilers of csrc/model_plans.cpp on their own (no device, no library): reads one model
// from a text file, prints the plan or the error message.  tests/test_model_plans_cpu.py compiles it together with
// model_plans.cpp under the address and undefined-behaviour sanitizers and checks what it prints.
//   file:   "model qcqp|nlp|block" and "who <entry point>", then lines "name count v1 v2 ..." (count -1: a null pointer;
//           doubles as C99 hex floats)
//   output: "rc 1 <code>", then "err <message>" or the fields of the plan, one per line in the same format
#include "../sqpsolver.jl_amd/csrc/model_plans.hpp"
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>

using namespace sqphip;

namespace {

struct Arr { bool null = true; std::vector<int64_t> i; std::vector<int32_t> i32; std::vector<double> d; };
std::map<std::string, Arr> in;
std::map<std::string, std::string> word;

const int64_t *I(const char *k) { return in[k].null ? nullptr : in[k].i.data(); }
const int32_t *I32(const char *k) { return in[k].null ? nullptr : in[k].i32.data(); }
const double *D(const char *k) { return in[k].null ? nullptr : in[k].d.data(); }
int64_t S(const char *k) { return in.at(k).i.at(0); }

void put(const char *name, const std::vector<int> &v)
{
    std::printf("%s %zu", name, v.size());
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}
void put(const char *name, const std::vector<double> &v)
{
    std::printf("%s %zu", name, v.size());
    for (double x : v) std::printf(" %a", x);
    std::printf("\n");
}
void put(const char *name, long v) { std::printf("%s 1 %ld\n", name, v); }

int done(int rc, const std::string &err)
{
    std::printf("rc 1 %d\n", rc);
    if (rc) std::printf("err %s\n", err.c_str());
    return rc;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: plan_smoke <model file>\n"); return 2; }
    std::ifstream f(argv[1]);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string name, tok;
        long count = 0;
        if (!(ss >> name)) continue;
        if (name == "model" || name == "who") { ss >> word[name]; continue; }
        ss >> count;
        Arr &a = in[name];
        a.null = count < 0;
        for (long k = 0; k < count && (ss >> tok); ++k) {
            a.d.push_back(std::strtod(tok.c_str(), nullptr));
            a.i.push_back(std::strtoll(tok.c_str(), nullptr, 10));
            a.i32.push_back((int32_t)a.i.back());
        }
        if ((long)a.d.size() != (count < 0 ? 0 : count)) { std::fprintf(stderr, "plan_smoke: %s: short line\n", name.c_str()); return 2; }
    }
    const StructureSlots slots(S("n"), (int64_t)in["jrow"].i.size(), I("jrow"), I("jcol"), (int64_t)in["hrow"].i.size(), I("hrow"), I("hcol"));
    const char *who = word["who"].c_str();
    std::string err;
    if (word["model"] == "qcqp") {
        QcqpPlan P;
        const int rc = build_qcqp_plan(slots, S("m"), S("nlin"), who, S("nnzQ0"), I("q0r"), I("q0c"), D("q0v"), S("nnzA"), I("ar"), I("ac"),
                                       D("av"), S("nnzQ"), I("qi"), I("qr"), I("qc"), D("qv"), D("c"), D("g0"), in.at("f0").d.at(0), P, err);
        if (done(rc, err)) return 0;
        put("n", P.n); put("m", P.m); put("nq0", P.nq0); put("f_ptr", P.f_ptr); put("j_ptr", P.j_ptr); put("h_ptr", P.h_ptr);
        put("nv", P.host.nv); put("off", std::vector<int>(P.host.off, P.host.off + 7));
        put("ptr", P.ptr); put("q0", P.q0); put("ge", P.ge); put("fe", P.fe); put("je", P.je); put("he", P.he); put("base", P.host.base);
    } else if (word["model"] == "nlp") {
        NlpPlan P;
        const NlpOptions O = {S("affine") != 0, (int)S("last_kind"), S("distinct") != 0, S("data") != 0};
        const int rc = build_nlp_plan(slots, S("m"), S("nlin"), who, O, S("nterms"), I("trow"), D("tcoef"), I("tptr"), I("aptr"), I("avar"),
                                      D("acoef"), I32("fkind"), I32("fexp"), D("fpar"), D("fshift"), D("g0"), in.at("f0").d.at(0), P, err);
        if (done(rc, err)) return 0;
        const NlpHost &H = P.host;
        put("n", P.n); put("m", P.m); put("nobj", P.nobj); put("f_ptr", P.f_ptr); put("j_ptr", P.j_ptr); put("h_ptr", P.h_ptr);
        put("multi", P.multi); put("nv", H.nv); put("nfac", H.nfac); put("nterms", H.nterms); put("nargs", H.nargs); put("end", H.end);
        put("ws", H.ws); put("data", H.data); put("ob", H.ob); put("oa", H.oa); put("op", H.op);
        put("ptr", P.ptr); put("fvar", P.fvar); put("fke", P.fke); put("ot", P.ot); put("ge", P.ge); put("fe", P.fe); put("je", P.je);
        put("he", P.he); put("avar", P.avar); put("tptr", H.tptr); put("aptr", H.aptr); put("kind", H.kind); put("lin_terms", H.lin_terms);
        put("fab", P.fab); put("acoef", P.acoef); put("aw", P.aw); put("fpar", P.fpar); put("base", H.base);
        if (in.count("check"))     // the data of one instance against the plan's host part, under the name given as "who"
            std::printf("check %s\n", nlp_data_check(H, S("nlin"), who, D("chk_fshift"), D("chk_acoef"), D("chk_fpar")).c_str());
    } else if (word["model"] == "block") {
        std::vector<int> cv, hs;
        err = nlp_block_columns(slots, (int)in["cols"].i.size(), I("cols"), cv, hs);
        if (done(err.empty() ? 0 : -1, err)) return 0;
        put("cv", cv); put("hs", hs);
    } else { std::fprintf(stderr, "plan_smoke: unknown model\n"); return 2; }
    return 0;
}
