// norm_targets_smoke.cpp -- nlp_block_targets (csrc/model_plans.cpp), the plan builder of sqphip_nlp_add_norm_block, on its own:
// built with the host sanitizers together with model_plans.cpp and run as a child process by tests/test_norm_targets_cpu.py.
// Prints "ok" and returns 0, or names the first check that failed and returns 1.
#include "../sqpsolver.jl_amd/csrc/model_plans.hpp"

#include <cstdio>
#include <string>
#include <vector>

using namespace sqphip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("failed line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static bool has(const std::string &s, const char *w) { return s.find(w) != std::string::npos; }

int main()
{
    // n = 6 variables, m = 5 rows, row 1 linear.  Jacobian: rows 2 and 4 hold the columns 2, 4, 5 (row 4 has (4, 2) twice: the
    // first copy owns the slot); row 3 lacks (3, 5); row 5 has none.
    const int64_t n = 6, m = 5, nlin = 1;
    const std::vector<int64_t> jrow = {1, 2, 2, 2, 3, 3, 4, 4, 4, 4}, jcol = {1, 5, 2, 4, 2, 4, 2, 2, 5, 4};
    const StructureSlots S(n, (int64_t)jrow.size(), jrow.data(), jcol.data(), 0, nullptr, nullptr);
    const std::vector<int> cv = {1, 3, 4};          // variables 2, 4, 5, 0-based
    NlpBlockTargets T;

    {   // first-appearance order, CSR contents, slots
        const std::vector<int64_t> rows = {4, 0, 2, 4, 0, 0, 2};
        const std::string e = nlp_block_targets(S, m, nlin, (int)rows.size(), rows.data(), cv, T);
        CHECK(e.empty());
        CHECK((T.trow == std::vector<int>{4, 0, 2}));
        CHECK((T.tgt == std::vector<int>{0, 1, 2, 0, 1, 1, 2}));
        CHECK((T.tptr == std::vector<int>{0, 2, 5, 7}));
        CHECK((T.tout == std::vector<int>{0, 3, 1, 4, 5, 2, 6}));
        CHECK((T.js == std::vector<int>{6, 9, 8, -1, -1, -1, 2, 3, 1}));
    }
    {   // one output; every output on the objective
        const std::vector<int64_t> one = {2}, obj = {0, 0, 0};
        CHECK(nlp_block_targets(S, m, nlin, 1, one.data(), cv, T).empty());
        CHECK((T.trow == std::vector<int>{2}) && (T.tptr == std::vector<int>{0, 1}) && (T.tout == std::vector<int>{0}) && (T.js == std::vector<int>{2, 3, 1}));
        CHECK(nlp_block_targets(S, m, nlin, 3, obj.data(), cv, T).empty());
        CHECK((T.trow == std::vector<int>{0}) && (T.tgt == std::vector<int>{0, 0, 0}) && (T.tptr == std::vector<int>{0, 3}) &&
              (T.tout == std::vector<int>{0, 1, 2}) && (T.js == std::vector<int>{-1, -1, -1}));
    }
    {   // the refusals
        const std::vector<int64_t> high = {0, 6}, neg = {-1}, lin = {2, 1}, miss = {2, 2, 3}, none = {0, 5};
        std::string e = nlp_block_targets(S, m, nlin, 2, high.data(), cv, T);
        CHECK(has(e, "output 2: row 6") && has(e, "outside 0..5"));
        e = nlp_block_targets(S, m, nlin, 1, neg.data(), cv, T);
        CHECK(has(e, "output 1: row -1") && has(e, "outside 0..5"));
        e = nlp_block_targets(S, m, nlin, 2, lin.data(), cv, T);
        CHECK(has(e, "output 2: row 1") && has(e, "num_linear = 1"));
        e = nlp_block_targets(S, m, nlin, 3, miss.data(), cv, T);
        CHECK(has(e, "output 3: row 3") && has(e, "column 3") && has(e, "Jacobian entry (3, 5)"));
        e = nlp_block_targets(S, m, nlin, 2, none.data(), cv, T);
        CHECK(has(e, "output 2: row 5") && has(e, "column 1") && has(e, "Jacobian entry (5, 2)"));
    }
    {   // R = 5000 outputs on three targets
        const int R = 5000;
        std::vector<int64_t> rows((size_t)R);
        const int64_t pick[3] = {2, 0, 4};
        for (int r = 0; r < R; ++r) rows[r] = pick[(r * 7 + r / 3) % 3];
        CHECK(nlp_block_targets(S, m, nlin, R, rows.data(), cv, T).empty());
        CHECK(T.trow.size() == 3 && T.tptr.size() == 4 && T.tptr[0] == 0 && T.tptr[3] == R && (int)T.tout.size() == R && T.js.size() == 9);
        std::vector<int> seen((size_t)R, 0);
        for (int t = 0; t < 3; ++t)
            for (int k = T.tptr[t]; k < T.tptr[t + 1]; ++k) {
                const int r = T.tout[k];
                CHECK(r >= 0 && r < R);
                if (r < 0 || r >= R) break;
                ++seen[r];
                CHECK(T.tgt[r] == t && rows[r] == T.trow[t]);
                CHECK(k == T.tptr[t] || T.tout[k - 1] < r);
            }
        for (int r = 0; r < R; ++r) CHECK(seen[r] == 1);
        CHECK(T.trow[0] == (int)rows[0]);
    }
    if (fails == 0) std::printf("ok\n");
    return fails != 0;
}
