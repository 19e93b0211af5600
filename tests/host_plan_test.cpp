// The plan builder on the host: reads pattern sets from stdin (plan_digest.h: one line each) and prints every plan's
// structure and digest.  Built with g++ from this file and csrc/apm_plan.cpp alone (tests/test_host_logic.py).
#include "../include/apm.h"
#include "apm_plan.h"
#include "plan_digest.h"

int main() {
    PlanRequest r;
    while (plan_read_request(stdin, &r)) {
        std::vector<PatternInfo> pats(r.pats.size());
        for (size_t i = 0; i < pats.size(); ++i) {
            pats[i].bytes = r.pats[i];
            pats[i].m = (int)r.pats[i].size();
        }
        ApmPlan plan;
        std::string err;
        const int rc = apm_build_plan(pats, r.k, r.kernel, &plan, &err);
        plan_report(stdout, r.name.c_str(), rc, err, pats, plan.tiled, plan.sieve, plan.tails, plan.stails, plan.wtails, plan.xtails, plan.longs,
                    plan.trivial, plan.allpat, plan.m_max);
    }
    return 0;
}
