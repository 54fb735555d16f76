// tests/qrows_plan_dump.cpp -- prints what param_amd/csrc/launch_plan.h plans for pm_embbag_fwd_qrows (tests/test_qrows_host.py builds it
// with -fsanitize=address,undefined and runs it: plan_qrows is pure host code).
// stdin: one request per line, 14 integers --
//   bits num_tables batch num_indices max_dim min_dim weighted bag_begin bag_count out_bytes | pm_set_tuning's unroll bags_per_block |
//   pm_set_forward_tuning's stage_out | lane dwords the caller expects (checked against kQrowsLaneDwords)
// stdout: one line per request, the twelve members of pm::LaunchPlan in their order.
#include <stdio.h>

#include "launch_plan.h"

int main() {
    for (;;) {
        long long v[14];
        for (int i = 0; i < 14; ++i)
            if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;
        if (v[13] != pm::kQrowsLaneDwords) return 3;
        pm_embbag_batch op = {};
        op.num_tables = static_cast<int32_t>(v[1]);
        op.batch = v[2];
        op.num_indices = v[3];
        op.max_dim = static_cast<int32_t>(v[4]);
        op.min_dim = static_cast<int32_t>(v[5]);
        op.index_dtype = PM_I64;
        static const float some_weight = 1.0f;
        op.per_sample_weights = v[6] ? &some_weight : nullptr;   // (the plan asks only whether there are any)
        op.bag_begin = v[7];
        op.bag_count = v[8];
        op.out_stride = static_cast<int64_t>(op.max_dim) * op.num_tables;
        pm::TuningSetters s;
        s.unroll = static_cast<int>(v[10]);
        s.bags_per_block = static_cast<int>(v[11]);
        s.stage_out = static_cast<int>(v[12]);
        const pm::PlanKnobs k = pm::resolve_knobs(s, pm::FwdEnv());
        const pm::LaunchPlan p = pm::plan_qrows(op, static_cast<int>(v[0]), k, static_cast<int>(v[9]));
        printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", p.tiles_per_table, p.bags_per_block, p.idx_cap, p.xcd_affine, p.nt_loads, p.ordered,
               p.stage_out, p.stage_bags, p.flat_bags, p.flat_target, p.flat_compact, p.unroll);
    }
}
