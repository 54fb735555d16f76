// tests/qgather_plan_dump.cpp -- prints what param_amd/csrc/launch_plan.h plans for pm_embedding_gather_qrows (tests/test_qgather_host.py
// builds it with -fsanitize=address,undefined and runs it: plan_gather_qrows is pure host code).
// stdin: one request per line, 7 integers --
//   bits num_tables num_indices max_dim | pm_set_tuning's unroll xcd_affine | lane dwords the caller expects (checked against kQrowsLaneDwords)
// stdout: one line per request, the eight members of pm::GatherPlan in their order, then how many positions of [0, num_indices) lie in
// exactly one tile when every block of the grid takes the tile gather_block_tile gives it (the kernel's own mapping).
#include <stdio.h>

#include <vector>

#include "launch_plan.h"

int main() {
    for (;;) {
        long long v[7];
        for (int i = 0; i < 7; ++i)
            if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;
        if (v[6] != pm::kQrowsLaneDwords) return 3;
        pm_embbag_batch op = {};
        op.num_tables = static_cast<int32_t>(v[1]);
        op.batch = 1;
        op.bag_count = 1;
        op.num_indices = v[2];
        op.max_dim = static_cast<int32_t>(v[3]);
        op.index_dtype = PM_I64;
        pm::TuningSetters s;
        s.unroll = static_cast<int>(v[4]);
        s.xcd_affine = static_cast<int>(v[5]);
        const pm::GatherPlan g = pm::plan_gather_qrows(op, static_cast<int>(v[0]), pm::resolve_knobs(s, pm::FwdEnv{}));
        std::vector<int> hits(static_cast<size_t>(op.num_indices), 0);
        for (int64_t b = 0; b < g.grid; ++b) {
            const int64_t j0 = pm::gather_block_tile(b, g.grid, g.xcd_contiguous != 0) * g.tile;
            for (int64_t j = j0; j < j0 + g.tile && j < op.num_indices; ++j)
                if (j >= 0) ++hits[static_cast<size_t>(j)];
        }
        long long once = 0;
        for (int h : hits) once += h == 1;
        printf("%d %d %d %d %d %d %d %lld %lld\n", g.vec, g.group_lanes, g.tile, g.col_passes, g.unroll, g.lds_borders, g.xcd_contiguous,
               static_cast<long long>(g.grid), once);
    }
}
