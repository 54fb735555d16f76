// tests/launch_plan_dump.cpp -- prints what param_amd/csrc/launch_plan.h plans (tests/test_launch_plan_host.py builds and runs it).
// stdin: one case per line, 27 integers --
//   kind (0 base, 1 forward, 2 quantized, 3 padded with 4-byte output elements, 4 padded with 2-byte ones; 5 the row gather,
//         which prints the eight members of pm::GatherPlan instead; 6 / 7 the FP8 pooled lookup with 4- / 2-byte output elements;
//         8 the FP8 row gather, eight members as 5 -- for 6 .. 8 dtype is PM_F8E4M3 / PM_F8E5M2; the scaled FP8 lookups plan on 6 .. 8
//         too, their pooled plan being plan_f8 followed by f8s_stage_out, which tests/plan_sweep.py restates;
//         9 / 10 the mixed-format pooled lookup with 4- / 2-byte output elements; 11 the mixed-format row gather, eight members as 5)
//   the request: num_tables batch num_indices bag_begin bag_count max_dim min_dim dtype weighted table_group grad_block_shift grad_block_extra
//   what the setters were given: unroll bags_per_block xcd_affine nt_loads | stage_out flat_grid flat_target
//   the environment's values: stage flat flat_maxl flat_target flat_bags tile_major flat_compact
// stdout: one line per case, the twelve members of pm::LaunchPlan in their order.
#include <stdio.h>

#include "launch_plan.h"

int main() {
    for (;;) {
        long long v[27];
        for (int i = 0; i < 27; ++i)
            if (scanf("%lld", &v[i]) != 1) return i == 0 ? 0 : 1;
        pm_embbag_batch op = {};
        op.num_tables = static_cast<int32_t>(v[1]);
        op.batch = v[2];
        op.num_indices = v[3];
        op.bag_begin = v[4];
        op.bag_count = v[5];
        op.max_dim = static_cast<int32_t>(v[6]);
        op.min_dim = static_cast<int32_t>(v[7]);
        op.weight_dtype = static_cast<int32_t>(v[8]);
        op.index_dtype = PM_I64;
        static const float some_weight = 1.0f;
        op.per_sample_weights = v[9] ? &some_weight : nullptr;   // (the plan asks only whether there are any)
        op.out_stride = op.max_dim;
        op.table_group = static_cast<int32_t>(v[10]);
        op.grad_block_shift = static_cast<int32_t>(v[11]);
        op.grad_block_extra = v[12];
        pm::TuningSetters s;
        s.unroll = static_cast<int>(v[13]);
        s.bags_per_block = static_cast<int>(v[14]);
        s.xcd_affine = static_cast<int>(v[15]);
        s.nt_loads = static_cast<int>(v[16]);
        s.stage_out = static_cast<int>(v[17]);
        s.flat_grid = static_cast<int>(v[18]);
        s.flat_target = static_cast<int>(v[19]);
        pm::FwdEnv e;
        e.stage = static_cast<int>(v[20]);
        e.flat = static_cast<int>(v[21]);
        e.flat_maxl = static_cast<int>(v[22]);
        e.flat_target = static_cast<int>(v[23]);
        e.flat_bags = static_cast<int>(v[24]);
        e.tile_major = static_cast<int>(v[25]);
        e.flat_compact = static_cast<int>(v[26]);
        const pm::PlanKnobs k = pm::resolve_knobs(s, e);
        pm::LaunchPlan p;
        switch (v[0]) {
            case 0: p = pm::plan_base(op, op.weight_dtype, k); break;
            case 1: p = pm::plan_forward(op, op.weight_dtype, k); break;
            case 2: p = pm::plan_quantized(op, op.weight_dtype, k); break;
            case 3: p = pm::plan_padded(op, op.weight_dtype, k, 4); break;
            case 4: p = pm::plan_padded(op, op.weight_dtype, k, 2); break;
            case 5: {
                const pm::GatherPlan g = pm::plan_gather(op, op.weight_dtype, k);
                printf("%d %d %d %d %d %d %d %lld\n", g.vec, g.group_lanes, g.tile, g.col_passes, g.unroll, g.lds_borders, g.xcd_contiguous,
                       static_cast<long long>(g.grid));
                continue;
            }
            case 6: p = pm::plan_f8(op, k, 4); break;
            case 7: p = pm::plan_f8(op, k, 2); break;
            case 8: {
                const pm::GatherPlan g = pm::plan_gather_f8(op, k);
                printf("%d %d %d %d %d %d %d %lld\n", g.vec, g.group_lanes, g.tile, g.col_passes, g.unroll, g.lds_borders, g.xcd_contiguous,
                       static_cast<long long>(g.grid));
                continue;
            }
            case 9: p = pm::plan_anyfmt(op, pm::anyfmt_shape(op, k), k, 4); break;
            case 10: p = pm::plan_anyfmt(op, pm::anyfmt_shape(op, k), k, 2); break;
            case 11: {
                const pm::GatherPlan g = pm::plan_gather_anyfmt(op, k);
                printf("%d %d %d %d %d %d %d %lld\n", g.vec, g.group_lanes, g.tile, g.col_passes, g.unroll, g.lds_borders, g.xcd_contiguous,
                       static_cast<long long>(g.grid));
                continue;
            }
            default: return 2;
        }
        printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", p.tiles_per_table, p.bags_per_block, p.idx_cap, p.xcd_affine, p.nt_loads, p.ordered,
               p.stage_out, p.stage_bags, p.flat_bags, p.flat_target, p.flat_compact, p.unroll);
    }
}
