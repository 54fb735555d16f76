// tests/drain_split_dump.cpp -- prints the forward's split last round as param_amd/csrc/launch_plan.h computes it
// (tests/test_drain_split_host.py builds and runs it; no HIP, no GPU).
//
// stdin, one case per line:
//   map T tiles_per_table R S
//       -> "grid N", then N lines "table tile part parts": drain_block_tile for blocks 0 .. N - 1, N = T * tiles_per_table plus the
//          appended blocks 8 * ((T / 8 * tiles_per_table) mod R) * (S - 1) (none with S <= 1)
//   resolve T tiles_per_table R want_split
//       -> "round_wgs drain_split extra_blocks": resolve_drain_split
//   plan T B N D dtype weighted bags_per_block xcd_affine stage_out drain_split round_wgs
//       -> the twelve reported members of plan_forward's LaunchPlan, then round_wgs drain_split
#include <cstdio>
#include <cstring>

#include "launch_plan.h"

int main() {
    char line[512];
    static const float some_weight = 1.0f;
    while (fgets(line, sizeof line, stdin)) {
        char what[16];
        long long v[11] = {};
        const int n = sscanf(line, "%15s %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", what, &v[0], &v[1], &v[2], &v[3], &v[4], &v[5],
                             &v[6], &v[7], &v[8], &v[9], &v[10]);
        if (n < 1) continue;
        if (!strcmp(what, "map") && n == 5) {
            const int T = static_cast<int>(v[0]), tpt = static_cast<int>(v[1]), R = static_cast<int>(v[2]), S = static_cast<int>(v[3]);
            const long long slots = static_cast<long long>(T / pm::kXcds) * tpt;
            const long long grid = static_cast<long long>(T) * tpt + (S > 1 ? pm::kXcds * (slots % R) * (S - 1) : 0);
            printf("grid %lld\n", grid);
            for (long long b = 0; b < grid; ++b) {
                const pm::BlockTile bt = pm::drain_block_tile(static_cast<int32_t>(b), T, tpt, R, S);
                printf("%d %d %d %d\n", bt.table, bt.tile, bt.part, bt.parts);
            }
        } else if (!strcmp(what, "resolve") && n == 5) {
            const pm::DrainSplit o =
                pm::resolve_drain_split(static_cast<int>(v[0]), static_cast<int>(v[1]), static_cast<int>(v[2]), static_cast<int>(v[3]));
            printf("%d %d %d\n", o.round_wgs, o.drain_split, o.extra_blocks);
        } else if (!strcmp(what, "plan") && n == 12) {
            pm_embbag_batch op;
            memset(&op, 0, sizeof op);
            op.num_tables = static_cast<int32_t>(v[0]);
            op.batch = v[1];
            op.num_indices = v[2];
            op.bag_begin = 0;
            op.bag_count = v[1];
            op.max_dim = static_cast<int32_t>(v[3]);
            op.weight_dtype = static_cast<int32_t>(v[4]);
            op.index_dtype = PM_I64;
            op.per_sample_weights = v[5] ? &some_weight : nullptr;
            op.out_stride = op.max_dim;
            pm::TuningSetters s;
            s.bags_per_block = static_cast<int>(v[6]);
            s.xcd_affine = static_cast<int>(v[7]);
            s.stage_out = static_cast<int>(v[8]);
            pm::FwdEnv e;
            e.drain_split = static_cast<int>(v[9]);
            e.round_wgs = static_cast<int>(v[10]);
            const pm::LaunchPlan p = pm::plan_forward(op, op.weight_dtype, pm::resolve_knobs(s, e));
            printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", p.tiles_per_table, p.bags_per_block, p.idx_cap, p.xcd_affine, p.nt_loads,
                   p.ordered, p.stage_out, p.stage_bags, p.flat_bags, p.flat_target, p.flat_compact, p.unroll, p.round_wgs, p.drain_split);
        } else {
            fprintf(stderr, "bad line: %s", line);
            return 2;
        }
    }
    return 0;
}
