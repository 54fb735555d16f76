"""The plan sweep on the CPU: what every case of tests/plan_sweep.py plans, pinned in tests/plan_sweep_host.json, and the conditions that
keep the case list from quietly shrinking.

launch_plan_dump.cpp is built as tests/test_launch_plan_host.py builds it and plans every case from its sizes and knobs; the JSON holds
one row per case -- the plan's members (twelve; the gather's eight) and the variant label ``plan_sweep.label`` derives from them.
tests/test_gpu_plan_sweep.py then requires ``pm_embbag_plan`` to report exactly these rows next to every launch it compares.

``PARAM_AMD_REWRITE_PLAN_SWEEP=1 pytest tests/test_plan_sweep_host.py`` writes the JSON anew from what launch_plan.h plans (read the
diff: a changed row is a changed kernel choice)."""
import json
import os
import shutil
import subprocess

import pytest

from tests import plan_sweep as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PINNED = os.path.join(HERE, "plan_sweep_host.json")
REWRITE = os.environ.get("PARAM_AMD_REWRITE_PLAN_SWEEP") == "1"


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """{case name: plan members} from launch_plan_dump"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("plan_sweep") / "launch_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "param_amd", "csrc"), os.path.join(HERE, "launch_plan_dump.cpp"), "-o", exe], check=True)
    text = "".join(c.dump_line() + "\n" for c in S.CASES)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(S.CASES)
    return {c.name: [int(x) for x in line.split()] for c, line in zip(S.CASES, out)}


def _rows(planned):
    rows = {}
    for c in S.CASES:                                              # (the scaled FP8 pooled plan: plan_f8's row after the restated LDS rule)
        plan = S.pinned_plan(c, planned[c.name])
        rows[c.name] = {"plan": plan, "label": " ".join(sorted(S.label(c, plan, planned[c.name])))}
    return rows


def _pinned():
    return json.load(open(PINNED))["rows"]


def test_every_case_plans_its_pinned_row(planned):
    rows = _rows(planned)
    if REWRITE:
        with open(PINNED, "w") as f:
            f.write('{\n "plan_fields": %s,\n "gather_fields": %s,\n "rows": {\n' % (json.dumps(list(S.PLAN_FIELDS)), json.dumps(list(S.GATHER_FIELDS))))
            f.write(",\n".join("  %s: %s" % (json.dumps(name), json.dumps(row)) for name, row in rows.items()))
            f.write("\n }\n}\n")
    pinned = _pinned()
    assert list(pinned) == [c.name for c in S.CASES], "the case list and the pinned rows name different cases"
    bad = [(name, pinned[name], row) for name, row in rows.items() if row != pinned[name]]
    assert not bad, f"{len(bad)} of {len(rows)} rows differ; the first (case, pinned, planned): {bad[0]}"


def test_the_pinned_rows_are_not_being_rewritten():
    assert not REWRITE, "PARAM_AMD_REWRITE_PLAN_SWEEP=1 rewrote tests/plan_sweep_host.json: read its diff, then run without the flag"


def test_the_plan_query_reports_the_pinned_rows_without_a_gpu():
    """``pm_embbag_plan`` / ``pm_embedding_gather_plan`` launch nothing and read no device memory: on a CPU-only machine, with dummy
    pointers, they report the pinned row of every case under its knobs -- the library's ``current_knobs`` and the dump tool's
    ``resolve_knobs`` agree.  The groups with an environment setting are asked in one child process each."""
    import sys

    from tests import plan_sweep_worker as W

    rows = _pinned()
    got = {}
    for group in S.GROUPS:
        if group not in S.ENV_GROUPS:
            got.update(W.host_plans(group))
            continue
        env = {k: v for k, v in os.environ.items() if k not in S.ENV}
        env.update({k: str(v) for k, v in next(c.env for c in S.CASES if c.group == group).items()})
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, "-m", "tests.plan_sweep_worker", "--plans", group], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got.update(json.loads(r.stdout.splitlines()[-1]))
    bad = [(name, rows[name]["plan"], plan) for name, plan in got.items() if plan != rows[name]["plan"]]
    assert len(got) == len(S.CASES) and not bad, f"{len(bad)} differ; the first (case, pinned, reported): {bad[0]}"


def test_the_plan_query_refuses_what_the_launching_call_refuses():
    import ctypes

    from param_amd import _lib

    L = _lib.load()
    out = (ctypes.c_int32 * 12)()
    op = _lib.pm_embbag_batch()
    assert L.pm_embbag_plan(ctypes.byref(op), _lib.PM_PLAN_FORWARD, out) == _lib.PM_ERR_INVALID and b"num_tables" in L.pm_last_error()
    assert L.pm_embbag_plan(None, _lib.PM_PLAN_FORWARD, out) == _lib.PM_ERR_INVALID
    op.num_tables, op.weight_dtype, op.index_dtype, op.max_dim = 1, _lib.PM_F32, _lib.PM_I64, 8
    op.tables = op.rows = op.dims = op.out_offsets = 8
    assert L.pm_embbag_plan(ctypes.byref(op), 5, out) == _lib.PM_ERR_INVALID and b"kind" in L.pm_last_error()
    assert L.pm_embbag_plan(ctypes.byref(op), _lib.PM_PLAN_BASE, None) == _lib.PM_ERR_INVALID
    assert L.pm_embedding_gather_plan(ctypes.byref(op), None) == _lib.PM_ERR_INVALID
    assert L.pm_embbag_plan(ctypes.byref(op), _lib.PM_PLAN_FORWARD, out) == _lib.PM_OK                # an empty request has a plan
    op.max_dim = 6
    assert L.pm_embbag_plan(ctypes.byref(op), _lib.PM_PLAN_FORWARD, out) == _lib.PM_ERR_UNSUPPORTED and b"multiple of 4" in L.pm_last_error()


def test_the_plans_the_issue_checked():
    """the plans quoted where the sweep was asked for, member for member"""
    rows = _pinned()
    p = lambda name: " ".join(map(str, rows[name]["plan"]))                                  # noqa: E731
    assert p("tile_staged_u2_plain") == "3 32 1280 3 0 0 128 32 0 0 0 2"
    assert p("tile_ordered_u2_plain").startswith("4 32 4096 0 0 1 0 32 ")
    assert p("tile_rank128_weighted").startswith("3 128 4096 0 0 1 0 128 ")
    assert p("env_tile_major_ordered").startswith("4 32 4096 2 0 1 ")
    assert p("auto_bench_fp32") == "43 32 1280 1 0 0 128 32 0 0 0 2"
    assert p("auto_t26") == "80 32 1280 3 0 0 128 32 0 0 0 2"
    assert p("auto_ragged_long") == "129 32 4096 1 0 1 0 32 0 0 0 2"


def test_auto_cases_plan_what_the_benchmark_shapes_plan():
    """no knob set: the three product-scale cases take the kernel variant of rows bench_fp32, t26 and ragged_long of
    tests/launch_plan_host.json -- every member but tiles_per_table, which counts the bags"""
    spec = json.load(open(os.path.join(HERE, "launch_plan_host.json")))
    rows = _pinned()
    for case, fixture in (("auto_bench_fp32", "bench_fp32"), ("auto_t26", "t26"), ("auto_ragged_long", "ragged_long")):
        c = next(c for c in S.CASES if c.name == case)
        assert not c.tuning and not c.forward and not c.env and c.entry == "fwd" and 1_200_000 < c.req.N < 1_400_000
        want = [r[3] for r in spec["rows"] if r[:3] == [fixture, "default", "forward"]]
        assert len(want) == 1 and rows[case]["plan"][1:] == want[0][1:], (case, rows[case]["plan"], want)
        assert rows[case]["plan"][0] == -(-c.req.B // want[0][1])


def _f8_conditions(cases, missing):
    """the FP8 entries (``f8``: pm_embbag_fwd_f8, ``f8_gather``: pm_embedding_gather_f8).  Every condition reads the label
    ``plan_sweep.f8_label`` derives from the request's offsets, indices and pads next to the pinned plan.  At the end: every FP8 case is
    the last one left to meet some condition, so deleting any of them is noticed."""
    f8 = [(c, w, p) for c, w, p in cases if c.entry in ("f8", "f8_gather")]
    assert all("f8" in w for c, w, p in cases if c.entry.startswith("f8")) and not any("f8" in w for c, w, p in cases if not c.entry.startswith("f8"))
    assert not any({"row", "table"} & w for c, w, p in f8)          # (the scaled entries' words: _f8s_conditions)
    held = []                                                      # (the cases that meet a condition, how many it asks for)

    def need(what, cond, at_least=1):
        got = [c.name for c, w, p in f8 if cond(c, w, p)]
        held.append((got, at_least))
        if len(got) < at_least:
            missing.append("f8: " + what)

    pooled = lambda c, w: "pooled" in w and not c.env                                           # noqa: E731
    tiles = lambda p: p["tiles_per_table"]                                                      # noqa: E731
    modes = ("unweighted", "weighted", "mean")
    # the multi-tile baseline: at least three tiles a table, a partial last one, two bags per lane group
    base = lambda c, w, p: pooled(c, w) and {"G16", "bpb32", "u2", "tile>NG", "partial", "xcd0"} <= w and tiles(p) >= 3 and c.dims[0] == 256  # noqa: E731
    for fmt in S.F8_DTYPE:
        for mode in modes:
            need(f"baseline {fmt} {mode}, fp32 rows leave one by one", lambda c, w, p: base(c, w, p) and {fmt, mode, "out-fp32", "plain"} <= w)
            need(f"baseline {fmt} {mode}, bf16 burst", lambda c, w, p: base(c, w, p) and {fmt, mode, "out-bf16", "staged"} <= w)
    for mode in modes:
        need(f"baseline {mode}, bf16 with stage_out 0", lambda c, w, p: base(c, w, p) and {mode, "out-bf16", "plain"} <= w)
    need("baseline fp16 burst", lambda c, w, p: base(c, w, p) and {"out-fp16", "staged"} <= w)
    # ... and with fp32 rows through the burst (two bags per lane group: G = 8 and D <= 64 only)
    for mode in modes:
        for burst in ("staged", "plain"):
            need(f"64-bag tiles of fp32 rows {mode} {burst}",
                 lambda c, w, p: pooled(c, w) and {"G8", "bpb64", "u2", "tile>NG", "partial", "out-fp32", mode, burst} <= w and tiles(p) >= 3)
    # every lane-group width x every depth, two bags per lane group, more than one tile a table
    for G, D, _ in S.F8_GROUP_DIMS:
        group = lambda c, w, p: pooled(c, w) and {f"G{G}", f"bpb{512 // G}", "tile>NG", "partial"} <= w and tiles(p) > 1 and c.dims[0] == D \
            and c.request == "pad100"                                                          # noqa: E731
        for u in (2, 4, 8):
            for mode in modes[:2]:
                need(f"G{G} u{u} {mode}", lambda c, w, p: group(c, w, p) and {f"u{u}", mode} <= w)
        need(f"G{G} mean", lambda c, w, p: group(c, w, p) and "mean" in w)
    # compaction: each of the three reached weighted, unweighted and under mean
    for word in ("rounds>1", "waves>1", "carry"):
        for mode in modes:
            need(f"{word} {mode}", lambda c, w, p: pooled(c, w) and {word, mode} <= w)
    # block orders, a slice, each over more than one tile a table
    for x in (0, 1, 3):
        need(f"xcd_affine {x}, the product's tile", lambda c, w, p: pooled(c, w) and {f"xcd{x}", "G8", "bpb32", "staged", "partial", "unweighted"} <= w
             and tiles(p) > 1 and not {"slice", "direct"} & w and c.dims == [128] * c.req.T)
    need("xcd_affine 1 on 8 tables", lambda c, w, p: pooled(c, w) and "xcd1" in w and c.req.T == 8 and tiles(p) > 1)
    for mode in ("unweighted", "mean"):
        need(f"slice inside tiles {mode}", lambda c, w, p: pooled(c, w) and {"slice", "partial", mode} <= w and tiles(p) > 1
             and c.bag_slice[0] % p["bags_per_block"] and sum(c.bag_slice) % p["bags_per_block"])
    # 1024-bag tiles whose indices are compacted in LDS: the fifth bound, ten rounds
    for mode in modes:
        for out in ("out-fp32", "out-bf16"):
            need(f"1024 bags {mode} {out}", lambda c, w, p: pooled(c, w) and {"bounds5", "bpb1024", "rounds>1", "waves>1", "carry", mode, out} <= w
                 and c.req.B > 1024)
    # a direct tile with padding among compacted tiles
    for mode in modes:
        for u in (2, 8):
            need(f"direct {mode} u{u}", lambda c, w, p: pooled(c, w) and {"direct", "rounds>1", "bpb32", mode, f"u{u}"} <= w and p["idx_cap"] == 1280
                 and c.req.pads is not None and tiles(p) > 1)
    need("mixed dims, the lane group sized for 128", lambda c, w, p: pooled(c, w) and "G8" in w and c.dims == [16, 64, 128] and tiles(p) > 1)
    wide = lambda c, w, p: pooled(c, w) and {"G32", "bpb16", "tile>NG"} <= w and c.dims[0] == 512 and tiles(p) > 1       # noqa: E731
    need("D = 512, 2-byte outputs: staged", lambda c, w, p: wide(c, w, p) and {"out-bf16", "staged"} <= w)
    need("D = 512, 4-byte outputs: not staged", lambda c, w, p: wide(c, w, p) and {"out-fp32", "plain"} <= w and not c.forward)
    need("two column passes over more than one tile", lambda c, w, p: pooled(c, w) and {"G64", "passes2", "tile>NG"} <= w and tiles(p) > 1)
    need("FWD_STAGE=0", lambda c, w, p: c.env.get("PARAM_AMD_FWD_STAGE") == 0 and {"pooled", "plain", "bpb32"} <= w and tiles(p) > 1
         and p["bags_per_block"] * c.dims[0] * 4 <= 16384)
    # the gather: 16 (G, U) pairs over tens of tiles with a last one that is not full, both orders
    gp = lambda p: dict(zip(S.GATHER_FIELDS, p.values()))                                       # noqa: E731
    rows = lambda c, w, p: "unpooled" in w and "partial" in w and gp(p)["grid"] > 8                    # noqa: E731
    for G in (8, 16, 32, 64):
        for u in (1, 2, 4, 8):
            need(f"gather G{G} u{u}", lambda c, w, p: rows(c, w, p) and {f"G{G}", f"u{u}", "out-fp32", "e4m3", "xcd1", "passes1"} <= w and "slice" not in w)
    for u in (1, 2, 4, 8):
        for out in ("out-bf16", "out-fp16"):
            need(f"gather u{u} {out}", lambda c, w, p: rows(c, w, p) and {f"u{u}", out} <= w)
    need("gather xcd0", lambda c, w, p: rows(c, w, p) and "xcd0" in w)
    need("gather two passes", lambda c, w, p: {"unpooled", "passes2", "G64"} <= w and c.dims[0] == 512)
    need("gather slice", lambda c, w, p: rows(c, w, p) and "slice" in w and c.bag_slice[0] > 0)
    need("gather e5m2 next to e4m3 at one (G, U)", lambda c, w, p: rows(c, w, p) and "e5m2" in w
         and any("e4m3" in w2 and w2 - {"e4m3"} == w - {"e5m2"} for _, w2, _ in f8))
    spare = [c.name for c, w, p in f8 if not any(c.name in got and len(got) == n for got, n in held)]
    assert not spare, f"FP8 cases that no condition depends on: {spare}"


def _needs(family, missing, prefix):
    """(need, spare): ``need(what, cond, at_least=1)`` notes ``what`` as missing unless ``at_least`` cases of ``family`` meet ``cond``;
    ``spare()`` names the cases that are never the last ones left to meet a condition -- deleting one of those would go unnoticed"""
    held = []

    def need(what, cond, at_least=1):
        got = [c.name for c, w, p in family if cond(c, w, p)]
        held.append((got, at_least))
        if len(got) < at_least:
            missing.append(f"{prefix}: {what}")

    return need, lambda: [c.name for c, w, p in family if not any(c.name in got and len(got) == n for got, n in held)]


def _f8s_conditions(cases, missing):
    """the scaled FP8 entries (``f8s``: pm_embbag_fwd_f8_scaled, ``f8s_gather``: pm_embedding_gather_f8_scaled): the FP8 entries'
    conditions on ``f8_label``'s words plus the kind of exponent, and the LDS edge where the row exponents' bytes cost a tile its burst.
    At the end: every scaled case is the last one left to meet some condition."""
    fam = [(c, w, p) for c, w, p in cases if c.entry.startswith("f8s")]
    assert all(len({"row", "table"} & w) == 1 for c, w, p in fam)
    need, spare = _needs(fam, missing, "f8s")
    pooled = lambda c, w: "pooled" in w and not c.env                                           # noqa: E731
    tiles = lambda p: p["tiles_per_table"]                                                      # noqa: E731
    modes = ("unweighted", "weighted", "mean")
    base = lambda c, w, p: pooled(c, w) and {"G16", "bpb32", "u2", "tile>NG", "partial", "xcd0"} <= w and tiles(p) >= 3 and c.dims[0] == 256  # noqa: E731
    for fmt in S.F8_DTYPE:
        for sc in ("row", "table"):
            for mode in modes:
                need(f"baseline {fmt} {sc} {mode}, fp32 rows leave one by one", lambda c, w, p: base(c, w, p) and {fmt, sc, mode, "out-fp32", "plain"} <= w)
                need(f"baseline {fmt} {sc} {mode}, bf16 burst", lambda c, w, p: base(c, w, p) and {fmt, sc, mode, "out-bf16", "staged"} <= w)
    need("baseline bf16 with stage_out 0", lambda c, w, p: base(c, w, p) and {"row", "out-bf16", "plain"} <= w and c.forward.get("stage_out") == 0)
    for sc, ms in (("row", modes), ("table", modes[:1])):
        for mode in ms:
            for burst in ("staged", "plain"):
                need(f"64-bag tiles of fp32 rows {sc} {mode} {burst}",
                     lambda c, w, p: pooled(c, w) and {"G8", "bpb64", "u2", "tile>NG", "partial", "out-fp32", sc, mode, burst} <= w and tiles(p) >= 3)
    for G, D, _ in S.F8_GROUP_DIMS:
        group = lambda c, w, p: pooled(c, w) and {f"G{G}", f"bpb{512 // G}", "tile>NG", "partial"} <= w and tiles(p) > 1 and c.dims[0] == D \
            and c.request == "pad100"                                                          # noqa: E731
        for u in (2, 4, 8):
            for mode in modes[:2]:
                need(f"G{G} u{u} {mode} row", lambda c, w, p: group(c, w, p) and {f"u{u}", mode, "row"} <= w)
        need(f"G{G} mean row", lambda c, w, p: group(c, w, p) and {"mean", "row"} <= w)
        need(f"G{G} table", lambda c, w, p: group(c, w, p) and "table" in w)
    for x in (0, 1, 3):
        need(f"xcd_affine {x}, row exponents", lambda c, w, p: pooled(c, w) and {f"xcd{x}", "G8", "bpb32", "staged", "partial", "unweighted", "row"} <= w
             and tiles(p) > 1 and not {"slice", "direct"} & w and c.dims == [128] * c.req.T)
    need("xcd_affine 1 on 8 tables", lambda c, w, p: pooled(c, w) and {"xcd1", "row"} <= w and c.req.T == 8 and tiles(p) > 1)
    for mode in ("unweighted", "mean"):
        need(f"slice inside tiles {mode}", lambda c, w, p: pooled(c, w) and {"slice", "partial", mode, "row"} <= w and tiles(p) > 1
             and c.bag_slice[0] % p["bags_per_block"] and sum(c.bag_slice) % p["bags_per_block"])
    for mode in modes:
        for out in ("out-fp32", "out-bf16"):
            need(f"1024 bags {mode} {out}", lambda c, w, p: pooled(c, w) and {"bounds5", "bpb1024", "rounds>1", "waves>1", "carry", mode, out, "row"} <= w
                 and c.req.B > 1024)
    for mode in modes:
        for u in (2, 8):
            need(f"direct {mode} u{u}", lambda c, w, p: pooled(c, w) and {"direct", "rounds>1", "bpb32", mode, f"u{u}", "row"} <= w
                 and p["idx_cap"] == 1280 and c.req.pads is not None and tiles(p) > 1)
    # the LDS edge (common.h: f8s_stage_out), byte for byte from the restated rule: (with the burst plan_f8 granted, as launched)
    # (the reach test sees the pinned rows only: the stage_out plan_f8 granted is put back from the label word here, so these conditions
    # hold the label, the pinned stage_out and the byte counts to one another; that the pinned row IS the dump's row after the rule is
    # test_every_case_plans_its_pinned_row's, which recomputes row and label from launch_plan_dump)
    def lds(c, w, p):
        dumped = dict(p, stage_out=max(c.dims) if "burst-dropped" in w else p["stage_out"])
        return S.f8s_case_lds(c, [dumped[f] for f in S.PLAN_FIELDS])
    edge = lambda c, w, p: pooled(c, w) and {"bpb512", "out-bf16", "G8"} <= w and p["idx_cap"] == 4096 and c.dims[0] == 16          # noqa: E731
    need("edge: row exponents and weights drop the burst", lambda c, w, p: edge(c, w, p) and {"row", "weighted", "burst-dropped", "plain"} <= w
         and p["stage_out"] == 0 and lds(c, w, p) == (65552, 49168))
    need("edge: a table exponent keeps it", lambda c, w, p: edge(c, w, p) and {"table", "weighted", "staged"} <= w and lds(c, w, p) == (61456, 61456))
    need("edge: row exponents without weights keep it", lambda c, w, p: edge(c, w, p) and {"row", "unweighted", "staged"} <= w and lds(c, w, p) == (49168, 49168))
    for c, w, p in fam:                                            # ... and nothing else plans past it
        if c.entry == "f8s":
            assert ("burst-dropped" in w) == (lds(c, w, p)[0] > 65536) and lds(c, w, p)[1] <= 65536, c.name
    need("mixed dims, the lane group sized for 128", lambda c, w, p: pooled(c, w) and {"G8", "row"} <= w and c.dims == [16, 64, 128] and tiles(p) > 1)
    wide = lambda c, w, p: pooled(c, w) and {"G32", "bpb16", "tile>NG", "row"} <= w and c.dims[0] == 512 and tiles(p) > 1       # noqa: E731
    need("D = 512, 2-byte outputs: staged", lambda c, w, p: wide(c, w, p) and {"out-bf16", "staged"} <= w)
    need("D = 512, 4-byte outputs: not staged", lambda c, w, p: wide(c, w, p) and {"out-fp32", "plain"} <= w and not c.forward)
    need("two column passes over more than one tile", lambda c, w, p: pooled(c, w) and {"G64", "passes2", "tile>NG", "row"} <= w and tiles(p) > 1)
    need("FWD_STAGE=0", lambda c, w, p: c.env.get("PARAM_AMD_FWD_STAGE") == 0 and {"pooled", "plain", "bpb32", "row"} <= w and tiles(p) > 1
         and p["bags_per_block"] * c.dims[0] * 4 <= 16384)
    gp = lambda p: dict(zip(S.GATHER_FIELDS, p.values()))                                       # noqa: E731
    rows = lambda c, w, p: "unpooled" in w and "partial" in w and gp(p)["grid"] > 8 and c.req.T > 1    # noqa: E731
    for G in (8, 16, 32, 64):
        for u in (1, 2, 4, 8):
            need(f"gather G{G} u{u} row", lambda c, w, p: rows(c, w, p) and {f"G{G}", f"u{u}", "out-fp32", "e4m3", "xcd1", "passes1", "row"} <= w
                 and "slice" not in w)
        need(f"gather G{G} table", lambda c, w, p: rows(c, w, p) and {f"G{G}", "table"} <= w)
    for out in ("out-bf16", "out-fp16"):
        need(f"gather {out}", lambda c, w, p: rows(c, w, p) and {out, "row"} <= w)
    need("gather xcd0", lambda c, w, p: rows(c, w, p) and "xcd0" in w)
    need("gather two passes", lambda c, w, p: {"unpooled", "passes2", "G64", "row"} <= w and c.dims[0] == 512)
    need("gather slice", lambda c, w, p: rows(c, w, p) and "slice" in w and c.bag_slice[0] > 0)
    need("gather e5m2", lambda c, w, p: rows(c, w, p) and {"e5m2", "row"} <= w)
    assert not spare(), f"scaled FP8 cases that no condition depends on: {spare()}"


def _anyfmt_conditions(cases, missing):
    """the mixed-format entries (``anyfmt``: pm_embbag_fwd_anyfmt, ``anyfmt_gather``: pm_embedding_gather_anyfmt) on the words of
    ``plan_sweep.anyfmt_label``.  At the end: every mixed-format case is the last one left to meet some condition."""
    fam = [(c, w, p) for c, w, p in cases if c.entry.startswith("anyfmt")]
    assert all("any" in w for c, w, p in fam) and not any("any" in w for c, w, p in cases if not c.entry.startswith("anyfmt"))
    need, spare = _needs(fam, missing, "anyfmt")
    seven = list(S.ANY_UNROLL)
    pooled = lambda c, w: "pooled" in w and not c.env                                           # noqa: E731
    tiles = lambda p: p["tiles_per_table"]                                                      # noqa: E731
    wt = ("unweighted", "weighted")
    differ = lambda c: all(a != b for a, b in zip(c.formats, c.formats[1:]))                    # noqa: E731
    all7 = lambda w: {f"fmt:{f}" for f in seven} <= w                                           # noqa: E731
    assert all(differ(c) for c, w, p in fam), "tables next to each other differ in format: so do consecutive tiles of different tables"
    # every (format, lane-group width, weighted) in a multi-tile case with two bags per lane group
    for G in (8, 16, 32, 64):
        for f in seven:
            for mode in wt:
                need(f"{f} G{G} {mode}", lambda c, w, p: pooled(c, w) and {f"fmt:{f}", f"G{G}", f"bpb{512 // G}", "tile>NG", "partial", "staged", mode,
                                                                          "out-fp32", "passes1"} <= w
                     and tiles(p) > 1 and c.request == "pad100" and c.dims == [G * 8] * 3 and not c.bag_slice)
    for f in seven:
        need(f"{f}: a bag that ends in the tail loop of its {S.ANY_UNROLL[f]} rows in flight", lambda c, w, p: pooled(c, w) and f"tail:{f}" in w)
    # four bags per lane group: the 16-bit burst fits, the 4-byte one does not; all seven formats
    four = lambda c, w, p: pooled(c, w) and {"G32", "bpb32", "tile>NG", "partial"} <= w and all7(w) and tiles(p) > 1       # noqa: E731
    need("bf16 burst", lambda c, w, p: four(c, w, p) and {"out-bf16", "staged"} <= w)
    need("fp16 burst", lambda c, w, p: four(c, w, p) and {"out-fp16", "staged"} <= w)
    need("fp32 rows of the same tile leave one by one", lambda c, w, p: four(c, w, p) and {"out-fp32", "plain"} <= w and not c.forward)
    for mode in wt:
        for burst in ("staged", "plain"):
            need(f"64-bag tiles of fp32 rows {mode} {burst}",
                 lambda c, w, p: pooled(c, w) and {"G8", "bpb64", "tile>NG", "partial", "out-fp32", mode, burst} <= w and tiles(p) >= 3 and c.req.B > 1024)
    need("xcd_affine 0, all seven formats", lambda c, w, p: pooled(c, w) and {"xcd0", "G16", "bpb32"} <= w and all7(w) and tiles(p) > 1)
    need("xcd_affine 1, all seven formats", lambda c, w, p: pooled(c, w) and {"xcd1", "G16", "bpb32"} <= w and all7(w) and tiles(p) > 1 and c.req.T == 8)
    need("xcd_affine 3", lambda c, w, p: pooled(c, w) and {"xcd3", "G16", "bpb32", "partial"} <= w and tiles(p) > 1)
    for mode in wt:
        need(f"slice inside tiles {mode}", lambda c, w, p: pooled(c, w) and {"slice", "partial", mode} <= w and tiles(p) > 1
             and c.bag_slice[0] % p["bags_per_block"] and sum(c.bag_slice) % p["bags_per_block"])
        need(f"1024 bags {mode}", lambda c, w, p: pooled(c, w) and {"bpb1024", "tile>NG", "partial", mode} <= w and c.req.B > 1024)
        for f in ("fp8_e4m3", "int4", "fp32"):
            need(f"direct tile of a {f} table {mode}", lambda c, w, p: pooled(c, w) and {f"direct:{f}", "G32", "bpb32", "tile>NG", mode} <= w
                 and p["idx_cap"] == 1280 and tiles(p) > 1)
        need(f"D = 520 {mode}", lambda c, w, p: pooled(c, w) and {"G64", "passes2", "row-ends-in-pass", "tile>NG", mode} <= w and tiles(p) > 1)
        need(f"four passes {mode}", lambda c, w, p: pooled(c, w) and {"G64", "passes4", "tile>NG", mode} <= w and c.dims[0] == 2048 and tiles(p) > 1)
    need("mixed dims, the lane group sized for 128", lambda c, w, p: pooled(c, w) and "G16" in w and c.dims == [16, 64, 128] and tiles(p) > 1)
    need("FWD_STAGE=0", lambda c, w, p: c.env.get("PARAM_AMD_FWD_STAGE") == 0 and {"any", "pooled", "plain", "bpb32"} <= w and tiles(p) > 1
         and p["bags_per_block"] * c.dims[0] * 4 <= 16384)
    # the launcher's 64 KiB fallback (embbag_fwd_anyfmt_kernel.inc: launch_any_w) is out of reach: the largest tile any plan can ask for
    # -- 1024 bags, 4096 index-tile entries, weights -- is 40976 bytes, the burst at most 16384
    any_lds = lambda bpb, cap, weighted, burst: ((bpb + 2) // 2 * 2 * 8 + cap * 4 * (2 if weighted else 1) + 15) // 16 * 16 + burst  # noqa: E731
    assert any_lds(1024, 4096, True, 16384) == 40976 + 16384 <= 65536
    for c, w, p in fam:
        if c.entry == "anyfmt":
            burst = p["bags_per_block"] * p["stage_out"] * (2 if c.out16 else 4)
            assert burst <= 16384 and p["idx_cap"] <= 4096 and any_lds(p["bags_per_block"], p["idx_cap"], c.weighted, burst) <= 57360, c.name
    # the gather: a tile of positions holds all seven formats, a wave several
    gp = lambda p: dict(zip(S.GATHER_FIELDS, p.values()))                                       # noqa: E731
    rows = lambda c, w, p: {"unpooled", "partial", "u4"} <= w and gp(p)["grid"] > 1                    # noqa: E731
    for G in (8, 16, 32, 64):
        for out in ("out-fp32", "out-bf16", "out-fp16"):
            need(f"gather G{G} {out}", lambda c, w, p: rows(c, w, p) and {f"G{G}", out, "tile-formats7", "lds_borders", "xcd1", "passes1"} <= w
                 and not {"wave-formats1", "slice"} & w and c.dims[0] == G * 8)
    need("gather xcd0", lambda c, w, p: rows(c, w, p) and {"xcd0", "tile-formats7"} <= w)
    need("gather slice", lambda c, w, p: rows(c, w, p) and "slice" in w and c.bag_slice[0] > 0)
    need("gather D = 520", lambda c, w, p: rows(c, w, p) and {"G64", "passes2", "row-ends-in-pass"} <= w)
    need("gather four passes", lambda c, w, p: rows(c, w, p) and {"G64", "passes4"} <= w and c.dims[0] == 2048)
    need("gather beyond 255 tables", lambda c, w, p: rows(c, w, p) and {"global_borders", "tile-formats7"} <= w and c.req.T > 255)
    assert not spare(), f"mixed-format cases that no condition depends on: {spare()}"


def test_the_sweep_reaches_every_variant():
    """conditions on the case list -- on the labels derived from the PLANS -- so that it cannot quietly stop covering a variant"""
    rows = _pinned()
    cases = [(c, set(rows[c.name]["label"].split()), dict(zip(S.PLAN_FIELDS, rows[c.name]["plan"]))) for c in S.CASES]
    missing = []
    from tests import plan_sweep_worker as W

    def need(what, cond, at_least=1):
        if sum(1 for c, w, p in cases if cond(c, w, p)) < at_least:
            missing.append(what)

    fwd = lambda c: c.entry == "fwd" and not c.env                                            # noqa: E731
    wt = {False: "unweighted", True: "weighted"}
    # tile kernel: unroll x weighted x {ordered, staged, plain}, fp32, G = 32, more than one bag per lane group
    for u in S.UNROLLS:
        for wgt in (False, True):
            for variant in ("ordered-bitonic", "staged", "plain"):
                need(f"tile {variant} u{u} {wt[wgt]}",
                     lambda c, w, p: fwd(c) and {"tile", "f32", "G32", f"u{u}", wt[wgt], variant, "tile>NG"} <= w)
    for kind in S.DTYPE:
        for G in (8, 16, 32, 64):
            for variant in ("ordered-bitonic", "staged"):
                need(f"tile {variant} {kind} G{G}", lambda c, w, p: fwd(c) and {"tile", kind, f"G{G}", "u2", variant, "tile>NG"} <= w)
    need("bitonic, partial last tile, direct-index tile", lambda c, w, p: {"tile", "ordered-bitonic", "partial", "direct"} <= w)
    need("rank at 128 bags, weighted, direct", lambda c, w, p: {"tile", "ordered-rank", "bpb128", "weighted", "direct"} <= w)
    need("rank at 1024 bags, direct", lambda c, w, p: {"tile", "ordered-rank", "bpb1024", "direct"} <= w)
    need("staged, power-of-two row", lambda c, w, p: {"tile", "staged", "burst-pow2", "partial"} <= w)
    need("staged 32-bag tile that overflows its index tile", lambda c, w, p: {"tile", "staged", "bpb32", "direct"} <= w and p["idx_cap"] == 1280, 2)
    need("staged, D = 56", lambda c, w, p: {"tile", "staged", "burst-div"} <= w and c.dims[0] == 56)
    for x in (0, 1, 3):
        need(f"tile staged xcd_affine {x}", lambda c, w, p: fwd(c) and {"tile", "staged", f"xcd{x}"} <= w)
    need("xcd_affine 1 on 8 tables", lambda c, w, p: {"tile", "xcd1"} <= w and c.req.T == 8)
    need("xcd_affine 3, tile count not divisible by 8", lambda c, w, p: {"tile", "xcd3"} <= w and c.req.T * p["tiles_per_table"] % 8 != 0)
    need("tile nt_loads staged", lambda c, w, p: {"tile", "staged", "nt1"} <= w)
    need("tile nt_loads ordered", lambda c, w, p: {"tile", "ordered-bitonic", "nt1"} <= w)
    need("tile slice staged", lambda c, w, p: {"tile", "staged", "slice", "partial"} <= w and c.bag_slice[0] > 0)
    need("tile slice ordered", lambda c, w, p: {"tile", "ordered-bitonic", "slice", "partial"} <= w and c.bag_slice[0] > 0)
    # flat kernel
    for u in S.UNROLLS:
        for wgt in (False, True):
            for rq in ("short1", "short2", "ragged", "mixed_even", "mixed_ragged"):
                need(f"flat {rq} u{u} {wt[wgt]}", lambda c, w, p: fwd(c) and c.request == rq and {"flat", f"u{u}", wt[wgt], "compact"} <= w)
    need("flat, ragged route, direct-index tile", lambda c, w, p: {"flat", "direct"} <= w and c.request == "ragged")
    need("flat_grid 0", lambda c, w, p: fwd(c) and {"flat", "old-grid"} <= w, 3)
    need("flat_grid 1", lambda c, w, p: fwd(c) and "flat" in w and c.forward.get("flat_grid") == 1 and p["flat_compact"] >= 1024, 3)
    need("3 workgroups, 16 lookups a tile", lambda c, w, p: {"flat", "grid3", "target16"} <= w, 3)
    need("flat slice", lambda c, w, p: {"flat", "slice"} <= w and c.bag_slice[0] > 0)
    for kind in ("bf16", "f16"):
        need(f"flat {kind}", lambda c, w, p: {"flat", kind} <= w, 2)
    # padded family
    fams = {"padded": lambda c: c.entry == "padded", "mean": lambda c: c.entry == "mean",
            "out16 bf16": lambda c: c.entry == "out16" and c.out16 == "bf16" and not c.mean,
            "out16 fp16": lambda c: c.entry == "out16" and c.out16 == "fp16", "out16 mean": lambda c: c.entry == "out16" and c.mean}
    for fam, is_fam in fams.items():
        pad = lambda c: is_fam(c) and not c.env and c.req.pads is not None                     # noqa: E731
        need(f"{fam}: 32 bags staged", lambda c, w, p: pad(c) and {"pad", "bpb32", "staged", "partial"} <= w)
        need(f"{fam}: 32 bags, stage_out 0", lambda c, w, p: pad(c) and {"pad", "bpb32", "plain"} <= w)
        need(f"{fam}: 1024 bags unweighted, staged", lambda c, w, p: pad(c) and {"pad", "bpb1024", "staged", "unweighted"} <= w
             and S.pad_lds_bytes(c, rows[c.name]["plan"]) <= 65536 and c.req.B > 1024)
        if fam != "mean" and fam != "out16 mean":                  # (mean pooling is unweighted)
            need(f"{fam}: 1024 bags weighted, the launcher's 64 KB fallback",
                 lambda c, w, p: pad(c) and {"pad", "bpb1024", "staged", "weighted"} <= w and S.pad_lds_bytes(c, rows[c.name]["plan"]) > 65536)
            need(f"{fam}: weighted", lambda c, w, p: pad(c) and {"pad", "bpb32", "weighted", "staged"} <= w)
        for x in (0, 1, 3):
            need(f"{fam}: xcd_affine {x}", lambda c, w, p: pad(c) and {"pad", f"xcd{x}"} <= w)
        need(f"{fam}: nt_loads", lambda c, w, p: pad(c) and {"pad", "nt1"} <= w)
        need(f"{fam}: slice", lambda c, w, p: pad(c) and {"pad", "slice", "partial"} <= w and c.bag_slice[0] > 0)
        for G in (8, 16, 32, 64):
            need(f"{fam}: G{G}", lambda c, w, p: pad(c) and {"pad", f"G{G}", "tile>NG"} <= w)
    need("D = 512 bf16 tables, 4-byte outputs: not staged", lambda c, w, p: c.entry == "padded" and {"pad", "bf16", "plain"} <= w and c.dims[0] == 512)
    need("D = 512 bf16 tables, 2-byte outputs: staged", lambda c, w, p: c.entry == "out16" and {"pad", "bf16", "staged"} <= w and c.dims[0] == 512)
    # max pooling: pm_embbag_fwd_max on the padded family's plan, for fp32 and for bf16 output
    for fam, o16 in (("max", None), ("max bf16", "bf16")):
        mx = lambda c, w: c.entry == "max" and c.out16 == o16 and not c.env and c.req.pads is not None and "max" in w  # noqa: E731
        need(f"{fam}: 32 bags staged", lambda c, w, p: mx(c, w) and {"pad", "bpb32", "staged", "partial"} <= w)
        need(f"{fam}: 32 bags, stage_out 0", lambda c, w, p: mx(c, w) and {"pad", "bpb32", "plain"} <= w and c.forward.get("stage_out") == 0)
        need(f"{fam}: 1024 bags staged", lambda c, w, p: mx(c, w) and {"pad", "bpb1024", "staged", "tile>NG"} <= w and c.req.B > 1024)
        for x in (0, 1, 3):
            need(f"{fam}: xcd_affine {x}", lambda c, w, p: mx(c, w) and {"pad", f"xcd{x}"} <= w)
        need(f"{fam}: nt_loads", lambda c, w, p: mx(c, w) and {"pad", "nt1"} <= w)
        need(f"{fam}: slice", lambda c, w, p: mx(c, w) and {"pad", "slice", "partial"} <= w and c.bag_slice[0] > 0)
        for G in (8, 16, 32, 64):
            need(f"{fam}: G{G}", lambda c, w, p: mx(c, w) and {"pad", f"G{G}", "tile>NG"} <= w)
        need(f"{fam}: G16 on fp32 tables", lambda c, w, p: mx(c, w) and {"pad", "f32", "G16", "tile>NG"} <= w)
        for kind16 in ("bf16", "f16"):             # (a 16-bit table's 16-bit output is its own type: fp16 tables give fp16)
            for G in (32, 64):
                need(f"{fam}: {kind16} tables G{G}", lambda c, w, p: c.entry == "max" and (c.out16 is None) == (o16 is None) and not c.env
                     and {"pad", "max", kind16, f"G{G}", "tile>NG"} <= w and c.dims[0] == G * 8)
        need(f"{fam}: fp32 rows of 512, two column passes", lambda c, w, p: mx(c, w) and {"pad", "f32", "G64", "tile>NG"} <= w and c.dims[0] == 512)
        need(f"{fam}: direct on a 32-bag tile", lambda c, w, p: mx(c, w) and {"pad", "bpb32", "direct", "tile>NG"} <= w and p["idx_cap"] == 1280)
        need(f"{fam}: mixed dims", lambda c, w, p: mx(c, w) and "pad" in w and c.dims == [16, 64, 128] and {lay for _, lay in W.variants(c)} == {"bd"})
    need("max: fp16 output", lambda c, w, p: c.entry == "max" and c.out16 == "fp16" and c.kind == "f32" and {"pad", "max", "bpb32", "staged"} <= w)
    need("max: D = 512 16-bit tables, 4-byte outputs: not staged",
         lambda c, w, p: c.entry == "max" and c.out16 is None and {"pad", "max", "plain"} <= w and c.dims[0] == 512 and c.kind != "f32", 2)
    need("max: D = 512 16-bit tables, 2-byte outputs: staged",
         lambda c, w, p: c.entry == "max" and c.out16 is not None and {"pad", "max", "staged"} <= w and c.dims[0] == 512 and c.kind != "f32", 2)
    need("max: FWD_STAGE=0", lambda c, w, p: c.entry == "max" and c.env.get("PARAM_AMD_FWD_STAGE") == 0 and {"pad", "max", "bpb32", "plain"} <= w)
    # the launcher's 64 KB fallback (embbag_fwd_max.hip: launch_max_a) is out of reach without weights: no max case plans past it
    for c, w, p in cases:
        if c.entry == "max":
            assert "max" in w and S.pad_lds_bytes(c, rows[c.name]["plan"]) <= 65536, c.name
            assert c.plan_kind == ("padded4" if c.out16 is None else "padded2") and not c.weighted and not c.mean, c.name
        else:
            assert "max" not in w, c.name
    # quantized, gather, base
    for u in (1, 3, 6):
        need(f"quantized u{u}", lambda c, w, p: c.entry == "quantized" and {"tile", "staged", "bpb32", f"u{u}"} <= w)
    for u in (1, 2, 4, 8):
        for x in (0, 1):
            need(f"gather u{u} xcd{x}", lambda c, w, p: {"gather", f"u{u}", f"xcd{x}"} <= w)
    need("gather two passes", lambda c, w, p: {"gather", "f32", "passes2"} <= w and c.dims[0] == 512)
    need("gather slice", lambda c, w, p: {"gather", "slice"} <= w)
    for entry in ("psw_grad", "mean_grad", "widen", "atomic"):
        need(f"base {entry}", lambda c, w, p: c.entry == entry and {"base", "bpb32", "xcd0"} <= w)
    # environment groups
    env = lambda c, name, value: c.env.get(name) == value                                       # noqa: E731
    need("TILE_MAJOR: xcd_affine 2, ordered", lambda c, w, p: env(c, "PARAM_AMD_FWD_TILE_MAJOR", 1) and {"tile", "xcd2", "ordered-bitonic"} <= w)
    need("TILE_MAJOR: xcd_affine 2, rank", lambda c, w, p: env(c, "PARAM_AMD_FWD_TILE_MAJOR", 1) and {"tile", "xcd2", "ordered-rank"} <= w)
    need("TILE_MAJOR: xcd_affine 2, flat", lambda c, w, p: env(c, "PARAM_AMD_FWD_TILE_MAJOR", 1) and {"flat", "xcd2"} <= w)
    need("FWD_FLAT=0: short bags on the tile kernel", lambda c, w, p: env(c, "PARAM_AMD_FWD_FLAT", 0) and "tile" in w, 4)
    need("FWD_FLAT=2: pooling 3 on the flat walk", lambda c, w, p: env(c, "PARAM_AMD_FWD_FLAT", 2) and "flat" in w and c.req.N == 3 * c.req.T * c.req.B, 2)
    need("FLAT_COMPACT=0", lambda c, w, p: env(c, "PARAM_AMD_FLAT_COMPACT", 0) and {"flat", "old-grid"} <= w, 4)
    need("FLAT_BAGS=48", lambda c, w, p: env(c, "PARAM_AMD_FLAT_BAGS", 48) and {"flat", "bpb48", "target64"} <= w, 2)
    need("FWD_STAGE=0: forward", lambda c, w, p: env(c, "PARAM_AMD_FWD_STAGE", 0) and {"tile", "plain"} <= w, 2)
    need("FWD_STAGE=0: padded family", lambda c, w, p: env(c, "PARAM_AMD_FWD_STAGE", 0) and {"pad", "plain"} <= w and "max" not in w, 2)
    _f8_conditions(cases, missing)
    _f8s_conditions(cases, missing)
    _anyfmt_conditions(cases, missing)
    assert {c.request for c in S.CASES if c.entry.startswith(("f8s", "anyfmt"))} - {c.request for c in S.CASES if not c.entry.startswith(("f8s", "anyfmt"))} \
        == {"pad600", "ragged8", "many260"}
    assert not missing, missing
    assert len(S.ENV_GROUPS) == 6 and len({tuple(sorted(c.env.items())) for c in S.CASES if c.env}) == 6
    assert all(max(c.req.rows) <= 1000 for c in S.CASES)
    # both index types and, where the dims are equal, both layouts: every case runs them (tests/plan_sweep_worker.py: variants)
    for c in S.CASES:
        v = W.variants(c)
        assert {i for i, _ in v} == {"i64", "i32"} and (len(set(c.dims)) > 1 or c.entry in S.GATHER_ENTRIES
                                                        or {lay for _, lay in v} == {"bd", "tbd"}), c.name


def test_the_padded_requests_serve_max_pooling():
    """the requests of the max cases were drawn for sums: under the max rule each of them still holds a bag whose lookups are all
    padded (+0.0, -1), a bag whose first lookup is padded and a bag that holds a winning row at two positions.  Checked with the rule on
    tables of 8 normal columns; the GPU worker asserts the same on the tables it compares (tests/plan_sweep_worker.py: max_reference)."""
    import numpy as np

    from tests import max_rules as MX

    names = sorted({c.request for c in S.CASES if c.entry == "max"})
    assert set(names) == {"pad100", "pad1100", "pad8", "padfix", "pad_lumpy"}
    for name in names:
        r = S.request(name)
        assert r.pads is not None and any(k is not None for k in r.pads) and r.N <= 11000
        tabs = [np.random.default_rng(70 + t).standard_normal((rows, 8)).astype(np.float32) for t, rows in enumerate(r.rows)]
        vals, args = MX.forward(tabs, r.idx, r.off, r.B, r.pads)
        # (pad_lumpy's bags hold 80 and 100 lookups for the index tile's sake: none is padded throughout)
        assert S.max_conditions(r, vals, args) == (name != "pad_lumpy", True, True), (name, S.max_conditions(r, vals, args))
    lumpy, plain = S.request("pad_lumpy"), S.request("even_lumpy")
    assert np.array_equal(lumpy.lens, plain.lens) and lumpy.rows == plain.rows      # (the plan is a function of the sizes)
