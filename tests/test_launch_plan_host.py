"""The launch geometry of every forward entry point, pinned on the CPU.

param_amd/csrc/launch_plan.h plans a request's geometry -- tile, index-tile capacity, XCD mapping, burst buffer, flat-walk grid, unroll
-- as pure functions of (request, element type, knob snapshot); capi.hip copies a plan into the kernel arguments.  launch_plan_dump.cpp
is a stand-alone program around that header alone; this test builds it with a plain C++ compiler, runs every row of
launch_plan_host.json through it and compares the twelve plan members.

Where the expected rows come from: NOT from launch_plan.h.  They were printed by the commit before the header existed, whose capi.hip
held the geometry in tile_bags / fill_params / plan_forward / plan_padded_forward / small_request_unroll and an edit inside
pm_embbag_fwd_quantized.  A host-only translation unit #included that capi.hip, was compiled with `hipcc --offload-host-only` and
linked with unresolved symbols ignored (no launcher is ever called), set the setters through pm_set_tuning / pm_set_forward_tuning and
called make_params, small_request_unroll and plan_padded_forward for each row -- one process per environment setting, because the
switches are read once per process.  That harness depends on internal names of one commit and is not kept; to regenerate a row after a
deliberate change of a rule, change the row by hand and say why in the commit.

Fields of the JSON: `requests` and `tunings` name the inputs (a tuning lists only what differs from `tuning_defaults`: what the setters
were given, then the environment's values), `rows` are [request, tuning, kind, plan]."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SPEC = json.load(open(os.path.join(HERE, "launch_plan_host.json")))
PLAN = SPEC["plan_fields"]


def _line(request, tuning, kind):
    t = SPEC["tunings"][tuning] if isinstance(tuning, str) else tuning
    assert not set(t) - set(SPEC["tuning_fields"]), t
    values = [t.get(f, d) for f, d in zip(SPEC["tuning_fields"], SPEC["tuning_defaults"])]
    return " ".join(map(str, [SPEC["kinds"].index(kind)] + SPEC["requests"][request] + values))


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "param_amd", "csrc"), os.path.join(HERE, "launch_plan_dump.cpp"), "-o", exe], check=True)

    def run(cases):
        text = "".join(_line(*c) + "\n" for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(cases)
        return [[int(x) for x in line.split()] for line in out]

    return run


def test_plans_are_the_pinned_ones(dump):
    rows = SPEC["rows"]
    got = dump([r[:3] for r in rows])
    bad = [(r[:3], dict(zip(PLAN, r[3])), dict(zip(PLAN, g))) for r, g in zip(rows, got) if g != r[3]]
    assert not bad, f"{len(bad)} of {len(rows)} plans differ; the first (case, expected, got): {bad[0]}"


def test_flat_target_below_one_plans_as_one(dump):
    """PARAM_AMD_FLAT_TARGET=0, a negative value or text (which reads as 0) divided by zero in the grid estimate of the even short-bag
    branch; every site now sees 1.  The commit the other rows come from cannot print this one."""
    cases = [("short_l1", {"env_flat_target": v}, kind) for v in (1, 0, -5) for kind in ("forward", "quantized")]
    got = dump(cases)
    assert got[0][PLAN.index("flat_bags")] > 0 and got[0][PLAN.index("flat_target")] == 1
    assert got[2:4] == got[0:2] and got[4:6] == got[0:2]


def test_the_fixture_reaches_every_branch():
    """conditions on the fixture, so that it cannot quietly stop covering a rule (the issue's list)"""
    req = {name: dict(zip(SPEC["request_fields"], v)) for name, v in SPEC["requests"].items()}
    rows = [(req[r], t, kind, dict(zip(PLAN, plan))) for r, t, kind, plan in SPEC["rows"]]

    def even(q):
        return q["num_indices"] % (q["num_tables"] * q["batch"]) == 0

    def mixed(q):
        return 0 < q["min_dim"] < q["max_dim"]

    conditions = {
        "ordered": lambda q, t, p: p["ordered"] == 1,
        "flat walk, even request": lambda q, t, p: p["flat_bags"] > 0 and even(q) and not mixed(q),
        "flat walk, uneven request": lambda q, t, p: p["flat_bags"] > 0 and not even(q) and not mixed(q),
        "flat walk, mixed dims": lambda q, t, p: p["flat_bags"] > 0 and mixed(q),
        "flat walk, old grid": lambda q, t, p: p["flat_bags"] > 0 and p["flat_compact"] == 0,
        "not staged under default knobs": lambda q, t, p: t == "default" and p["stage_out"] == 0,
    }
    conditions.update({f"xcd_affine {v}": (lambda q, t, p, v=v: p["xcd_affine"] == v) for v in (0, 1, 2, 3)})
    conditions.update({f"unroll {v}": (lambda q, t, p, v=v: p["unroll"] == v) for v in (2, 4, 8)})
    conditions.update({f"idx_cap {v}": (lambda q, t, p, v=v: p["idx_cap"] == v) for v in (512, 1024, 4096)})
    forward = [(q, t, p) for q, t, kind, p in rows if kind == "forward"]
    missing = [name for name, cond in conditions.items() if not any(cond(*r) for r in forward)]
    assert not missing, missing
    assert {kind for _, _, kind, _ in rows} == set(SPEC["kinds"])
    assert os.path.getsize(os.path.join(HERE, "launch_plan_host.json")) < os.path.getsize(os.path.join(HERE, "call_trace_host.json"))
