"""Every forward kernel variant the launch plan can choose, run on a real MI355X (``pytest -m gpu``).

The forward is several hundred template instances -- ``embbag_fwd_kernel<WT, G, UNROLL, WEIGHTED, ORDERED, STAGE>``,
``embbag_fwd_flat_kernel<WT, G, UNROLL, WEIGHTED>``, ``pad_fwd_kernel<WT, G, WEIGHTED, MEAN, OT>``, ``max_fwd_kernel<WT, G, OT, WITH_ARG>``
and the row gather with an unroll of its own -- and param_amd/csrc/launch_plan.h picks one from a request's sizes and the tuning knobs.
Small requests under default knobs all land in one corner of that plan (one bag per lane group, the flat walk, unroll 2, 4 or 8).
The cases of tests/plan_sweep.py set an explicit
tile, unroll, XCD mapping, grid or environment switch so that a few hundred bags over 1000-row tables take the variants the product
takes at benchmark size: the longest-bag-first kernel with its bitonic and rank-counting orders, staged 32-bag tiles, unrolls 1, 3 and
6 with their tails, 1024-bag padded tiles and their launcher's 64 KB fallback, the old flat grid, tile-major order.

For every case: the knobs are set, ``pm_embbag_plan`` must report the plan pinned in tests/plan_sweep_host.json (so the comparison is
known to be of THAT variant, environment included), the entry point runs with int64 and int32 indices and both layouts, and the output
must equal the rule of its operation bit for bit -- ``coracle.fwd_batched``, ``padding_rules.forward``, ``mean_rules.forward``,
``out16_rules.forward``, ``max_rules.forward`` (values and ``max_indices``, with and without the arg-max output), ``embedding_rules.forward``,
the rowquant reference and the default-knob bytes; a batch slice writes into a NaN canvas that must stay NaN elsewhere.  The FP8 lookups
(``f8_fwd_kernel<WT, G, U, WEIGHTED, MEAN, OT>``, ``embedding_gather_f8_kernel<WT, OT, G, U>``; tests/test_gpu_f8.py runs one tile a table)
have their multi-tile paths pinned here: groups ``f8_*`` hold ``Float8BatchedEmbeddingBagMI355`` to ``f8_rules.forward`` / ``sequence``
under ``pm_embbag_f8_plan`` / ``pm_embedding_gather_f8_plan`` -- tiles behind tile 0, the block orders, compaction over several waves and
rounds, 1024-bag and direct tiles, every (lane group, rows in flight) pair of both kernels.  The scaled FP8 lookups
(``f8s_fwd_kernel<WT, G, U, WEIGHTED, MEAN, ROW, OT>``, ``embedding_gather_f8s_kernel``; tests/test_gpu_f8s.py runs one table and one tile)
are pinned in groups ``f8s_*``: the same shapes with row exponents -- the exponent byte compacted next to its index over ten rounds, loaded
next to the index of a direct tile, picked per table under every block order, the burst behind the exponent bytes -- and with a table
exponent, under ``pm_embbag_f8_scaled_plan``, whose ``stage_out`` must be 0 on the one side of the 64 KiB edge (``f8s_edge``) and the
row's width on the other; the un-pooled lookup's ``sequence_plan`` must equal an unscaled module's.  The mixed-format lookups
(``anyfmt_fwd_kernel<G, WEIGHTED, OT>``, ``anyfmt_gather_kernel<OT, G>``; tests/test_gpu_anyfmt.py runs G = 8, 32 and 64 with one tile a
table) are pinned in groups ``any_*``: every format at every lane-group width, weighted and not, over several tiles a table whose
neighbours differ in format, each format's tail loop, direct tiles of an FP8, a 4-bit and an fp32 table, D = 520 and 2048, 1024-bag
tiles, block orders and slices; the gather with seven formats in one tile of positions and with more tables than it stages borders for.  The entry
points on the base plan equal their default-knob bits and their rule; the one non-deterministic entry, the alternates' atomic backward, is held to the fuzz test's 1e-5 bar.  No tolerance is new.

One test is one group: a few dozen launches on one small request.  The groups with an environment setting run in a fresh child each
(``python -m tests.plan_sweep_worker GROUP``), one after another, each under its own time limit; once a child has died of a signal or
run into its limit no later child is started."""
import os
import subprocess
import sys

import pytest

from tests import plan_sweep as S
from tests import plan_sweep_worker as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_SECONDS = 120          # a child imports torch, loads the library and runs at most a dozen small launches: seconds
_child_died = []             # the first group that ended by a signal, an abort, its time limit or a HIP error: nothing is started after it


@pytest.fixture(autouse=True)
def _default_knobs():
    yield
    import param_amd

    param_amd.set_tuning()
    param_amd.set_forward_tuning()


@pytest.mark.parametrize("group", [g for g in S.GROUPS if g not in S.ENV_GROUPS])
def test_group_same_bits_under_its_plan(group, coracle):
    assert not _child_died, f"not started: {_child_died[0]} ended in an error of the device, not of a comparison"
    try:
        failures = W.run_group(group, coracle)
    except AssertionError:
        raise
    except BaseException:                  # a HIP error: no later group launches anything on this device
        _child_died.append(group)
        raise
    assert not failures, f"{len(failures)} failed, the first: {failures[0]}"


@pytest.mark.parametrize("group", S.ENV_GROUPS)
def test_environment_group_in_a_fresh_process(group):
    assert not _child_died, f"not started: the child of {_child_died[0]} did not end by itself"
    setting = next(c.env for c in S.CASES if c.group == group)
    env = {k: v for k, v in os.environ.items() if k not in S.ENV}
    env.update({k: str(v) for k, v in setting.items()})
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    try:
        r = subprocess.run([sys.executable, "-m", "tests.plan_sweep_worker", group], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired:
        _child_died.append(group)
        raise AssertionError(f"{group}: the child ran into its limit of {CHILD_SECONDS} s")
    if r.returncode < 0 or r.returncode in (134, 139):
        _child_died.append(group)
    assert r.returncode == 0, f"{group}: exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    assert f"{group}: 0 failures" in r.stdout
