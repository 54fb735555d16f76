"""The forward's split last round on a real MI355X (``pytest -m gpu``): same bits as with the switch off.

The split changes which workgroup pools which bags, never a sum: every bag is pooled by one lane group in index order.
tests/drain_split_worker.py runs 16 tables x (11 * 32 - 5 | 4 * 32 | 2 * 32) bags x pooling 20 on explicit 32-bag tiles, fp32 and bf16
tables, with and without per_sample_weights, both output layouts and a bag slice, compares every output with the C oracle bit for bit
and reports a digest of its bytes.  The switches are read once per process, so each setting is a process of its own; with 4 resident
workgroups per XCD forced, the small requests have several rounds per XCD, a partial last round and a partial last tile.

One test is one setting; its outputs must equal the oracle's (checked in the child) and the digests of the child with the switch off.
Once a child has died of a signal or run into its limit no later child is started."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("PARAM_AMD_FWD_DRAIN_SPLIT", "PARAM_AMD_FWD_ROUND_WGS")
OFF = (0, 0)
SETTINGS = {"split_in_four": (4, 4), "split_in_two": (2, 4)}
CHILD_SECONDS = 120          # a child imports torch, loads the library and runs 32 small launches: seconds
_child_died = []
_off = {}


def _child(setting):
    assert not _child_died, f"not started: the child of {_child_died[0]} did not end by itself"
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(dict(zip(SWITCHES, map(str, setting))))
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    try:
        r = subprocess.run([sys.executable, "-m", "tests.drain_split_worker"], env=env, cwd=ROOT, capture_output=True, text=True,
                           timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired:
        _child_died.append(setting)
        raise AssertionError(f"{setting}: the child ran into its limit of {CHILD_SECONDS} s")
    if r.returncode < 0 or r.returncode in (134, 139):
        _child_died.append(setting)
    assert r.returncode in (0, 1), f"{setting}: exit status {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert not res["failures"], f"{setting}: {len(res['failures'])} failed, the first: {res['failures'][0]}"
    assert len(res["digests"]) == 32
    return res["digests"]


def _switches_off():
    if "digests" not in _off:
        _off["digests"] = _child(OFF)
    return _off["digests"]


def test_switch_off_equals_the_oracle():
    _switches_off()


@pytest.mark.parametrize("name", list(SETTINGS))
def test_same_bits_as_with_the_switch_off(name):
    want = _switches_off()
    got = _child(SETTINGS[name])
    assert got.keys() == want.keys()
    bad = [k for k in want if got[k] != want[k]]
    assert not bad, f"{name}: {len(bad)} outputs differ from the switch-off bytes, the first: {bad[0]}"
