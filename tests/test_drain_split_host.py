"""The forward's split last round -- the block -> (table, tile, part) map of the staged bag-count launches -- checked on the CPU.

param_amd/csrc/launch_plan.h computes the map as a pure constexpr function (drain_block_tile: host and device) and decides where a launch
uses it (with_drain_split in plan_forward, resolve_drain_split in the launcher).  drain_split_dump.cpp is a stand-alone program around
that header alone; this test builds it with a plain C++ compiler.

What the map must be, for every (T, tiles_per_table, R, S):
  * a bijection: every (table, tile) is served, a tile of an XCD's last round (its last slots mod R slots) by S blocks with parts
    0 .. S - 1, every other tile by one;
  * XCD x = block % 8 serves tables t % 8 == x only, the appended blocks included;
  * the first T x tiles_per_table blocks are in the order of block_to_tile's xcd_affine == 1 branch, block for block -- with S = 1 that is
    the whole map.
(The whole-round table passes the map first had, and their cases here, left with their code: profiles/fwd_round_timeline.md.)
The reported plan members are pinned by tests/test_launch_plan_host.py and tests/test_plan_sweep_host.py, which stay as they are; here the
benchmark request's twelve are compared once more next to the two unreported ones."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
XCDS = 8

TABLES = (8, 16, 48)
TILES = (1, 3, 4, 5, 11, 256)
RESIDENT = (1, 4, 224, 256)
SPLITS = (1, 2, 4)


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("drain_split") / "drain_split_dump")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "param_amd", "csrc"), os.path.join(HERE, "drain_split_dump.cpp"), "-o", exe], check=True)

    def run(lines):
        return subprocess.run([exe], input="".join(x + "\n" for x in lines), capture_output=True, text=True, check=True).stdout.splitlines()

    return run


def _maps(dump, cases):
    """{case: [(table, tile, part, parts) per block]} for cases (T, tiles, R, S)"""
    out = iter(dump(["map %d %d %d %d" % c for c in cases]))
    res = {}
    for c in cases:
        head = next(out).split()
        assert head[0] == "grid"
        res[c] = [tuple(int(x) for x in next(out).split()) for _ in range(int(head[1]))]
    assert next(out, None) is None
    return res


def _plain_order(T, tiles, bid):
    """block_to_tile's xcd_affine == 1 branch (common.h)"""
    xcd, slot = bid % XCDS, bid // XCDS
    return xcd + XCDS * (slot // tiles), slot % tiles


@pytest.mark.parametrize("T", TABLES)
def test_block_map_is_a_bijection_on_the_own_xcd_in_the_plain_order(dump, T):
    cases = [(T, tiles, R, S) for tiles, R, S in itertools.product(TILES, RESIDENT, SPLITS)]
    for case, blocks in _maps(dump, cases).items():
        _, tiles, R, S = case
        slots = T // XCDS * tiles
        drain = slots % R if S > 1 else 0
        assert len(blocks) == T * tiles + XCDS * drain * (S - 1), case
        assert [b[:2] for b in blocks[:T * tiles]] == [_plain_order(T, tiles, bid) for bid in range(T * tiles)], case
        seen = {}
        for bid, (t, tile, part, parts) in enumerate(blocks):
            assert 0 <= t < T and 0 <= tile < tiles and 0 <= part < parts and parts in (1, S), (case, bid)
            assert t % XCDS == bid % XCDS, (case, bid)                  # every XCD gets only its own tables
            assert (bid >= T * tiles) == (part > 0), (case, bid)         # the appended blocks are the parts behind the first
            assert (t, tile, part) not in seen, (case, bid, seen[(t, tile, part)])
            seen[(t, tile, part)] = bid
        per_tile = {}
        for (t, tile, part), bid in seen.items():
            per_tile.setdefault((t, tile), []).append((part, blocks[bid][3]))
        assert len(per_tile) == T * tiles, case                          # every (table, tile) is served ...
        split = 0
        for key, parts in per_tile.items():
            n = parts[0][1]
            assert sorted(parts) == [(q, n) for q in range(n)], (case, key)   # ... by all of its parts, each once
            split += n > 1
        assert split == XCDS * drain, case                               # the last round of every XCD, nothing else, is split
        for x in range(XCDS if drain else 0):                            # ... and it is the XCD's LAST slots in dispatch order
            own = [b for bid, b in enumerate(blocks[:T * tiles]) if bid % XCDS == x]
            assert [b[3] for b in own] == [1] * (slots - drain) + [S] * drain, (case, x)


def test_a_launch_splits_only_where_it_has_more_than_one_round_and_a_partial_last_one(dump):
    rows = {
        (48, 256, 224, 4): (224, 4, XCDS * 192 * 3),   # the benchmark: 1536 tiles per XCD, the last 1536 mod 224 = 192 split four ways
        (48, 256, 224, 2): (224, 2, XCDS * 192),
        (48, 256, 224, 1): (0, 0, 0),
        (48, 256, 224, 0): (0, 0, 0),
        (48, 256, 256, 4): (0, 0, 0),                  # 1536 = 6 whole rounds of 256
        (48, 256, 0, 4): (0, 0, 0),                    # residency unknown
        (8, 224, 224, 4): (0, 0, 0),                   # one round
        (8, 225, 224, 4): (224, 4, XCDS * 1 * 3),
        (16, 11, 4, 4): (4, 4, XCDS * 2 * 3),
        (16, 4, 4, 4): (0, 0, 0),                      # two whole rounds
        (16, 2, 4, 4): (0, 0, 0),                      # grid <= 8 R
        (26, 256, 224, 4): (0, 0, 0),                  # T % 8 != 0 is not the t % 8 order
    }
    out = dump(["resolve %d %d %d %d" % c for c in rows])
    assert [tuple(int(x) for x in line.split()) for line in out] == list(rows.values())


def test_the_plan_asks_for_the_split_where_it_is_scoped(dump):
    F32, BF16 = 0, 1
    bench = (256, 32, 1280, 1, 0, 0, 128, 32, 0, 0, 0, 2)          # the benchmark's reported plan (tests/launch_plan_host.json pins it)
    N = 48 * 8192 * 20
    # T B N D dtype weighted bags_per_block xcd_affine stage_out | drain_split round_wgs -> the twelve, round_wgs, drain_split
    cases = [
        ((48, 8192, N, 128, F32, 0, 0, -1, -1, 4, 0), bench + (0, 4)),
        ((48, 8192, N, 128, F32, 0, 0, -1, -1, 0, 0), bench + (0, 1)),
        ((48, 8192, N, 128, F32, 0, 0, -1, -1, 64, 200), bench + (200, 4)),    # S <= bags_per_block / NG
        ((48, 8192, N, 128, F32, 0, 0, -1, -1, 3, 7), bench + (7, 2)),         # a power of two
        ((48, 8192, N, 128, F32, 0, 0, -1, -1, 1, 7), bench + (0, 1)),
    ]
    out = dump(["plan " + " ".join(map(str, c)) for c, _ in cases])
    assert [tuple(int(x) for x in line.split()) for line in out] == [w for _, w in cases]
    # never for: xcd_affine 0, unstaged tiles, ragged (ordered) requests, the flat walk, table counts off the t % 8 order
    off = [
        (48, 8192, N, 128, F32, 0, 0, 0, -1, 4, 4),
        (48, 8192, N, 128, F32, 0, 0, -1, 0, 4, 4),
        (48, 8192, N + 1, 128, F32, 0, 32, -1, -1, 4, 4),
        (48, 8192, 48 * 8192 * 2, 128, F32, 0, 0, -1, -1, 4, 4),
        (26, 8192, 26 * 8192 * 20, 128, BF16, 1, 0, -1, -1, 4, 4),
    ]
    for c, line in zip(off, dump(["plan " + " ".join(map(str, c)) for c in off])):
        assert [int(x) for x in line.split()][12:] == [0, 0], c
