"""Constructed requests for the direct backward of max pooling (tests/test_gpu_max_direct.py, tests/test_max_direct_host.py): hot runs
placed against the piece cuts (every ``max_direct_rules.EXACT_RUN`` pairs from a run's start) and the tile borders (every ``TILE`` sorted
pairs) of param_amd/csrc/embbag_max_bwd.hip.  Pure numpy, fixed seeds.

Every bag holds one or two lookups, so the sorted order is known: pairs ascend by (table, row, bag), a bag that holds a row twice is two
adjacent pairs.  ``max_indices`` is written by hand -- whether a bag wins a column is the case's choice, not a forward's."""
import functools

import numpy as np

ROWS = (40, 17, 300)
TILE = 1024      # kMbTile
PIECE = 256      # kExactRun


class Case:
    """``bags[t]``: table t's bags, each a list of one or two rows; ``win(t, b, row, c)``: whether bag b of table t names ``row`` in column c"""

    def __init__(self, bags, dims=(8, 8, 8), win=None, seed=0, bag_slice=None, pads=(None, None, None)):
        self.B, self.dims, self.pads = len(bags[0]), tuple(dims), tuple(pads)
        assert len(bags) == 3 and all(len(b) == self.B for b in bags) and all(1 <= len(x) <= 2 for b in bags for x in b)
        self.bags = bags
        self.idx = np.array([r for b in bags for x in b for r in x], np.int64)
        self.off = np.concatenate([[0], np.cumsum([len(x) for b in bags for x in b])])[:-1].astype(np.int64)
        self.slice = bag_slice or (0, self.B)
        rng = np.random.default_rng(seed)
        self.grads = [rng.standard_normal((self.B, d)).astype(np.float32) for d in dims]      # (no multiples of a power of two)
        self.args = []
        for t, d in enumerate(dims):
            a = np.full((self.B, d), -1, np.int32)
            for b, x in enumerate(bags[t]):
                if x[0] != self.pads[t]:
                    a[b] = [x[0] if win is None or win(t, b, x[0], c) else -1 for c in range(d)]
            self.args.append(a)

    @functools.cached_property
    def pairs(self):
        """the sorted pairs the device holds: ``[n, 3]`` (table, row, bag), of the slice, without padded lookups"""
        b0, nb = self.slice
        p = [(t, r, b) for t in range(3) for b in range(b0, b0 + nb) for r in self.bags[t][b] if r != self.pads[t]]
        return np.array(sorted(p), np.int64)

    def run(self, t, row):
        """(sorted position of the run's first pair, its pairs)"""
        hit = np.flatnonzero((self.pairs[:, 0] == t) & (self.pairs[:, 1] == row))
        assert hit.size and (np.diff(hit) == 1).all()
        return int(hit[0]), int(hit.size)

    def hot(self):
        """{(table, row): pairs} of the runs longer than a piece"""
        keys, counts = np.unique(self.pairs[:, :2], axis=0, return_counts=True)
        return {(int(k[0]), int(k[1])): int(n) for k, n in zip(keys, counts) if n > PIECE}

    def repeats(self, t, row):
        """run positions k whose pair repeats the bag of the pair in front"""
        s, n = self.run(t, row)
        return [k for k in range(1, n) if self.pairs[s + k, 2] == self.pairs[s + k - 1, 2]]


def fill(n, rows):
    rows = list(rows)
    return [[rows[i % len(rows)]] for i in range(n)]


@functools.lru_cache(maxsize=None)
def repeat(n_low):
    """row 7 of table 1: a run of 600 pairs over 598 bags; the bags at run positions 255 and 511 hold the row twice, so each repeat lies
    across a piece cut.  ``n_low`` bags of table 1 look up rows below 7 and move the run's start: 263 puts it 100 pairs behind a tile border
    (both cuts inside the tile), 85 puts it 768 behind (the cut at run position 256 IS a tile border: the pair in front of the piece is the
    pair in front of the tile).  Every bag wins every column."""
    run = [[7, 7] if k in (255, 510) else [7] for k in range(598)]
    nb = 598 + n_low
    c = Case([fill(nb, range(40)), run + fill(n_low, range(7)), fill(nb, range(300))], seed=600 + n_low)
    s, n = c.run(1, 7)
    assert n == 600 and c.repeats(1, 7) == [256, 512] and s == nb + n_low and s % TILE == {263: 100, 85: 768}[n_low] and set(c.hot()) == {(1, 7)}
    return c


@functools.lru_cache(maxsize=None)
def nothing():
    """row 7 of table 1: a run of 900, four pieces; ``max_indices`` names it for bags of pieces 1 and 3 only, in the columns c with
    (bag + c) % 3 == 0 but never in column 7; pieces 0 and 2 win no column.  Row 3 of table 2: a run of 700 that wins nothing at all.
    Column 0 of table 1's gradient is -0.0 throughout: the row's sum there is -0.0, and +0.0 for a combine that starts from +0.0."""
    def win(t, b, row, c):
        if (t, row) == (1, 7):
            return b // PIECE in (1, 3) and (b + c) % 3 == 0 and c != 7
        return (t, row) != (2, 3)
    c = Case([fill(1000, range(40)), fill(900, [7]) + fill(100, range(8, 17)), fill(700, [3]) + fill(300, range(10, 300))], win=win, seed=900)
    c.grads[1][:, 0] = -0.0
    assert c.hot() == {(1, 7): 900, (2, 3): 700} and c.run(1, 7)[0] % PIECE and not (c.args[2] == 3).any()
    won = np.array([[(c.args[1][p * PIECE:(p + 1) * PIECE, col] == 7).any() for col in range(8)] for p in range(4)])
    assert not won[[0, 2]].any() and won[[1, 3], :7].all() and not won[:, 7].any()
    return c


@functools.lru_cache(maxsize=None)
def far():
    """row 7 of table 1: a run of 5000 pairs that crosses four tile borders; the last tile sees its start 4016 pairs back"""
    c = Case([fill(5100, range(40)), fill(100, range(7)) + fill(5000, [7]), fill(5100, range(300))], seed=5000)
    s, n = c.run(1, 7)
    assert (s, n) == (5200, 5000) and (s + n - 1) // TILE - s // TILE == 4 and (s + n - 1) // TILE * TILE - s == 4016 and set(c.hot()) == {(1, 7)}
    return c


@functools.lru_cache(maxsize=None)
def zero():
    """row 0 of table 0: a run of 2500 pairs from sorted position 0, across two tile borders"""
    c = Case([fill(2500, [0]) + fill(100, range(1, 40)), fill(2600, range(17)), fill(2600, range(300))], seed=2500)
    assert c.run(0, 0) == (0, 2500) and set(c.hot()) == {(0, 0)}
    return c


@functools.lru_cache(maxsize=None)
def sliced():
    """1200 bags a table, the slice is bags 100 .. 999.  Table 0 has padding row 5: 400 bags look it up (300 of them in the slice: the
    device holds that many pairs fewer than the request has lookups), 300 bags look up row 9 (hot).  Row 7 of table 1 is looked up by bags
    0 .. 356: 257 pairs in the slice, one over a piece.  Row 3 of table 2 by bags 744 .. 1199: 256 pairs in the slice, exactly cold."""
    t0 = fill(400, [5]) + fill(300, [9]) + fill(500, range(20, 40))
    t1 = fill(357, [7]) + fill(843, [r for r in range(17) if r != 7])
    t2 = fill(744, range(10, 300)) + fill(456, [3])
    c = Case([t0, t1, t2], seed=1200, bag_slice=(100, 900), pads=(5, None, None))
    assert c.run(1, 7)[1] == 257 and c.run(2, 3)[1] == 256 and c.hot() == {(0, 9): 300, (1, 7): 257}
    assert len(c.pairs) == 3 * 900 - 300 and sum(x == [5] for x in t0) == 400 and c.idx.size == 3600
    return c


@functools.lru_cache(maxsize=None)
def mixed():
    """dims (8, 2048, 32): the slots are sized for 2048 columns and the lane group is 64 lanes; table 0's two pieces of four columns leave
    62 lanes idle, table 1's 512 take eight passes.  Hot runs in tables 0 (600 pairs) and 1 (300)."""
    c = Case([fill(600, [9]) + fill(100, range(20, 40)), fill(300, [7]) + fill(400, range(7)), fill(700, range(300))], dims=(8, 2048, 32), seed=2048)
    assert c.hot() == {(0, 9): 600, (1, 7): 300}
    return c
