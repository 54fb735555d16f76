"""The case list of the plan sweep: small requests that, with an explicit tuning knob or an environment switch, make the library plan
every forward kernel variant param_amd/csrc/launch_plan.h can choose -- the variants the product takes at benchmark size.

Pure numpy, no GPU, fixed seeds.  tests/test_plan_sweep_host.py plans every case on the CPU (tests/launch_plan_dump.cpp) and pins the
plans in tests/plan_sweep_host.json; tests/test_gpu_plan_sweep.py (and tests/plan_sweep_worker.py for the environment groups) asserts
that ``pm_embbag_plan`` reports that very plan on the device's host, runs the entry point and compares bits with the rule of the
operation.  A plan is a function of a request's SIZES and the knobs only, which is why a few hundred bags over 1000-row tables reach
what 8192 bags over 10 M-row tables reach.

A case names its entry point, table dtype / dims / rows, request, the arguments of ``set_tuning`` and ``set_forward_tuning``, at most
one environment setting (its group then runs in a child process: the switches are read once per process) and, optionally, a batch
slice.  ``label()`` derives the variant from the PLAN, never from the case's intent; ``test_the_sweep_reaches_every_variant`` holds the
list to conditions on those labels."""
import functools

import numpy as np

from tests import padding_rules as P

PLAN_FIELDS = ("tiles_per_table", "bags_per_block", "idx_cap", "xcd_affine", "nt_loads", "ordered", "stage_out", "stage_bags",
               "flat_bags", "flat_target", "flat_compact", "unroll")
GATHER_FIELDS = ("vec", "group_lanes", "tile", "col_passes", "unroll", "lds_borders", "xcd_contiguous", "grid")
# the `kind` codes of tests/launch_plan_dump.cpp (0 .. 4: pm_embbag_plan's PM_PLAN_*; 5: the gather plan)
# (6 .. 8: plan_f8 for 4- / 2-byte output elements and plan_gather_f8, the plans of pm_embbag_f8_plan / pm_embedding_gather_f8_plan)
KIND = {"base": 0, "forward": 1, "quantized": 2, "padded4": 3, "padded2": 4, "gather": 5, "f8_4": 6, "f8_2": 7, "f8_gather": 8}
DTYPE = {"f32": 0, "bf16": 1, "f16": 2}
F8_DTYPE = {"e4m3": 3, "e5m2": 4}                                             # PM_F8E4M3 / PM_F8E5M2: the table kinds of the FP8 entries
VEC = {"f32": 4, "bf16": 8, "f16": 8, "e4m3": 16, "e5m2": 16}                 # columns per lane of the pooled kernels
F8_GATHER_VEC = 4                                                             # ... of the FP8 gather (one dword)
OUT16_CODE = {None: 0, "bf16": 1, "fp16": 2}                                  # PM_F32 / PM_BF16 / PM_F16 of a case's ``out16``
TUNING = ("unroll", "bags_per_block", "xcd_affine", "nt_loads")               # set_tuning's arguments and their "not set"
TUNING_DEFAULT = (0, 0, -1, -1)
FORWARD_TUNING = ("stage_out", "flat_grid", "flat_target")                    # set_forward_tuning's
FORWARD_TUNING_DEFAULT = (-1, -1, -1)
# the environment switches in the order of pm::FwdEnv, with its defaults
ENV = ("PARAM_AMD_FWD_STAGE", "PARAM_AMD_FWD_FLAT", "PARAM_AMD_FLAT_MAXL", "PARAM_AMD_FLAT_TARGET", "PARAM_AMD_FLAT_BAGS",
       "PARAM_AMD_FWD_TILE_MAJOR", "PARAM_AMD_FLAT_COMPACT")
ENV_DEFAULT = (1, 1, 0, 256, 256, -1, 1)
# which plan an entry point launches with (capi.hip); a pair: (fp32 output, 16-bit output) -- pm_embbag_fwd_max plans on the padded
# family's plan for its output element, so the case decides
ENTRY_KIND = {"fwd": "forward", "quantized": "quantized", "padded": "padded4", "mean": "padded4", "out16": "padded2", "gather": "gather",
              "psw_grad": "base", "mean_grad": "base", "widen": "base", "atomic": "base", "max": ("padded4", "padded2"),
              "f8": ("f8_4", "f8_2"), "f8_gather": "f8_gather"}
UNROLLS = (1, 2, 3, 4, 6, 8)
# FP8 pooled: (lane-group width, the D its unroll cases run at, the unroll its mean case runs at)
F8_GROUP_DIMS = ((8, 64, 4), (16, 192, 8), (32, 400, 2), (64, 1024, 4))
K_BLOCK = 256


def group_lanes(max_dim, vec):
    g = 8
    while g < (max_dim + vec - 1) // vec and g < 64:
        g *= 2
    return g


# ---- requests -------------------------------------------------------------------------------------------------------------------
class Request:
    """T tables of ``rows`` rows, B bags each, bag lengths ``lens`` (table-major); indices and weights are drawn on first use"""

    def __init__(self, name, T, B, rows, lens, seed, pads=None, idx=None):
        self.name, self.T, self.B, self.rows, self.seed, self.pads = name, T, B, list(rows), seed, pads
        self.lens = np.asarray(lens, dtype=np.int64)
        assert self.lens.shape == (T * B,) and len(self.rows) == T and max(self.rows) <= 1000
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.N = int(self.off[-1])
        self._idx = idx

    @property
    def idx(self):
        if self._idx is None:
            rng = np.random.default_rng(self.seed + 1)
            per_table = np.add.reduceat(self.lens, np.arange(0, self.T * self.B, self.B))
            self._idx = np.concatenate([rng.integers(0, r, int(n)) for r, n in zip(self.rows, per_table)]).astype(np.int64)
        return self._idx

    @functools.cached_property
    def psw(self):
        return np.random.default_rng(self.seed + 2).standard_normal(self.N).astype(np.float32)


def _ragged_lens(rng, T, B):
    """lengths 0 .. 40 from ten values (many ties), runs of empty bags, ONE bag longer than any index tile (4096 entries)"""
    lens = rng.choice(np.array([0, 1, 2, 3, 5, 8, 13, 21, 34, 40]), T * B)
    for t in range(T):
        lens[t * B + 10 + 7 * t:t * B + 25 + 7 * t] = 0
    lens[B + 37] = 4200
    return lens


@functools.lru_cache(maxsize=None)
def request(name):
    if name in ("even", "even8"):
        # lookups divide evenly over the bags (the planner's "even") without fixed pooling: half the bags hold 0 .. 9 lookups -- every
        # residue of every unroll, in the tail loop alone -- the others 25 .. 40, an average of exactly 20
        T, B = (5, 70) if name == "even" else (8, 70)
        rng = np.random.default_rng(101 + T)
        lens = rng.integers(0, 10, T * B)
        long_ = rng.permutation(T * B)[:T * B // 2]
        lens[long_] += 31
        k = 0
        while lens.sum() != 20 * T * B:
            step = 1 if lens.sum() < 20 * T * B else -1
            if 25 <= lens[long_[k % len(long_)]] + step <= 40:
                lens[long_[k % len(long_)]] += step
            k += 1
        r = Request(name, T, B, [1000, 997, 640, 333, 1000, 64, 1000, 500][:T], lens, 100 + T)
        assert r.N % (T * B) == 0 and all({int(v) % u for v in lens} == set(range(u)) for u in UNROLLS)
        return r
    if name == "even_lumpy":
        # divides evenly (average 20) but one 32-bag tile holds 1600 lookups: more than the 1280 entries a staged tile's index tile is
        # sized for, so that tile reads its indices from the request
        T, B = 3, 96
        lens = np.zeros(T * B, dtype=np.int64)
        lens[32:64:2] = 100
        rest = [b for b in range(0, T * B, 4) if not 32 <= b < 64][:52]
        lens[rest] = 80
        r = Request(name, T, B, [1000, 500, 250], lens, 150)
        assert r.N == 20 * T * B and lens[32:64].sum() > 1280
        return r
    if name in ("ragged", "ragged300"):
        T, B = 3, 100 if name == "ragged" else 300
        lens = _ragged_lens(np.random.default_rng(200 + B), T, B)
        if lens.sum() % 2 == 0:
            lens[3] += 1
        r = Request(name, T, B, [1000, 777, 123], lens, 200 + B)
        assert r.N % 2 == 1 and r.N % (T * B) != 0 and B % 32 != 0 and lens.max() > 4096
        return r
    if name in ("short1", "short2"):
        L = int(name[-1])
        return Request(name, 8, 512, [1000] * 8, np.full(8 * 512, L), 300 + L)
    if name == "mixed_even":
        return Request(name, 3, 100, [1000, 500, 250], np.full(300, 3), 400)
    if name == "mixed_ragged":
        lens = np.random.default_rng(401).integers(0, 8, 300)
        lens[5:20] = 0
        if lens.sum() % 300 == 0:
            lens[0] += 1
        return Request(name, 3, 100, [1000, 500, 250], lens, 401)
    if name == "pad_lumpy":
        # even_lumpy's bag lengths with padding rows: the plan is even_lumpy's (a staged tile's index tile holds 1280 entries), the
        # 32-bag tile of 1600 lookups reads its indices -- 40 % of them table 0's padding row -- from the request
        T, B, rows = 3, 96, [1000, 500, 250]
        lens = request("even_lumpy").lens
        pads = [5, rows[1] - 1, None]
        rng = np.random.default_rng(550)
        idx = np.concatenate([rng.integers(0, r, int(n)) for r, n in zip(rows, np.add.reduceat(lens, np.arange(0, T * B, B)))]).astype(np.int64)
        for t, k in enumerate(pads):
            if k is not None:
                lo, hi = int(lens[:t * B].sum()), int(lens[:(t + 1) * B].sum())
                idx[lo:hi][rng.random(hi - lo) < 0.4] = k
        r = Request(name, T, B, rows, lens, 550, pads=pads, idx=idx)
        assert r.N == 20 * T * B and lens[32:64].sum() > 1280 and 500 < (idx[r.off[32]:r.off[64]] == 5).sum() < 800
        return r
    if name.startswith("pad"):
        # about 40 % of the lookups of a table with a padding row are that row (padding_rules.padded_request)
        T, B, rows, kw = {"pad100": (3, 100, [1000, 500, 250], dict(max_len=9)), "pad1100": (2, 1100, [1000, 300], dict(max_len=5)),
                          "pad8": (8, 40, [1000, 500, 250, 125, 1000, 500, 250, 125], dict(max_len=9)),
                          "padfix": (3, 100, [1000, 500, 250], dict(fixed=4))}[name]
        pads = [5, rows[1] - 1] + [None if t % 2 == 0 else 0 for t in range(2, T)]
        idx, off = P.padded_request(np.random.default_rng(500 + B + T), rows, B, pads, **kw)
        r = Request(name, T, B, rows, np.diff(off), 500 + B + T, pads=pads, idx=idx)
        share = P.padded_mask(idx, off, T, B, pads).mean()
        assert 0.2 < share < 0.45, share
        return r
    if name.startswith("auto"):
        # product scale, no knob set: about 1.3 M lookups over 1000-row tables
        T, B = {"auto48": (48, 1376), "auto26": (26, 2560), "auto16r": (16, 4100)}[name]
        if name == "auto16r":
            lens = np.random.default_rng(600).integers(0, 41, T * B)
            k = 0
            while lens.sum() != 1312003:
                step = 1 if lens.sum() < 1312003 else -1
                if 0 <= lens[k % (T * B)] + step <= 40:
                    lens[k % (T * B)] += step
                k += 7
        else:
            lens = np.full(T * B, 20)
        return Request(name, T, B, [1000 - (t % 7) for t in range(T)], lens, 600 + T)
    raise KeyError(name)


def max_conditions(r, vals, args):
    """What a padded request is there for under max pooling, read off the rule's result on some tables (``vals`` / ``args``: per table
    ``[B, D]``, tests/max_rules.py: forward) -> three booleans: a bag all of whose lookups are padded gives +0.0 and -1; a bag's first
    lookup is padded and a later one is kept; a bag holds the row that won a column at two positions."""
    all_padded = first_padded = twice = False
    for t in range(r.T):
        k = -1 if r.pads is None or r.pads[t] is None else r.pads[t]
        for b in range(r.B):
            bag = r.idx[r.off[t * r.B + b]:r.off[t * r.B + b + 1]]
            kept = bag[bag != k]
            if bag.size and not kept.size:
                all_padded |= bool((np.ascontiguousarray(vals[t][b]).view(np.uint32) == 0).all() and (args[t][b] == -1).all())
            first_padded |= bool(bag.size and bag[0] == k and kept.size)
            twice |= any((kept == a).sum() >= 2 for a in np.unique(args[t][b]))
    return all_padded, first_padded, twice


# ---- cases ----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, group, entry, request, kind="f32", dims=128, tuning=None, forward=None, env=None, weighted=False,
                 bag_slice=None, out16=None, mean=False, bits=None):
        self.name, self.group, self.entry, self.request, self.kind = name, group, entry, request, kind
        self.tuning, self.forward, self.env = dict(tuning or {}), dict(forward or {}), dict(env or {})
        self.weighted, self.bag_slice, self.out16, self.mean, self.bits = weighted, bag_slice, out16, mean, bits
        self._dims = dims
        assert not set(self.tuning) - set(TUNING) and not set(self.forward) - set(FORWARD_TUNING) and not set(self.env) - set(ENV)
        assert entry in ENTRY_KIND and not (mean and weighted) and not (entry == "max" and (weighted or mean))
        # an FP8 entry has FP8 tables (dims: multiples of 16 in [16, 2048]) and nothing else has
        assert (kind in F8_DTYPE and all(d % 16 == 0 and 16 <= d <= 2048 for d in self.dims)) if entry.startswith("f8") else kind in DTYPE

    @property
    def req(self):
        return request(self.request)

    @property
    def dims(self):
        return [self._dims] * self.req.T if isinstance(self._dims, int) else list(self._dims)

    @property
    def plan_kind(self):
        kind = ENTRY_KIND[self.entry]
        return kind if isinstance(kind, str) else kind[self.out16 is not None]

    @property
    def bags(self):
        """(bag_begin, bag_count)"""
        return self.bag_slice or (0, self.req.B)

    @property
    def plan_weighted(self):
        """whether the request the entry point plans for carries weights (the gather, the weights' gradient and the mean scaling
        build theirs without)"""
        return bool(self.weighted and self.entry not in ("gather", "f8_gather", "psw_grad", "mean_grad"))

    @property
    def dtype_code(self):
        """the library's code of the table element (``weight_dtype``)"""
        return F8_DTYPE[self.kind] if self.kind in F8_DTYPE else DTYPE[self.kind]

    def tuning_args(self):
        return [self.tuning.get(f, d) for f, d in zip(TUNING, TUNING_DEFAULT)]

    def forward_args(self):
        return [self.forward.get(f, d) for f, d in zip(FORWARD_TUNING, FORWARD_TUNING_DEFAULT)]

    def dump_line(self):
        """the case as tests/launch_plan_dump.cpp reads it.  min_dim: the modules always pass the narrowest table's width."""
        r, (b0, n) = self.req, self.bags
        weighted = int(self.plan_weighted)
        env = [int(self.env.get(f, d)) for f, d in zip(ENV, ENV_DEFAULT)]
        env[0] = 0 if str(self.env.get(ENV[0], "1")).startswith("0") else 1
        v = [KIND[self.plan_kind], r.T, r.B, r.N, b0, n, max(self.dims), min(self.dims), self.dtype_code, weighted, 0, 0, 0]
        return " ".join(map(str, v + self.tuning_args() + self.forward_args() + env))


def label(case, plan):
    """the variant a plan selects, as a set of words; what depends on the request's own offsets (``direct``: some tile's lookups
    exceed the index tile and are read from the request; ``partial``: the last tile of a table is not full) is derived from them"""
    r, (b0, n) = case.req, case.bags
    G = group_lanes(max(case.dims), VEC[case.kind])
    if case.entry.startswith("f8"):
        return f8_label(case, plan)
    if case.plan_kind == "gather":
        p = dict(zip(GATHER_FIELDS, plan))
        return {"gather", case.kind, f"G{p['group_lanes']}", f"u{p['unroll']}", f"passes{p['col_passes']}", f"xcd{p['xcd_contiguous']}",
                "lds_borders" if p["lds_borders"] else "global_borders"} | ({"slice"} if case.bag_slice else set())
    p = dict(zip(PLAN_FIELDS, plan))
    NG = K_BLOCK // G
    family = "base" if case.plan_kind == "base" else "pad" if case.plan_kind.startswith("padded") else "flat" if p["flat_bags"] > 0 else "tile"
    words = {family, case.kind, f"G{G}", f"u{p['unroll']}", "weighted" if case.weighted else "unweighted", f"xcd{p['xcd_affine']}",
             f"nt{p['nt_loads']}", f"bpb{p['bags_per_block']}"}
    if family in ("tile", "pad"):
        words.add(("ordered-bitonic" if p["bags_per_block"] <= 64 else "ordered-rank") if p["ordered"] else "staged" if p["stage_out"] else "plain")
    if case.entry == "max":
        words.add("max")
    if p["bags_per_block"] > NG:
        words.add("tile>NG")
    if family == "flat":
        words |= {"compact" if p["flat_compact"] > 0 else "old-grid", f"grid{p['flat_compact']}", f"target{p['flat_target']}"}
    if case.bag_slice:
        words.add("slice")
    if p["stage_out"] and family != "flat":
        q = max(case.dims) // 4
        words.add("burst-pow2" if q & (q - 1) == 0 else "burst-div")
    # tiles of each table: the flat walk sizes them per table (embbag_fwd.hip: geometry), everything else by bags_per_block
    for t in range(r.T):
        bags = p["bags_per_block"]
        if family == "flat":
            g = max(1, K_BLOCK // p["flat_bags"])
            while g < G and g * VEC[case.kind] < case.dims[t]:
                g *= 2
            lo, hi = r.off[t * r.B + b0], r.off[t * r.B + b0 + n]
            avg = -(-(hi - lo) // n) if n else 1
            bags = max(K_BLOCK // g, min(p["flat_bags"], p["flat_target"] // max(avg, 1)) // (K_BLOCK // g) * (K_BLOCK // g))
        edges = r.off[t * r.B + b0 + np.minimum(np.arange(0, n + bags, bags), n)]
        if (np.diff(edges) > p["idx_cap"]).any():
            words.add("direct")
        if n % bags:
            words.add("partial")
    return words


def f8_label(case, plan):
    """the variant of an FP8 case.  Family words ``f8`` and ``pooled`` / ``unpooled`` (no word of another family: an FP8 case meets no
    condition that is there for another kernel).  ``staged`` / ``plain`` is the output burst, as everywhere.  Read off the request's
    offsets, indices and pads next to the plan, tile by tile as embbag_fwd_f8_kernel.inc walks them -- a tile whose lookups fit the
    index tile compacts them in LDS, 256 entries a round, four waves a round:
      ``rounds>1``  such a tile holds more than 256 entries before compaction;
      ``waves>1``   in one round of such a tile at least two waves hold a kept AND a padded entry each (the prefix over the waves'
                    counts is not the identity, and a wave behind wave 0 keeps an entry);
      ``carry``     such a tile has a bag that is not empty and whose first entry lies in a round after the first, with a padded entry
                    in an earlier round (the bag's bound is read from ``s_pre`` beyond the first round and the carry over rounds counts);
      ``bounds5``   such a tile has 1024 bags (a thread's fifth bound);
      ``direct``    a tile's lookups exceed the index tile: its indices are read from the request;  ``partial``: a last tile is not full.
    The gather: ``partial`` is a last tile of positions that is not full."""
    r, (b0, n) = case.req, case.bags
    words = {"f8", case.kind, "out-" + (case.out16 or "fp32")} | ({"slice"} if case.bag_slice else set())
    if case.entry == "f8_gather":
        p = dict(zip(GATHER_FIELDS, plan))
        assert p["vec"] == F8_GATHER_VEC
        return words | {"unpooled", f"G{p['group_lanes']}", f"u{p['unroll']}", f"passes{p['col_passes']}", f"xcd{p['xcd_contiguous']}",
                        "lds_borders" if p["lds_borders"] else "global_borders"} | ({"partial"} if r.N % p["tile"] else set())
    p = dict(zip(PLAN_FIELDS, plan))
    G = group_lanes(max(case.dims), VEC[case.kind])
    bpb, cap = p["bags_per_block"], p["idx_cap"]
    words |= {"pooled", f"G{G}", f"u{p['unroll']}", "mean" if case.mean else "weighted" if case.weighted else "unweighted", f"xcd{p['xcd_affine']}",
              f"bpb{bpb}", "staged" if p["stage_out"] else "plain", f"passes{-(-max(case.dims) // (G * VEC[case.kind]))}"}
    if bpb > K_BLOCK // G:
        words.add("tile>NG")
    for t in range(r.T):
        pad = -1 if r.pads is None or r.pads[t] is None else r.pads[t]
        for k in range(-(-n // bpb)):
            g0, nb = t * r.B + b0 + k * bpb, min(bpb, n - k * bpb)
            lo, cnt = int(r.off[g0]), int(r.off[g0 + nb] - r.off[g0])
            if nb < bpb:
                words.add("partial")
            if cnt > cap:
                words.add("direct")
                continue
            keep = r.idx[lo:lo + cnt] != pad
            if nb == 1024:
                words.add("bounds5")
            if cnt > K_BLOCK:
                words.add("rounds>1")
            for i0 in range(0, cnt, K_BLOCK):
                waves = [keep[i:min(i + 64, i0 + K_BLOCK)] for i in range(i0, min(i0 + K_BLOCK, cnt), 64)]
                if sum(1 for w in waves if w.any() and not w.all()) >= 2:
                    words.add("waves>1")
            padded_before = np.concatenate([[0], np.cumsum(~keep)])
            first = r.off[g0:g0 + nb] - lo
            later = first[(r.lens[g0:g0 + nb] > 0) & (first >= K_BLOCK)]
            if (padded_before[later // K_BLOCK * K_BLOCK] > 0).any():
                words.add("carry")
    return words


def pad_lds_bytes(case, plan):
    """LDS the padded family's launcher asks for before its 64 KB fallback (embbag_fwd_pad_kernel.inc: launch_pad_w;
    embbag_fwd_max.hip: launch_max_a, never weighted)"""
    p = dict(zip(PLAN_FIELDS, plan))
    tile = (p["bags_per_block"] + 2) // 2 * 2 * 8 + p["idx_cap"] * 4 * (2 if case.weighted else 1)
    tile = (tile + p["idx_cap"] * 2 + 15) // 16 * 16
    return tile + (p["bags_per_block"] * p["stage_out"] * (2 if case.plan_kind == "padded2" else 4) if p["stage_out"] else 0)


def _cases():
    out = []

    def add(*a, **kw):
        out.append(Case(*a, **kw))

    wname = {False: "plain", True: "weighted"}
    # -- tile kernel: every unroll x weighted x {ordered, staged, plain} at fp32, G = 32, a 32-bag tile (NG = 8)
    for u in UNROLLS:
        for w in (False, True):
            add(f"tile_ordered_u{u}_{wname[w]}", "tile_ordered", "fwd", "ragged", tuning=dict(unroll=u, bags_per_block=32), weighted=w)
            add(f"tile_staged_u{u}_{wname[w]}", "tile_even", "fwd", "even", tuning=dict(unroll=u, bags_per_block=32), weighted=w)
            add(f"tile_plain_u{u}_{wname[w]}", "tile_even", "fwd", "even", tuning=dict(unroll=u, bags_per_block=32), forward=dict(stage_out=0),
                weighted=w)
    # -- every dtype x every G, ordered and staged, two bags per lane group, unroll 2
    for kind in DTYPE:
        for G in (8, 16, 32, 64):
            D, bpb = G * VEC[kind] // (2 if G == 8 and kind == "f32" else 1), 2 * K_BLOCK // G
            for w in (False, True):
                add(f"tile_ordered_{kind}_G{G}_{wname[w]}", f"tile_dtype_{kind}", "fwd", "ragged", kind, D, dict(unroll=2, bags_per_block=bpb), weighted=w)
                add(f"tile_staged_{kind}_G{G}_{wname[w]}", f"tile_dtype_{kind}", "fwd", "even", kind, D, dict(unroll=2, bags_per_block=bpb), weighted=w)
    # -- ordered: rank counting at 128 and 1024 bags (bitonic with a partial last tile: tile_ordered_*), each with a direct-index tile
    for bpb in (128, 1024):
        for w in (False, True):
            add(f"tile_rank{bpb}_{wname[w]}", "tile_rank", "fwd", "ragged300", tuning=dict(bags_per_block=bpb), weighted=w)
    # -- staged: a row of 14 pieces (no power of two), the XCD mappings, non-temporal loads, a batch slice
    add("tile_staged_D56", "tile_knobs", "fwd", "even", dims=56, tuning=dict(unroll=2, bags_per_block=32))
    add("tile_staged_xcd0", "tile_knobs", "fwd", "even", tuning=dict(unroll=2, bags_per_block=32, xcd_affine=0))
    add("tile_staged_nt", "tile_knobs", "fwd", "even", tuning=dict(unroll=2, bags_per_block=32, nt_loads=1))
    add("tile_ordered_nt", "tile_knobs", "fwd", "ragged", tuning=dict(unroll=2, bags_per_block=32, nt_loads=1), weighted=True)
    add("tile_staged_direct", "tile_knobs", "fwd", "even_lumpy", tuning=dict(unroll=2, bags_per_block=32))
    add("tile_staged_direct_weighted", "tile_knobs", "fwd", "even_lumpy", tuning=dict(unroll=3, bags_per_block=32), weighted=True)
    add("tile_staged_slice", "tile_knobs", "fwd", "even", tuning=dict(unroll=2, bags_per_block=32), bag_slice=(5, 50))
    add("tile_ordered_slice", "tile_knobs", "fwd", "ragged", tuning=dict(unroll=3, bags_per_block=32), bag_slice=(3, 90), weighted=True)
    for w in (False, True):
        add(f"tile_staged_xcd1_{wname[w]}", "tile_xcd1", "fwd", "even8", tuning=dict(unroll=2, bags_per_block=32), weighted=w)
        add(f"tile_plain_xcd1_{wname[w]}", "tile_xcd1", "fwd", "even8", tuning=dict(unroll=2, bags_per_block=32), forward=dict(stage_out=0), weighted=w)
    # -- flat-walk kernel: every unroll x weighted on one-hot and two-hot tables, the ragged one-bag-per-group route and mixed dims
    for u in UNROLLS:
        for w in (False, True):
            for rq in ("short1", "short2", "ragged"):
                add(f"flat_{rq}_u{u}_{wname[w]}", f"flat_{rq}", "fwd", rq, tuning=dict(unroll=u), weighted=w)
            for rq in ("mixed_even", "mixed_ragged"):
                add(f"flat_{rq}_u{u}_{wname[w]}", "flat_mixed", "fwd", rq, dims=[16, 64, 128], tuning=dict(unroll=u), weighted=w)
    for rq, dims in (("short1", 128), ("ragged", 128), ("mixed_ragged", [16, 64, 128])):
        for grid, fwd in (("grid0", dict(flat_grid=0)), ("grid1", dict(flat_grid=1)), ("grid3", dict(flat_grid=3, flat_target=16))):
            add(f"flat_{rq}_{grid}", "flat_grid", "fwd", rq, dims=dims, forward=fwd, weighted=rq == "ragged")
    add("flat_short2_slice", "flat_grid", "fwd", "short2", bag_slice=(7, 300))
    add("flat_ragged_slice", "flat_grid", "fwd", "ragged", bag_slice=(3, 90), forward=dict(flat_grid=3, flat_target=16))
    for kind in ("bf16", "f16"):
        add(f"flat_short2_{kind}", "flat_grid", "fwd", "short2", kind, 128, weighted=True)
        add(f"flat_mixed_{kind}", "flat_grid", "fwd", "mixed_ragged", kind, [16, 64, 128])
    # -- the padded family: pm_embbag_fwd_padded, pm_embbag_fwd_mean, pm_embbag_fwd_out16 (bf16 and fp16)
    for fam, kw in (("padded", dict(entry="padded")), ("mean", dict(entry="mean", mean=True)), ("out16bf", dict(entry="out16", out16="bf16")),
                    ("out16h", dict(entry="out16", out16="fp16")), ("out16mean", dict(entry="out16", out16="bf16", mean=True))):
        entry = kw.pop("entry")
        ws = (False,) if kw.get("mean") else (False, True)
        for w in ws:
            add(f"{fam}_bpb32_{wname[w]}", f"pad_{fam}", entry, "pad100", tuning=dict(bags_per_block=32), weighted=w, **kw)
            add(f"{fam}_bpb32_unstaged_{wname[w]}", f"pad_{fam}", entry, "pad100", tuning=dict(bags_per_block=32), forward=dict(stage_out=0), weighted=w, **kw)
            # 1024-bag tiles of 4-element (16-bit output: 8-element) rows are staged: 16 KB of burst buffer; weighted, the launcher's
            # LDS passes 64 KB and it falls back to row-by-row stores
            add(f"{fam}_bpb1024_{wname[w]}", f"pad_{fam}_1024", entry, "pad1100", dims=8 if entry == "out16" else 4, tuning=dict(bags_per_block=1024),
                weighted=w, **kw)
        add(f"{fam}_xcd0", f"pad_{fam}", entry, "pad100", tuning=dict(bags_per_block=32, xcd_affine=0), **kw)
        add(f"{fam}_xcd3", f"pad_{fam}", entry, "padfix", tuning=dict(bags_per_block=32), **kw)
        add(f"{fam}_xcd1", f"pad_{fam}_T8", entry, "pad8", tuning=dict(bags_per_block=32), **kw)
        add(f"{fam}_nt", f"pad_{fam}", entry, "pad100", tuning=dict(bags_per_block=32, nt_loads=1), **kw)
        add(f"{fam}_slice", f"pad_{fam}", entry, "pad100", tuning=dict(bags_per_block=32), bag_slice=(5, 70), **kw)
        for G in (8, 16, 64):                                      # (G = 32: every case above)
            add(f"{fam}_G{G}", f"pad_{fam}_G", entry, "pad100", dims=G * 4, tuning=dict(bags_per_block=2 * K_BLOCK // G), **kw)
    # 2-byte against 4-byte burst sizing: 16 bags of 512 bf16 elements fit the 16 KB burst as 2-byte outputs only
    add("padded_D512_bf16_tables", "pad_D512", "padded", "pad100", "bf16", 512, tuning=dict(bags_per_block=16))
    add("out16_D512_bf16_tables", "pad_D512", "out16", "pad100", "bf16", 512, tuning=dict(bags_per_block=16), out16="bf16")
    add("out16_D512_f16_tables", "pad_D512", "out16", "pad100", "f16", 512, tuning=dict(bags_per_block=16), out16="fp16", weighted=True)
    # -- max pooling: pm_embbag_fwd_max on the padded family's plan, fp32 and bf16 output (unweighted: max takes no weights)
    for fam, kw in (("max", {}), ("max16bf", dict(out16="bf16"))):
        add(f"{fam}_bpb32", f"pad_{fam}", "max", "pad100", tuning=dict(bags_per_block=32), **kw)
        add(f"{fam}_bpb32_unstaged", f"pad_{fam}", "max", "pad100", tuning=dict(bags_per_block=32), forward=dict(stage_out=0), **kw)
        add(f"{fam}_bpb1024", f"pad_{fam}_1024", "max", "pad1100", dims=8 if kw else 4, tuning=dict(bags_per_block=1024), **kw)
        add(f"{fam}_xcd0", f"pad_{fam}", "max", "pad100", tuning=dict(bags_per_block=32, xcd_affine=0), **kw)
        add(f"{fam}_xcd3", f"pad_{fam}", "max", "padfix", tuning=dict(bags_per_block=32), **kw)
        add(f"{fam}_xcd1", f"pad_{fam}_T8", "max", "pad8", tuning=dict(bags_per_block=32), **kw)
        add(f"{fam}_nt", f"pad_{fam}", "max", "pad100", tuning=dict(bags_per_block=32, nt_loads=1), **kw)
        add(f"{fam}_slice", f"pad_{fam}", "max", "pad100", tuning=dict(bags_per_block=32), bag_slice=(5, 70), **kw)
        for G in (8, 16, 64):                                      # (G = 32: every case above)
            add(f"{fam}_G{G}", f"pad_{fam}_G", "max", "pad100", dims=G * 4, tuning=dict(bags_per_block=2 * K_BLOCK // G), **kw)
        # fp32 rows of 512: the column loop runs twice at G = 64; 8 bags (two per lane group) fill the burst exactly
        add(f"{fam}_D512_f32_tables", f"pad_{fam}_wide", "max", "pad100", dims=512, tuning=dict(bags_per_block=8), **kw)
        # mixed dims: the forward takes them (only the gradient refuses); the lane group is sized for 128, the narrow tables idle lanes
        add(f"{fam}_mixed_dims", f"pad_{fam}_wide", "max", "pad100", dims=[16, 64, 128], tuning=dict(bags_per_block=32), **kw)
        # a 32-bag tile of 1600 lookups against an index tile of 1280: its indices, padding included, come from the request
        add(f"{fam}_direct", f"pad_{fam}_wide", "max", "pad_lumpy", tuning=dict(bags_per_block=32), **kw)
    add("max16h_bpb32", "pad_max16bf", "max", "pad100", tuning=dict(bags_per_block=32), out16="fp16")
    # 16-bit tables at G = 32 and G = 64, two and four bags per lane group: at D = 512 the 4-byte burst does not fit, the 2-byte one does
    for kind, o16 in (("bf16", "bf16"), ("f16", "fp16")):
        for D in (256, 512):
            add(f"max_D{D}_{kind}_tables", f"pad_max_{kind}_tables", "max", "pad100", kind, D, tuning=dict(bags_per_block=16))
            add(f"max16_D{D}_{kind}_tables", f"pad_max_{kind}_tables", "max", "pad100", kind, D, tuning=dict(bags_per_block=16), out16=o16)
    # -- quantized forward: staged 32-bag tiles under the unrolls no other test runs
    for u, bits in ((1, 8), (3, 4), (6, 8), (6, 2), (3, 16)):
        add(f"quantized_u{u}_{bits}bit", "quantized", "quantized", "even", tuning=dict(unroll=u, bags_per_block=32), bits=bits)
    # -- gather (lookup_sequence): its four unrolls x both tile orders, two column passes, 16-bit rows, a slice
    for u in (1, 2, 4, 8):
        for x in (0, 1):
            add(f"gather_u{u}_xcd{x}", "gather", "gather", "ragged", tuning=dict(unroll=u, xcd_affine=-1 if x else 0))
    add("gather_D512_two_passes", "gather", "gather", "mixed_ragged", dims=512, tuning=dict(unroll=2))
    add("gather_bf16_u1", "gather", "gather", "ragged", "bf16", 128, tuning=dict(unroll=1))
    add("gather_slice_u4", "gather", "gather", "ragged", tuning=dict(unroll=4), bag_slice=(3, 90))
    # -- entry points on the base plan, under an explicit tile and the plain block order
    base = dict(tuning=dict(bags_per_block=32, xcd_affine=0))
    add("base_psw_grad", "base", "psw_grad", "pad100", **base)
    add("base_mean_grad", "base", "mean_grad", "pad100", mean=True, **base)
    add("base_widen_mean_bf16", "base", "widen", "pad100", mean=True, out16="bf16", **base)
    add("base_widen_sum_fp16", "base", "widen", "pad100", out16="fp16", weighted=True, **base)
    add("base_atomic", "base_atomic", "atomic", "ragged", weighted=True, **base)
    # -- no knob set, product scale: the plans of the benchmark shapes
    add("auto_bench_fp32", "auto48", "fwd", "auto48")
    add("auto_t26", "auto26", "fwd", "auto26")
    add("auto_ragged_long", "auto16r", "fwd", "auto16r")
    # -- FP8 tables, pooled: pm_embbag_fwd_f8 on plan_f8, sixteen columns per lane (G = 8 up to D = 128, 64 from D = 528 on), every case
    #    under an explicit tile.  With two bags per lane group a tile's fp32 rows fit the 16 KB burst at G = 8 and D <= 64 only
    #    (bags_per_block * D * 4 = 2 * 256 / G * D * 4 <= 16384), its 16-bit rows up to G = 16.
    def f8(name, group, rq, dims, mode="plain", fmt="e4m3", **kw):
        add(name, group, "f8", rq, fmt, dims, weighted=mode == "weighted", mean=mode == "mean", **kw)

    modes = ("plain", "weighted", "mean")
    # the multi-tile baseline, both formats: pad100 at D = 256 (G = 16), four 32-bag tiles a table, the last of 4 bags, two bags per lane
    # group; fp32 rows do not fit the burst (the plan says plain), 16-bit rows fill it exactly: staged, and with stage_out = 0
    for fmt in F8_DTYPE:
        for mode in modes:
            f8(f"f8_base_{fmt}_{mode}", f"f8_base_{fmt}", "pad100", 256, mode, fmt, tuning=dict(bags_per_block=32))
            f8(f"f8_base_{fmt}_{mode}_bf16", f"f8_base_{fmt}", "pad100", 256, mode, fmt, tuning=dict(bags_per_block=32), out16="bf16")
    for mode in modes:
        f8(f"f8_base_e4m3_{mode}_bf16_unstaged", "f8_base_e4m3", "pad100", 256, mode, tuning=dict(bags_per_block=32), forward=dict(stage_out=0), out16="bf16")
    f8("f8_base_e4m3_plain_fp16", "f8_base_e4m3", "pad100", 256, tuning=dict(bags_per_block=32), out16="fp16")
    # ... and with fp32 output through the burst: 64-bag tiles of D = 64 rows, 18 tiles a table (pad1100), the last of 12 bags
    for mode in modes:
        f8(f"f8_burst_{mode}", "f8_burst", "pad1100", 64, mode, tuning=dict(bags_per_block=64))
        f8(f"f8_burst_{mode}_unstaged", "f8_burst", "pad1100", 64, mode, tuning=dict(bags_per_block=64), forward=dict(stage_out=0))
    # every lane-group width x every depth, two bags per lane group, several tiles a table; mean at one depth per width.  At G = 16
    # and 32 the row ends inside the lane group (12 of 16, 25 of 32 lanes hold columns): the full groups are the baseline and D = 512
    for G, D, mean_u in F8_GROUP_DIMS:
        for u in (2, 4, 8):
            for mode in modes[:2] + (("mean",) if u == mean_u else ()):
                f8(f"f8_G{G}_u{u}_{mode}", f"f8_G{G}", "pad100", D, mode, tuning=dict(unroll=u, bags_per_block=2 * K_BLOCK // G))
    # block orders and a slice that begins and ends inside tiles, on the product's tile: D = 128, one bag per lane group, fp32 burst
    f8("f8_xcd0", "f8_orders", "pad100", 128, tuning=dict(bags_per_block=32, xcd_affine=0))
    f8("f8_xcd1", "f8_orders", "pad8", 128, tuning=dict(bags_per_block=32))
    f8("f8_xcd3", "f8_orders", "padfix", 128, tuning=dict(bags_per_block=32))
    f8("f8_slice", "f8_orders", "pad100", 128, tuning=dict(bags_per_block=32), bag_slice=(5, 70))
    f8("f8_slice_mean", "f8_orders", "pad100", 128, "mean", tuning=dict(bags_per_block=32), bag_slice=(5, 70))
    # 1024-bag tiles: about 2500 entries a tile, ten rounds of compaction, a thread's fifth bound; rows leave one by one (no burst)
    for mode in modes:
        f8(f"f8_bpb1024_{mode}", "f8_1024", "pad1100", 16, mode, tuning=dict(bags_per_block=1024))
        f8(f"f8_bpb1024_{mode}_bf16", "f8_1024", "pad1100", 16, mode, tuning=dict(bags_per_block=1024), out16="bf16")
    # a 32-bag tile of 1600 lookups, 40 % of them padded, read from the request, among compacted tiles of 640
    for mode in modes:
        for u in (2, 8):
            f8(f"f8_direct_u{u}_{mode}", "f8_direct", "pad_lumpy", 128, mode, tuning=dict(unroll=u, bags_per_block=32))
    # mixed dims (the lane group sized for 128), the 2-byte against the 4-byte burst at D = 512, two column passes at G = 64
    f8("f8_mixed_dims", "f8_wide", "pad100", [16, 64, 128], "weighted", tuning=dict(bags_per_block=32))
    f8("f8_D512_bf16", "f8_wide", "pad100", 512, tuning=dict(bags_per_block=16), out16="bf16")
    f8("f8_D512_fp32", "f8_wide", "pad100", 512, tuning=dict(bags_per_block=16))
    f8("f8_D1040_two_passes", "f8_wide", "pad100", 1040, "weighted", tuning=dict(bags_per_block=8))
    # -- FP8 tables, un-pooled: pm_embedding_gather_f8 on plan_gather_f8, four columns per lane (G = D / 4 up to 64)
    def f8g(name, group, rq="ragged", dims=128, fmt="e4m3", **kw):
        add(name, group, "f8_gather", rq, fmt, dims, **kw)

    for G, D in ((8, 16), (16, 64), (32, 128), (64, 256)):
        for u in (1, 2, 4, 8):
            f8g(f"f8_gather_G{G}_u{u}", "f8_gather_GU", dims=D, tuning=dict(unroll=u))
    for u in (1, 2, 4, 8):
        for o16 in ("bf16", "fp16"):
            f8g(f"f8_gather_G32_u{u}_{o16}", "f8_gather_16", tuning=dict(unroll=u), out16=o16)
    f8g("f8_gather_xcd0", "f8_gather_knobs", tuning=dict(unroll=2, xcd_affine=0))
    f8g("f8_gather_D512_two_passes", "f8_gather_knobs", "mixed_ragged", 512, tuning=dict(unroll=4))
    f8g("f8_gather_slice", "f8_gather_knobs", tuning=dict(unroll=4), bag_slice=(3, 90))
    f8g("f8_gather_e5m2", "f8_gather_knobs", fmt="e5m2", tuning=dict(unroll=8))
    # -- the environment switches: one group per setting, each in a process of its own
    e = "env_tile_major"
    add(f"{e}_ordered", e, "fwd", "ragged", tuning=dict(bags_per_block=32), env={"PARAM_AMD_FWD_TILE_MAJOR": 1})
    add(f"{e}_ordered_weighted", e, "fwd", "ragged300", tuning=dict(bags_per_block=128), env={"PARAM_AMD_FWD_TILE_MAJOR": 1}, weighted=True)
    add(f"{e}_flat", e, "fwd", "ragged", env={"PARAM_AMD_FWD_TILE_MAJOR": 1})
    e = "env_flat_off"
    for rq, dims in (("short1", 128), ("short2", 128), ("ragged", 128), ("mixed_ragged", [16, 64, 128])):
        add(f"{e}_{rq}", e, "fwd", rq, dims=dims, env={"PARAM_AMD_FWD_FLAT": 0}, weighted=rq == "short2")
    e = "env_flat_2"
    add(f"{e}_mixed_even", e, "fwd", "mixed_even", dims=128, env={"PARAM_AMD_FWD_FLAT": 2})
    add(f"{e}_mixed_even_weighted", e, "fwd", "mixed_even", dims=128, env={"PARAM_AMD_FWD_FLAT": 2}, weighted=True, tuning=dict(unroll=3))
    add(f"{e}_short2", e, "fwd", "short2", env={"PARAM_AMD_FWD_FLAT": 2})
    e = "env_old_grid"
    for rq, dims in (("short1", 128), ("ragged", 128), ("mixed_ragged", [16, 64, 128]), ("mixed_even", [16, 64, 128])):
        add(f"{e}_{rq}", e, "fwd", rq, dims=dims, env={"PARAM_AMD_FLAT_COMPACT": 0}, weighted=rq == "ragged")
    e, env = "env_flat_bags48", {"PARAM_AMD_FLAT_BAGS": 48, "PARAM_AMD_FLAT_TARGET": 64}
    for rq, dims in (("short1", 128), ("short2", 128), ("ragged", 128), ("short2", 32), ("mixed_ragged", [16, 64, 128])):
        add(f"{e}_{rq}_D{dims if isinstance(dims, int) else 'mixed'}", e, "fwd", rq, dims=dims, env=env, weighted=rq == "short2")
    e, env = "env_stage_off", {"PARAM_AMD_FWD_STAGE": 0}
    add(f"{e}_even", e, "fwd", "even", tuning=dict(bags_per_block=32), env=env)
    add(f"{e}_even_auto", e, "fwd", "even", env=env, weighted=True)
    add(f"{e}_short1", e, "fwd", "short1", env=env)
    add(f"{e}_padded", e, "padded", "pad100", tuning=dict(bags_per_block=32), env=env)
    add(f"{e}_max", e, "max", "pad100", tuning=dict(bags_per_block=32), env=env)
    add(f"{e}_f8", e, "f8", "pad100", "e4m3", 128, tuning=dict(bags_per_block=32), env=env)
    add(f"{e}_out16", e, "out16", "pad100", tuning=dict(bags_per_block=32), env=env, out16="bf16")
    assert len({c.name for c in out}) == len(out)
    for c in out:                                                  # a group shares its environment; its cases are one test
        assert c.env == next(d.env for d in out if d.group == c.group), c.name
    return out


CASES = _cases()
GROUPS = sorted({c.group for c in CASES})
ENV_GROUPS = sorted({c.group for c in CASES if c.env})
