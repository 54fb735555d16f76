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
list to conditions on those labels.

The scaled FP8 entries (``f8s``, ``f8s_gather``) add ``scale`` (``"table"`` / ``"row"``) to a case and plan on the FP8 plans; the pooled
one's plan is ``plan_f8`` followed by the launcher's LDS rule, which ``f8s_out_offset`` / ``f8s_lds_bytes`` / ``f8s_stage_out`` restate
here and ``pinned_plan`` applies to the dumped row -- group ``f8s_edge`` sits on both sides of the one corner where the row exponents'
bytes cost a tile its burst.  The mixed-format entries (``anyfmt``, ``anyfmt_gather``) add ``formats``, one stored format per table; they
take no padding row and read the padded requests' indices as plain indices, and ``anyfmt_label`` derives, per format, which tiles it
owns, which of them read their indices from the request and which reach the tail loop behind that format's rows in flight."""
import functools

import numpy as np

from tests import padding_rules as P

PLAN_FIELDS = ("tiles_per_table", "bags_per_block", "idx_cap", "xcd_affine", "nt_loads", "ordered", "stage_out", "stage_bags",
               "flat_bags", "flat_target", "flat_compact", "unroll")
GATHER_FIELDS = ("vec", "group_lanes", "tile", "col_passes", "unroll", "lds_borders", "xcd_contiguous", "grid")
# the `kind` codes of tests/launch_plan_dump.cpp (0 .. 4: pm_embbag_plan's PM_PLAN_*; 5: the gather plan)
# (6 .. 8: plan_f8 for 4- / 2-byte output elements and plan_gather_f8, the plans of pm_embbag_f8_plan / pm_embedding_gather_f8_plan)
# (9 .. 11: plan_anyfmt for 4- / 2-byte output elements and plan_gather_anyfmt, the plans of pm_embbag_anyfmt_plan / pm_embedding_gather_anyfmt_plan)
KIND = {"base": 0, "forward": 1, "quantized": 2, "padded4": 3, "padded2": 4, "gather": 5, "f8_4": 6, "f8_2": 7, "f8_gather": 8,
        "anyfmt_4": 9, "anyfmt_2": 10, "anyfmt_gather": 11}
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
              "f8": ("f8_4", "f8_2"), "f8_gather": "f8_gather",
              # the scaled FP8 lookups plan on the FP8 plans: the pooled one on plan_f8 followed by f8s_stage_out (``pinned_plan`` below)
              "f8s": ("f8_4", "f8_2"), "f8s_gather": "f8_gather", "anyfmt": ("anyfmt_4", "anyfmt_2"), "anyfmt_gather": "anyfmt_gather"}
GATHER_ENTRIES = ("gather", "f8_gather", "f8s_gather", "anyfmt_gather")
UNROLLS = (1, 2, 3, 4, 6, 8)
# FP8 pooled: (lane-group width, the D its unroll cases run at, the unroll its mean case runs at)
F8_GROUP_DIMS = ((8, 64, 4), (16, 192, 8), (32, 400, 2), (64, 1024, 4))
K_BLOCK = 256
ANY_VEC = 8                                                                   # columns per lane of both mixed-format kernels
# the mixed-format pooled kernel's compile-time rows in flight per format (embbag_fwd_anyfmt_kernel.inc: kUnroll -- the float formats'
# 2, kF8Unroll, kQrowsUnroll)
ANY_UNROLL = {"fp32": 2, "bf16": 2, "fp16": 2, "fp8_e4m3": 2, "fp8_e5m2": 2, "int8": 4, "int4": 4}


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
                          "padfix": (3, 100, [1000, 500, 250], dict(fixed=4)),
                          # 600 bags of 4.5 lookups on average: an explicit 512-bag tile gets the whole index tile (4096 entries)
                          "pad600": (2, 600, [1000, 300], dict(max_len=9))}[name]
        pads = [5, rows[1] - 1] + [None if t % 2 == 0 else 0 for t in range(2, T)]
        idx, off = P.padded_request(np.random.default_rng(500 + B + T), rows, B, pads, **kw)
        r = Request(name, T, B, rows, np.diff(off), 500 + B + T, pads=pads, idx=idx)
        share = P.padded_mask(idx, off, T, B, pads).mean()
        assert 0.2 < share < 0.45, share
        return r
    if name == "ragged8":
        # the gathers' eight tables: seven of them end inside the first 256-position tile (one tile holds seven formats, a wave several),
        # the eighth reaches into a second tile that is not full; empty bags, an empty first bag of table 3
        T, B = 8, 14
        lens = np.random.default_rng(802).integers(0, 6, T * B)
        lens[3 * B] = 0
        r = Request(name, T, B, [1000, 500, 250, 125, 1000, 500, 250, 125], lens, 810)
        assert r.off[7 * B] <= K_BLOCK < r.N < 2 * K_BLOCK and all(r.off[(t + 1) * B] > r.off[t * B] for t in range(T))
        return r
    if name == "many260":
        # more tables than the gathers stage borders for in LDS (T + 1 > 256): a few rows and two bags each
        T, B = 260, 2
        lens = np.random.default_rng(803).integers(0, 4, T * B)
        lens[0] = lens[7] = 0
        r = Request(name, T, B, [3 + t % 5 for t in range(T)], lens, 803)
        assert r.N > 2 * K_BLOCK and r.N % K_BLOCK
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
                 bag_slice=None, out16=None, mean=False, bits=None, scale=None, formats=None):
        self.name, self.group, self.entry, self.request, self.kind = name, group, entry, request, kind
        self.tuning, self.forward, self.env = dict(tuning or {}), dict(forward or {}), dict(env or {})
        self.weighted, self.bag_slice, self.out16, self.mean, self.bits = weighted, bag_slice, out16, mean, bits
        self.scale, self.formats = scale, None if formats is None else list(formats)
        self._dims = dims
        assert not set(self.tuning) - set(TUNING) and not set(self.forward) - set(FORWARD_TUNING) and not set(self.env) - set(ENV)
        assert entry in ENTRY_KIND and not (mean and weighted) and not (entry == "max" and (weighted or mean))
        # an FP8 entry has FP8 tables (dims: multiples of 16 in [16, 2048]) and nothing else has
        assert (kind in F8_DTYPE and all(d % 16 == 0 and 16 <= d <= 2048 for d in self.dims)) if entry.startswith("f8") else kind in DTYPE
        # a scaled FP8 entry says which exponents its tables carry, and nothing else does
        assert (scale in ("table", "row")) if entry.startswith("f8s") else scale is None
        # a mixed-format entry names one stored format per table (the request struct says fp32, which no kernel reads), dims in
        # multiples of 8 -- of 16 for an FP8 table -- up to 2048, no mean pooling; nothing else names formats
        if entry.startswith("anyfmt"):
            assert kind == "f32" and not mean and len(self.formats) == self.req.T and set(self.formats) <= set(ANY_UNROLL)
            assert all(d % (16 if f.startswith("fp8") else 8) == 0 and 8 <= d <= 2048 for f, d in zip(self.formats, self.dims))
        else:
            assert formats is None

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
        return bool(self.weighted and self.entry not in GATHER_ENTRIES + ("psw_grad", "mean_grad"))

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


def label(case, plan, dumped=None):
    """the variant a plan selects, as a set of words; what depends on the request's own offsets (``direct``: some tile's lookups
    exceed the index tile and are read from the request; ``partial``: the last tile of a table is not full) is derived from them.
    ``plan`` is the pinned row (``pinned_plan``), ``dumped`` what launch_plan_dump printed for the case where the two can differ"""
    r, (b0, n) = case.req, case.bags
    if case.entry.startswith("anyfmt"):
        return anyfmt_label(case, plan)
    G = group_lanes(max(case.dims), VEC[case.kind])
    if case.entry.startswith("f8s"):
        # f8_label's words, the kind of exponent, and whether the restated LDS rule took a burst that plan_f8 had granted
        words = f8_label(case, plan) | {case.scale}
        if case.entry == "f8s":
            assert dumped is not None and pinned_plan(case, dumped) == list(plan), "a scaled pooled case is labelled next to its dumped plan_f8 row"
            if dict(zip(PLAN_FIELDS, dumped))["stage_out"] > 0 and not dict(zip(PLAN_FIELDS, plan))["stage_out"]:
                words.add("burst-dropped")
        return words
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
    if case.entry in ("f8_gather", "f8s_gather"):
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


def anyfmt_label(case, plan):
    """the variant of a mixed-format case.  Family words ``any`` and ``pooled`` / ``unpooled``; the output type; per format and tile, from
    the request's offsets next to the plan (a tile's bags belong to one table, so to one format):
      ``fmt:<name>``     the format owns at least one tile (the gather: at least one written position);
      ``direct:<name>``  ... a tile whose lookups exceed the index tile: its indices are read from the request;
      ``tail:<name>``    ... a tile with a bag whose length is no multiple of that format's rows in flight (``ANY_UNROLL``): its tail loop runs.
    The gather: ``partial`` is a last tile of positions that is not full, ``tile-formats<k>`` the most formats one 256-position tile
    holds, ``wave-formats<k>`` the most formats the 64 positions of one wave hold."""
    r, (b0, n) = case.req, case.bags
    words = {"any", "out-" + (case.out16 or "fp32")} | ({"slice"} if case.bag_slice else set())
    if case.entry == "anyfmt_gather":
        p = dict(zip(GATHER_FIELDS, plan))
        assert p["vec"] == ANY_VEC
        words |= {"unpooled", f"G{p['group_lanes']}", f"u{p['unroll']}", f"passes{p['col_passes']}", f"xcd{p['xcd_contiguous']}",
                  "lds_borders" if p["lds_borders"] else "global_borders"} | ({"partial"} if r.N % p["tile"] else set())
        if max(case.dims) % (p["group_lanes"] * ANY_VEC):
            words.add("row-ends-in-pass")                          # the last pass has pieces at or behind the row's width
        owner = np.full(r.N, -1)
        for t in range(r.T):
            owner[r.off[t * r.B + b0]:r.off[t * r.B + b0 + n]] = t
        fmt_of = np.array([list(ANY_UNROLL).index(f) for f in case.formats] + [-1])[owner]          # -1: the position is not written
        words |= {f"fmt:{list(ANY_UNROLL)[k]}" for k in set(fmt_of.tolist()) - {-1}}
        per = lambda width: max(len(set(fmt_of[i:i + width].tolist()) - {-1}) for i in range(0, r.N, width))  # noqa: E731
        return words | {f"tile-formats{per(p['tile'])}", f"wave-formats{per(64)}"}
    p = dict(zip(PLAN_FIELDS, plan))
    G = group_lanes(max(case.dims), ANY_VEC)
    bpb, cap = p["bags_per_block"], p["idx_cap"]
    assert p["unroll"] == 0                                        # (the rows in flight are the formats' own)
    words |= {"pooled", f"G{G}", "weighted" if case.weighted else "unweighted", f"xcd{p['xcd_affine']}", f"bpb{bpb}",
              "staged" if p["stage_out"] else "plain", f"passes{-(-max(case.dims) // (G * ANY_VEC))}"}
    if max(case.dims) % (G * ANY_VEC):
        words.add("row-ends-in-pass")
    if bpb > K_BLOCK // G:
        words.add("tile>NG")
    for t, fmt in enumerate(case.formats):
        for k in range(-(-n // bpb)):
            g0, nb = t * r.B + b0 + k * bpb, min(bpb, n - k * bpb)
            words.add(f"fmt:{fmt}")
            if nb < bpb:
                words.add("partial")
            if r.off[g0 + nb] - r.off[g0] > cap:
                words.add(f"direct:{fmt}")
            if (r.lens[g0:g0 + nb] % ANY_UNROLL[fmt]).any():
                words.add(f"tail:{fmt}")
    return words


# ---- the scaled FP8 pooled launcher's LDS rule, restated (param_amd/csrc/common.h: f8s_out_offset / f8s_lds_bytes / f8s_stage_out) -----
def f8s_out_offset(bpb, idx_cap, weighted, row):
    """where the burst begins: int64 offsets[bpb + 1, rounded up to even] | int32 indices[idx_cap] | fp32 weights[idx_cap] (weighted) |
    uint16 compacted positions[idx_cap] | int8 row exponents[idx_cap] (``row``), rounded up to 16 bytes"""
    tile = (bpb + 2) // 2 * 2 * 8 + idx_cap * 4 * (2 if weighted else 1)
    return (tile + idx_cap * (3 if row else 2) + 15) // 16 * 16


def f8s_lds_bytes(bpb, idx_cap, weighted, row, stage_out, out_bytes):
    return f8s_out_offset(bpb, idx_cap, weighted, row) + (bpb * stage_out * out_bytes if stage_out > 0 else 0)


def f8s_stage_out(bpb, idx_cap, weighted, row, stage_out, out_bytes):
    """the burst leaves where it pushes the tile's LDS past 64 KiB"""
    return 0 if f8s_lds_bytes(bpb, idx_cap, weighted, row, stage_out, out_bytes) > 65536 else stage_out


def f8s_case_lds(case, dumped):
    """(bytes with the burst plan_f8 granted, bytes the launcher asks for) of a scaled pooled case"""
    p = dict(zip(PLAN_FIELDS, dumped))
    a = (p["bags_per_block"], p["idx_cap"], case.plan_weighted and not case.mean, case.scale == "row")
    ob = 2 if case.out16 else 4
    return f8s_lds_bytes(*a, p["stage_out"], ob), f8s_lds_bytes(*a, f8s_stage_out(*a, p["stage_out"], ob), ob)


def pinned_plan(case, dumped):
    """the row tests/plan_sweep_host.json pins for a case: what launch_plan_dump printed, but for the scaled FP8 pooled lookup, whose
    plan is plan_f8's with ``stage_out`` as f8s_stage_out leaves it -- what ``pm_embbag_f8_scaled_plan`` must report"""
    if case.entry != "f8s":
        return list(dumped)
    p = dict(zip(PLAN_FIELDS, dumped))
    p["stage_out"] = f8s_stage_out(p["bags_per_block"], p["idx_cap"], case.plan_weighted and not case.mean, case.scale == "row", p["stage_out"],
                                   2 if case.out16 else 4)
    return [p[f] for f in PLAN_FIELDS]


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
    # -- scaled FP8 tables, pooled: pm_embbag_fwd_f8_scaled on plan_f8 followed by f8s_stage_out; the FP8 cases' shapes with row exponents
    #    (one byte per index-tile entry in LDS, behind the compacted positions and in front of the burst) or a table exponent
    def f8s(name, group, rq, dims, scale, mode="plain", fmt="e4m3", **kw):
        add(name, group, "f8s", rq, fmt, dims, weighted=mode == "weighted", mean=mode == "mean", scale=scale, **kw)

    scales = ("row", "table")
    # the multi-tile baseline (see f8_base_*): both formats x both kinds of exponent x the three modes, fp32 rows one by one and bf16 burst
    for fmt in F8_DTYPE:
        for sc in scales:
            for mode in modes:
                f8s(f"f8s_base_{fmt}_{sc}_{mode}", f"f8s_base_{fmt}_{sc}", "pad100", 256, sc, mode, fmt, tuning=dict(bags_per_block=32))
                f8s(f"f8s_base_{fmt}_{sc}_{mode}_bf16", f"f8s_base_{fmt}_{sc}", "pad100", 256, sc, mode, fmt, tuning=dict(bags_per_block=32), out16="bf16")
    f8s("f8s_base_e4m3_row_weighted_bf16_unstaged", "f8s_base_e4m3_row", "pad100", 256, "row", "weighted", tuning=dict(bags_per_block=32),
        forward=dict(stage_out=0), out16="bf16")
    # fp32 rows through the burst, which lies behind the exponent bytes: 64-bag tiles of D = 64 rows, 18 tiles a table
    for sc, ms in (("row", modes), ("table", modes[:1])):
        for mode in ms:
            f8s(f"f8s_burst_{sc}_{mode}", "f8s_burst", "pad1100", 64, sc, mode, tuning=dict(bags_per_block=64))
            f8s(f"f8s_burst_{sc}_{mode}_unstaged", "f8s_burst", "pad1100", 64, sc, mode, tuning=dict(bags_per_block=64), forward=dict(stage_out=0))
    # every lane-group width x every depth with row exponents, two bags per lane group; mean and a table exponent at one depth per width
    for G, D, mean_u in F8_GROUP_DIMS:
        for u in (2, 4, 8):
            for mode in modes[:2] + (("mean",) if u == mean_u else ()):
                f8s(f"f8s_G{G}_u{u}_{mode}", f"f8s_G{G}", "pad100", D, "row", mode, tuning=dict(unroll=u, bags_per_block=2 * K_BLOCK // G))
        f8s(f"f8s_G{G}_u{mean_u}_table", f"f8s_G{G}", "pad100", D, "table", "weighted", tuning=dict(unroll=mean_u, bags_per_block=2 * K_BLOCK // G))
    # block orders (block_to_tile picks the table's exponent pointer) and a slice that begins and ends inside tiles
    f8s("f8s_xcd0", "f8s_orders", "pad100", 128, "row", tuning=dict(bags_per_block=32, xcd_affine=0))
    f8s("f8s_xcd1", "f8s_orders", "pad8", 128, "row", tuning=dict(bags_per_block=32))
    f8s("f8s_xcd3", "f8s_orders", "padfix", 128, "row", tuning=dict(bags_per_block=32))
    f8s("f8s_slice", "f8s_orders", "pad100", 128, "row", tuning=dict(bags_per_block=32), bag_slice=(5, 70))
    f8s("f8s_slice_mean", "f8s_orders", "pad100", 128, "row", "mean", tuning=dict(bags_per_block=32), bag_slice=(5, 70))
    # 1024-bag tiles: ten rounds of compaction with the exponent bytes travelling next to the indices, a thread's fifth bound
    for mode in modes:
        f8s(f"f8s_bpb1024_{mode}", "f8s_1024", "pad1100", 16, "row", mode, tuning=dict(bags_per_block=1024))
        f8s(f"f8s_bpb1024_{mode}_bf16", "f8s_1024", "pad1100", 16, "row", mode, tuning=dict(bags_per_block=1024), out16="bf16")
    # the direct tile loads a row's exponent next to the index it reads from the request
    for mode in modes:
        for u in (2, 8):
            f8s(f"f8s_direct_u{u}_{mode}", "f8s_direct", "pad_lumpy", 128, "row", mode, tuning=dict(unroll=u, bags_per_block=32))
    # the LDS edge: 512-bag tiles of D = 16 bf16 rows fill the 16 KiB burst; with 4096 index-tile entries, weights and row exponents the
    # tile is 49168 + 16384 = 65552 bytes, sixteen over, and the burst leaves; with a table exponent (61456) or without weights it stays
    f8s("f8s_edge_row_weighted", "f8s_edge", "pad600", 16, "row", "weighted", tuning=dict(bags_per_block=512), out16="bf16")
    f8s("f8s_edge_table_weighted", "f8s_edge", "pad600", 16, "table", "weighted", tuning=dict(bags_per_block=512), out16="bf16")
    f8s("f8s_edge_row_plain", "f8s_edge", "pad600", 16, "row", tuning=dict(bags_per_block=512), out16="bf16")
    f8s("f8s_mixed_dims", "f8s_wide", "pad100", [16, 64, 128], "row", "weighted", tuning=dict(bags_per_block=32))
    f8s("f8s_D512_bf16", "f8s_wide", "pad100", 512, "row", tuning=dict(bags_per_block=16), out16="bf16")
    f8s("f8s_D512_fp32", "f8s_wide", "pad100", 512, "row", tuning=dict(bags_per_block=16))
    f8s("f8s_D1040_two_passes", "f8s_wide", "pad100", 1040, "row", "weighted", tuning=dict(bags_per_block=8))
    # -- scaled FP8 tables, un-pooled: pm_embedding_gather_f8_scaled on plan_gather_f8; three tables, each with exponents of its own
    def f8sg(name, group, scale="row", rq="ragged", dims=128, fmt="e4m3", **kw):
        add(name, group, "f8s_gather", rq, fmt, dims, scale=scale, **kw)

    for (G, D), table_u in zip(((8, 16), (16, 64), (32, 128), (64, 256)), (2, 8, 1, 4)):
        for u in (1, 2, 4, 8):
            f8sg(f"f8s_gather_G{G}_u{u}", "f8s_gather_GU", dims=D, tuning=dict(unroll=u))
        f8sg(f"f8s_gather_G{G}_u{table_u}_table", "f8s_gather_GU", "table", dims=D, tuning=dict(unroll=table_u))
    f8sg("f8s_gather_bf16", "f8s_gather_knobs", tuning=dict(unroll=8), out16="bf16")
    f8sg("f8s_gather_fp16", "f8s_gather_knobs", tuning=dict(unroll=2), out16="fp16")
    f8sg("f8s_gather_xcd0", "f8s_gather_knobs", tuning=dict(unroll=2, xcd_affine=0))
    f8sg("f8s_gather_D512_two_passes", "f8s_gather_knobs", rq="mixed_ragged", dims=512, tuning=dict(unroll=4))
    f8sg("f8s_gather_slice", "f8s_gather_knobs", tuning=dict(unroll=4), bag_slice=(3, 90))
    f8sg("f8s_gather_e5m2", "f8s_gather_knobs", fmt="e5m2", tuning=dict(unroll=8))
    # -- mixed-format tables, pooled: pm_embbag_fwd_anyfmt on plan_anyfmt, eight columns per lane whatever the format (G = 8 up to D = 64,
    #    64 from D = 264 on); a tile's table decides which of the seven row loops the workgroup runs, each with its own rows in flight
    def anyf(name, group, rq, dims, formats, **kw):
        add(name, group, "anyfmt", rq, "f32", dims, formats=formats, **kw)

    seven = list(ANY_UNROLL)
    rot = [[seven[(3 * k + t) % 7] for t in range(3)] for k in range(3)]    # three tables, three rotations: every format, neighbours differ
    eight = seven + ["int8"]
    # every format x every lane-group width x weighted, two bags per lane group (the fp32 burst filled exactly), several tiles a table
    for G in (8, 16, 32, 64):
        for k in range(3):
            for w in (False, True):
                anyf(f"any_G{G}_rot{k}_{wname[w]}", f"any_G{G}", "pad100", G * ANY_VEC, rot[k], tuning=dict(bags_per_block=2 * K_BLOCK // G), weighted=w)
    # four bags per lane group: the 2-byte burst fits, the 4-byte one does not; all seven formats
    anyf("any_out_bf16", "any_out16", "pad8", 256, eight, tuning=dict(bags_per_block=32), out16="bf16")
    anyf("any_out_fp16_weighted", "any_out16", "pad8", 256, eight, tuning=dict(bags_per_block=32), out16="fp16", weighted=True)
    anyf("any_out_fp32", "any_out16", "pad8", 256, eight, tuning=dict(bags_per_block=32))
    # the fp32 burst over 18 tiles a table, and the same rows one by one
    for w in (False, True):
        anyf(f"any_burst_{wname[w]}", "any_burst", "pad1100", 64, ["fp8_e4m3", "int4"], tuning=dict(bags_per_block=64), weighted=w)
        anyf(f"any_burst_{wname[w]}_unstaged", "any_burst", "pad1100", 64, ["fp8_e4m3", "int4"], tuning=dict(bags_per_block=64), forward=dict(stage_out=0),
             weighted=w)
    # block orders (block_to_tile picks the table, hence the format; the plain order on three tables: any_G16_*) and slices that begin
    # and end inside tiles
    anyf("any_xcd0_seven", "any_orders", "pad8", 128, eight, tuning=dict(bags_per_block=32, xcd_affine=0), weighted=True)
    anyf("any_xcd1_seven", "any_orders", "pad8", 128, eight, tuning=dict(bags_per_block=32))
    anyf("any_xcd3", "any_orders", "padfix", 128, rot[2], tuning=dict(bags_per_block=32))
    anyf("any_slice", "any_orders", "pad100", 128, rot[1], tuning=dict(bags_per_block=32), bag_slice=(5, 70))
    anyf("any_slice_weighted", "any_orders", "pad100", 128, rot[2], tuning=dict(bags_per_block=32), bag_slice=(5, 70), weighted=True)
    # 1024-bag tiles
    anyf("any_bpb1024_plain", "any_1024", "pad1100", 16, ["fp8_e5m2", "int4"], tuning=dict(bags_per_block=1024))
    anyf("any_bpb1024_weighted", "any_1024", "pad1100", 16, ["bf16", "int8"], tuning=dict(bags_per_block=1024), weighted=True)
    # the 32-bag tile of 1600 lookups (table 0's) reads its indices from the request: owned by an FP8, a 4-bit and an fp32 table
    for first, rest in (("fp8_e4m3", ["bf16", "int8"]), ("int4", ["fp16", "fp8_e5m2"]), ("fp32", ["int8", "bf16"])):
        for w in (False, True):
            anyf(f"any_direct_{first}_{wname[w]}", "any_direct", "pad_lumpy", 256, [first] + rest, tuning=dict(bags_per_block=32), weighted=w)
    # a second pass that ends inside the lane group (D = 520: one lane of 64 holds columns; no FP8 table has that width), four
    # passes, mixed dims with the lane group sized for 128
    anyf("any_D520_weighted", "any_wide", "pad100", 520, ["int4", "fp32", "int8"], tuning=dict(bags_per_block=8), weighted=True)
    anyf("any_D520", "any_wide", "pad100", 520, ["bf16", "int4", "fp16"], tuning=dict(bags_per_block=8))
    anyf("any_D2048_four_passes", "any_wide", "pad100", 2048, ["fp8_e4m3", "int4", "fp16"], tuning=dict(bags_per_block=8))
    anyf("any_D2048_four_passes_weighted", "any_wide", "pad100", 2048, ["int8", "fp8_e5m2", "fp32"], tuning=dict(bags_per_block=8), weighted=True)
    anyf("any_mixed_dims", "any_wide", "pad100", [16, 64, 128], ["fp8_e5m2", "int8", "fp32"], tuning=dict(bags_per_block=32), weighted=True)
    # -- mixed-format tables, un-pooled: pm_embedding_gather_anyfmt on plan_gather_anyfmt; a lane group branches on its row's format
    def anyg(name, group, rq="ragged8", dims=128, formats=None, **kw):
        add(name, group, "anyfmt_gather", rq, "f32", dims, formats=formats or seven + ["fp16"], **kw)

    plain5 = ["fp32", "int8", "bf16", "int4", "fp16", "int8", "fp32", "int4"]          # (D = 520 is no FP8 width)
    for G in (8, 16, 32, 64):
        for o16 in (None, "bf16", "fp16"):
            anyg(f"any_gather_G{G}_{o16 or 'fp32'}", "any_gather_G", dims=G * ANY_VEC, out16=o16)
    anyg("any_gather_xcd0", "any_gather_knobs", tuning=dict(xcd_affine=0))
    anyg("any_gather_slice", "any_gather_knobs", bag_slice=(3, 8), out16="fp16")
    anyg("any_gather_D520", "any_gather_knobs", dims=520, formats=plain5, out16="bf16")
    anyg("any_gather_D2048_four_passes", "any_gather_knobs", dims=2048)
    anyg("any_gather_260_tables", "any_gather_knobs", rq="many260", dims=64, formats=[seven[t % 7] for t in range(260)])
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
    add(f"{e}_f8s", e, "f8s", "pad100", "e4m3", 128, tuning=dict(bags_per_block=32), env=env, scale="row")
    add(f"{e}_anyfmt", e, "anyfmt", "pad100", "f32", 128, tuning=dict(bags_per_block=32), env=env, formats=rot[1])
    add(f"{e}_out16", e, "out16", "pad100", tuning=dict(bags_per_block=32), env=env, out16="bf16")
    assert len({c.name for c in out}) == len(out)
    for c in out:                                                  # a group shares its environment; its cases are one test
        assert c.env == next(d.env for d in out if d.group == c.group), c.name
    return out


CASES = _cases()
GROUPS = sorted({c.group for c in CASES})
ENV_GROUPS = sorted({c.group for c in CASES if c.env})
