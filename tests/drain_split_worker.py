"""Runs the forward's staged 32-bag kernel under ONE setting of the split-last-round switches (PARAM_AMD_FWD_DRAIN_SPLIT,
PARAM_AMD_FWD_ROUND_WGS: read once per process, so tests/test_gpu_drain_split.py starts one ``python -m tests.drain_split_worker`` per
setting) and prints one JSON document: the comparisons with the C oracle that failed, and a SHA-256 of every output's bytes, which the
test compares between the settings.

Requests: 16 tables of 1000 x 128, pooling 20, Zipf 1.05, explicit 32-bag tiles; with 4 resident workgroups per XCD forced
  B = 11 * 32 - 5   an XCD has 22 tiles: its last round is 22 mod 4 = 2 tiles, split -- tiles 9 and 10 of table 8 + x, the last of which
                    has 27 bags, so its four parts get 8, 8, 8 and 3;  the slice [3, 3 + 10 * 32 + 5) ends in a tile of 5 bags: parts of
                    5, 0, 0, 0
  B = 4 * 32        two whole rounds, nothing left over: the launcher keeps the plain path
  B = 2 * 32        one round: the plain path
each with fp32 and bf16 tables, with and without per_sample_weights, in both output layouts."""
import hashlib
import json
import sys

import numpy as np

DEV = "cuda:0"
T, ROWS, D, L, TILE = 16, 1000, 128, 20, 32
BATCHES = (11 * TILE - 5, 4 * TILE, 2 * TILE)
SLICE = (3, 10 * TILE + 5)          # of the first batch size


def main():
    import torch

    import param_amd
    from oracle.embbag_oracle import COracle
    from param_amd.indices import tbe_request

    assert torch.cuda.is_available(), "needs a ROCm device"
    param_amd.load_library()
    orc = COracle()
    rows = [ROWS] * T
    failures, digests = [], {}
    param_amd.set_tuning(bags_per_block=TILE)
    try:
        for dt_name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            for layout in ("bd", "tbd"):
                m = param_amd.BatchedEmbeddingBagMI355(rows, D, dtype=dt, device=DEV, layout=layout, init="normal", seed=7, fused_update=False)
                tabs = [m.table(t).float().cpu().numpy().copy() for t in range(T)]
                shape = lambda B: (B, T * D) if layout == "bd" else (T, B, D)                 # noqa: E731
                for B in BATCHES:
                    idx, off = tbe_request(rows, B, L, alpha=1.05, device=DEV, seed=B)
                    idx_h, off_h = idx.cpu().numpy(), off.cpu().numpy()
                    psw = torch.from_numpy(np.random.default_rng(B).standard_normal(idx_h.size).astype(np.float32)).to(DEV)
                    for weighted in (False, True):
                        w_t, w_h = (psw, psw.cpu().numpy()) if weighted else (None, None)
                        want = orc.fwd_batched(tabs, idx_h, off_h, B, psw=w_h, layout=layout)
                        for b0, n in ((0, B),) + ((SLICE,) if B == BATCHES[0] else ()):
                            name = f"{dt_name} {layout} B={B} weighted={int(weighted)} bags=[{b0},{b0 + n})"
                            canvas = torch.full(shape(B), float("nan"), dtype=torch.float32, device=DEV)
                            m.lookup(idx, off, w_t, out=canvas, batch=B, bag_begin=b0, bag_count=n)
                            got = canvas.cpu().numpy()
                            digests[name] = hashlib.sha256(got.tobytes()).hexdigest()
                            sel = (slice(b0, b0 + n),) if layout == "bd" else (slice(None), slice(b0, b0 + n))
                            rest = np.ones(got.shape, dtype=bool)
                            rest[sel] = False
                            if not np.array_equal(got[sel].view(np.uint32), want[sel].view(np.uint32)):
                                failures.append(name + ": differs from the oracle in %d elements" % int((got[sel] != want[sel]).sum()))
                            elif not np.isnan(got[rest]).all():
                                failures.append(name + ": written outside the slice")
    finally:
        param_amd.set_tuning()
    print(json.dumps({"failures": failures, "digests": digests}))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
