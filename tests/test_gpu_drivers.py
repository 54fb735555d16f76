"""GPU tests of the driver / plug-in layers on ONE MI355X (world size 1): the compute/pt driver rows,
the compute/python operator, the comms backend's embedding functions and the DLRM driver end to end."""
import contextlib
import io
import json
import os
import socket
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _port():
    """A TCP port for a rendezvous: below the kernel's ephemeral range (32768+), so it cannot collide with the local port
    of some earlier store client's connection still in TIME_WAIT (seen as EADDRINUSE once in a long GPU suite run), never
    handed out twice by this process, and bindable right now."""
    import itertools
    import os as _os

    global _PORTS
    try:
        _PORTS
    except NameError:
        _PORTS = itertools.count(12000 + (_os.getpid() * 37) % 18000)
    for p in _PORTS:
        p = 12000 + (p - 12000) % 20000
        s = socket.socket()
        try:
            s.bind(("127.0.0.1", p))
        except OSError:
            continue
        finally:
            s.close()
        return p


def test_compute_pt_driver_gpu_rows():
    from param_amd.compute.pt import pytorch_emb

    args = types.SimpleNamespace(device="gpu", randomseed=0, warmups=2, steps=5, alpha=0.0, usexlabag=False,
                                 dtype="float32", tables=1, json=True)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        pytorch_emb.run(args, [(1000000, 32, 20, 512), (200000, 128, 30, 2048)])
        args.tables, args.alpha, args.dtype = 8, 1.05, "bfloat16"
        pytorch_emb.run(args, [(100000, 128, 20, 1024)])
    lines = buf.getvalue().splitlines()
    assert lines[1] == pytorch_emb.HEADER
    rows = [json.loads(ln) for ln in lines if ln.startswith("{")]
    assert len(rows) == 3 and all(r["lookups_per_s"] > 1e8 for r in rows)
    assert rows[0]["param_GBps"] == pytest.approx(512 * 20 * 32 * 4 / rows[0]["s_per_step"] / 1e9)
    assert rows[2]["tables"] == 8 and rows[2]["dtype"] == "bfloat16"


def test_compute_python_operator_forward_backward(coracle):
    from param_amd.compute.python import op_map
    from param_amd.compute.python.split_table_batched_embeddings_ops import generate_batched_request

    op = op_map["SplitTableBatchedEmbeddingBagsCodegen"]
    op.device = "cuda"
    op.cleanup()
    op.build(3, [300, 500, 700], 64, 0, True, "fp32", "sgd", lr=0.1)
    torch.manual_seed(1)
    idx, off, w = generate_batched_request(3, [300, 500, 700], 16, [4, 6, 2], alpha=1.0, weighted=True, device=DEV)
    out = op.forward(idx, off, w)
    tabs = [op.op.table(t).cpu().numpy().copy() for t in range(3)]
    ref = coracle.fwd_batched(tabs, idx.cpu().numpy(), off.cpu().numpy(), 16, psw=w.cpu().numpy())
    assert np.array_equal(out.cpu().numpy(), ref)
    op.create_grad()
    op.backward()
    B = 16
    idx_h, off_h, w_h = idx.cpu().numpy(), off.cpu().numpy(), w.cpu().numpy()
    for t in range(3):
        s, e = off_h[t * B], off_h[(t + 1) * B]
        exp = coracle.bwd_f32(tabs[t].copy(), idx_h[s:e], off_h[t * B:(t + 1) * B] - s, np.ones((B, 64), np.float32),
                              w_h[s:e], alpha=-0.1)
        assert np.array_equal(op.op.table(t).cpu().numpy(), exp), t
    op.cleanup()


def test_backend_embedding_functions_single_rank(coracle):
    """MI355XBackend.alloc_embedding_tables / emb_lookup / lookup_all_to_all on a 1-rank RCCL group."""
    import torch.distributed as dist

    from param_amd.comms.pt import comms_utils
    from param_amd.comms.pt.mi355_backend import MI355XBackend, register
    from param_amd.comms.pt.pytorch_backend_utils import collectiveArgsHolder, customized_backend

    register()
    assert customized_backend["rccl_xgmi"] is MI355XBackend
    env = {"world_size": 1, "local_size": 1, "global_rank": 0, "local_rank": 0}
    port = _port()
    bf = MI355XBackend(comms_utils.bootstrap_info_holder("127.0.0.1", str(port), 0, env), {"device": "cuda", "backend": "nccl"})
    bf.initialize_backend("127.0.0.1", str(port), backend="rccl_xgmi")
    try:
        E = bf.alloc_embedding_tables(1000, 32, DEV, torch.float32)
        lim = np.sqrt(1 / 1000)
        assert float(E.weight.data.abs().max()) <= lim and float(E.weight.data.std()) > lim / 3
        idx = torch.randint(0, 1000, (200,), device=DEV)
        off = torch.arange(20, device=DEV) * 10
        with torch.no_grad():
            o = E(idx, off)
        assert np.array_equal(o.cpu().numpy(), coracle.fwd(E.weight.data.cpu().numpy(), idx.cpu().numpy(), off.cpu().numpy()))
        ca = collectiveArgsHolder()
        ca.world_size, ca.global_rank, ca.group, ca.device = 1, 0, bf.get_default_group(), bf.get_device()
        ca.emb = [bf.alloc_batched_embedding_tables([500, 600], 64, DEV, torch.float32) for _ in range(2)]
        from param_amd.indices import tbe_request
        ca.embRequests = [tbe_request([500, 600], 8, 5, device=DEV, seed=s) + (None,) for s in (1, 2)]
        ca.num_emb_ops, ca.num_emb_tables_batched, ca.asyncOp, ca.direction = 2, 2, False, "forward"
        bf.emb_lookup(ca)
        assert ca.LookupOut.shape == (8, 128)
        # the fused lookup -> all_to_all entry is an explicit opt-in (the reference needs extend_distributed for it):
        # without it a batched-table holder changes nothing about a plain all_to_all call
        ca.ipTensor, ca.opTensor = torch.arange(4.0, device=DEV), torch.empty(4, device=DEV)
        bf.all_to_all(ca)
        assert torch.equal(ca.opTensor, ca.ipTensor) and getattr(ca, "a2a_recv", None) is None
        bf.fused_lookup_a2a = True
        bf.all_to_all(ca)                     # fused lookup -> all_to_all per op (1 rank: identity exchange)
        bf.complete_accel_ops(ca)
        for i in range(2):
            assert torch.equal(ca.a2a_recv[i], ca.emb[i].lookup(*ca.embRequests[i][:2]))
        ca.asyncOp = True                     # non-blocking: the individual handles join waitObj, wait() takes them one by one
        assert bf.all_to_all(ca) is None and len(ca.waitObj) == 2 and all(hasattr(w, "wait") for w in ca.waitObj)
        bf.wait(ca)
        assert len(ca.waitObj) == 1
        bf.complete_accel_ops(ca)
        assert ca.waitObj == []
        ca.collective = "all_to_all"          # pooled into the collective: emb_lookup itself is skipped (reference :835-839)
        ca.LookupOut = None
        bf.emb_lookup(ca)
        assert ca.LookupOut is None
        ca.collective, ca.asyncOp = "", False
        bf.fused_lookup_a2a = False
        before = ca.emb[0].table(0).clone()
        ca.direction, ca.grad_output = "backward", torch.ones(8, 128, device=DEV)
        bf.emb_lookup(ca)
        assert not torch.equal(before, ca.emb[0].table(0))
        t = torch.ones(16, device=DEV)
        ca.ipTensor, ca.asyncOp = t, True
        bf.all_reduce(ca)
        bf.sync_barrier(ca)
        assert ca.waitObj == [] and float(t.sum()) == 16.0
    finally:
        bf.shutdown()


def test_dlrm_driver_single_gpu(tmp_path):
    from param_amd.comms.pt import dlrm

    cwd = os.getcwd()
    os.chdir(tmp_path)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_SIZE"):
        os.environ.pop(k, None)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            rep = dlrm.main(["--master-ip", "127.0.0.1", "--master-port", str(_port()), "--device", "rocm",
                             "--mini-batch-size", "256", "--num-batches", "6", "--warmup-batches", "2",
                             "--arch-mlp-bot", "64-32", "--arch-mlp-top", "32-1", "--arch-sparse-feature-size", "128",
                             "--arch-embedding-size", "20000-30000-40000-50000", "--num-indices-per-lookup", "20",
                             "--num-indices-per-lookup-fixed", "--print-comms"])
    finally:
        os.chdir(cwd)
    assert rep["iter_time"]["p50"] > 0 and rep["fwd_a2a_bw"]["bytes_per_rank"] == 256 * 4 * 128 * 4
    rec = json.load(open(tmp_path / "dlrm_np1" / "rank0.json"))
    assert [r["comms"] for r in rec][:3] == ["all_to_all"] * 3 and rec[2]["msg_size"] == 256 * 4 * 128 * 4


def test_dlrm_sparse_path_hip_vs_oracle(coracle):
    """DLRMSparsePath with the HIP lookup/update at world size 1: pooled == oracle, update == oracle."""
    import torch.distributed as dist

    from param_amd import BatchedEmbeddingBagMI355
    from param_amd.comms.pt import comms_utils, dlrm as D_
    from param_amd.comms.pt.mi355_backend import MI355XBackend
    from param_amd.comms.pt.pytorch_backend_utils import collectiveArgsHolder

    env = {"world_size": 1, "local_size": 1, "global_rank": 0, "local_rank": 0}
    port = _port()
    bf = MI355XBackend(comms_utils.bootstrap_info_holder("127.0.0.1", str(port), 0, env), {"device": "cuda", "backend": "nccl"})
    bf.initialize_backend("127.0.0.1", str(port), backend="nccl")
    try:
        rows, D, B, L = [3000, 5000, 800], 64, 128, 12
        emb = BatchedEmbeddingBagMI355(rows, D, device=DEV, init="uniform_dlrm", seed=3)
        tabs = [emb.table(t).cpu().numpy().copy() for t in range(3)]
        ca = collectiveArgsHolder()
        ca.world_size, ca.global_rank, ca.group, ca.device = 1, 0, bf.get_default_group(), bf.get_device()
        path = D_.DLRMSparsePath(bf, ca, [3], D, B, lambda i, o, out: emb.lookup(i, o, out=out, batch=B),
                                 lambda g, i, o: emb.scatter_add_(g, i, o, alpha=-0.05, batch=B))
        gen = torch.Generator(device=DEV).manual_seed(9)
        lengths, indices = D_.generate_sparse_batch(rows, B, L, False, torch.device(DEV), gen)
        idx_tbe, off_tbe = path.sparse_data_dist(lengths, indices)
        assert torch.equal(idx_tbe, indices)                       # one rank: regrouping is the identity
        pooled, osp, isp = path.alltoallv_fwd(path.apply_emb(idx_tbe, off_tbe))
        ref = coracle.fwd_batched(tabs, idx_tbe.cpu().numpy(), off_tbe.cpu().numpy(), B)
        assert np.array_equal(pooled.cpu().numpy(), ref)
        g = path.alltoallv_bwd(pooled, osp, isp)
        path.update(g, idx_tbe, off_tbe)
        ih, oh = idx_tbe.cpu().numpy(), off_tbe.cpu().numpy()
        for t in range(3):
            s, e = oh[t * B], oh[(t + 1) * B]
            exp = coracle.bwd_f32(tabs[t].copy(), ih[s:e], oh[t * B:(t + 1) * B] - s,
                                  np.ascontiguousarray(ref[:, t * D:(t + 1) * D]), alpha=-0.05)
            assert np.array_equal(emb.table(t).cpu().numpy(), exp), t
    finally:
        bf.shutdown()


def test_comms_compute_overlap_bench_single_gpu():
    """comm (all_to_allv on the PG stream) || emb_lookup on the compute stream, per-stream device timers"""
    from param_amd.comms.pt import commsComputeBench

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_SIZE"):
        os.environ.pop(k, None)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = commsComputeBench.main(["--master-ip", "127.0.0.1", "--master-port", str(_port()), "--b", "1M", "--e", "4M",
                                      "--f", "4", "--n", "4", "--w", "2", "--collective", "all_to_allv", "--device", "rocm",
                                      "--kernel", "emb_lookup", "--num-compute", "3", "--ntables", "8", "--num-embs", "200000",
                                      "--emb-dim", "128", "--batch-size", "2048", "--bag-size", "20"])
    assert [r["size"] for r in res] == [1 << 20, 4 << 20]
    for r in res:
        assert r["compute_dev_us"] > 0 and r["comm_dev_us"] >= 0 and r["lookups_per_iter"] == 8 * 2048 * 20 * 3
        assert r["lookups_per_s_compute_stream"] > 1e9
    assert "COMMS-COMPUTE-RES-all_to_allv-emb_lookup" in buf.getvalue()
    res = commsComputeBench.main(["--master-ip", "127.0.0.1", "--master-port", str(_port()), "--b", "1M", "--e", "1M",
                                  "--n", "2", "--w", "1", "--collective", "all_to_allv", "--device", "rocm", "--mode", "compute",
                                  "--direction", "backward", "--num-compute", "2", "--ntables", "4", "--num-emb-tables-batched", "2",
                                  "--num-embs", "50000", "--batch-size", "512"])
    assert res[0]["memSize"] == 0 and res[0]["compute_dev_us"] > 0
    # --bitwidth: the collective of the overlap bench exchanges quantised rows, the record carries the (de-)quantise times
    res = commsComputeBench.main(["--master-ip", "127.0.0.1", "--master-port", str(_port()), "--b", "4M", "--e", "4M",
                                  "--n", "3", "--w", "1", "--collective", "all_to_allv", "--device", "rocm", "--kernel", "emb_lookup",
                                  "--ntables", "4", "--num-embs", "50000", "--batch-size", "512", "--bitwidth", "8",
                                  "--quant-a2a-embedding-dim", "128", "--z", "1"])
    assert res[0]["bitwidth"] == 8 and res[0]["quant_us"] > 0 and res[0]["dequant_us"] > 0 and res[0]["compute_dev_us"] > 0


def test_trace_replay_single_gpu(tmp_path):
    """examples/trace_replay/0.json (one DLRM iteration: a2a's, all_reduce, emb_lookup forward and backward as compute
    entries) replayed on one GPU through RCCL + the HIP kernels: blocking (kernel time) and non-blocking (wait by request id)"""
    from param_amd.comms.pt import commsTraceReplay

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_SIZE"):
        os.environ.pop(k, None)
    tdir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "trace_replay")
    for blocking in ("1", "0"):
        out = tmp_path / f"z{blocking}"
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            b = commsTraceReplay.main(["--trace-path", tdir, "--device", "rocm", "--master-ip", "127.0.0.1",
                                       "--master-port", str(_port()), "--num-replays", "3", "--do-warm-up", "--reuse-tensors",
                                       "--z", blocking, "--output-path", str(out)])
        assert len(b.compLat["emb_lookup"]) == 6 and min(b.compLat["emb_lookup"]) > 0
        assert len(b.collLat["all_to_allv"]) == 9 and len(b.collLat["all_reduce"]) == 3
        assert len(b.embLookupReuse) == 2                       # forward and backward entry shapes cached once
        rec = json.load(open(out / "replayedCommsPerf.rank0.json"))
        fwd = [r for r in rec if r.get("compute") == "emb_lookup" and r["direction"] == "forward"]
        assert len(fwd) == 3 and fwd[0]["num_emb_tables"] == 8 and fwd[0]["latency_us"] > 0
        assert "Replayed 6 emb_lookup (compute)" in buf.getvalue()
        if blocking == "1":   # blocking replay times the kernels: 8 x 2048 x 20 lookups well under a millisecond each
            assert np.median([r["latency_us"] for r in fwd]) < 5000


def test_dlrm_regroup_hip_kernel(golden_dir):
    """pm_dlrm_regroup (2 launches, no host sync) == the host regrouping == the reference's splitPerTable golden"""
    from param_amd.comms.pt import dlrm as D_

    s = json.load(open(os.path.join(golden_dir, "comms_pure.json")))["splitPerTable"]
    lengths, indices = torch.tensor(s["lengths"], device=DEV), torch.tensor(s["indices"], device=DEV)
    o, i = D_.splitPerTable(lengths, indices, s["batch"], s["features"], s["world"])
    assert [x.tolist() for x in o] == s["offsets_out"] and [x.tolist() for x in i] == s["indices_out"]
    g = torch.Generator().manual_seed(3)
    for W, F, B, Lmax in [(8, 4, 8192, 40), (2, 3, 5, 4), (8, 26, 64, 3), (1, 1, 1, 1), (4, 2, 1000, 0)]:
        lengths = torch.randint(0, Lmax + 1, (W * F * B,), generator=g)
        indices = torch.randint(0, 1 << 40, (int(lengths.sum()),), generator=g)
        ci, co = D_.regroup_per_table(lengths, indices, B, F, W)                      # host form (torch ops)
        gi, go = D_.regroup_per_table(lengths.to(DEV), indices.to(DEV), B, F, W)     # HIP kernels
        assert torch.equal(gi.cpu(), ci) and torch.equal(go.cpu(), co), (W, F, B)


def test_compute_python_json_config_runner(tmp_path):
    """the reference's example configuration for this operator (examples/pytorch/configs/
    split_table_batched_embeddings_ops.json: 1 table 228582 x 128 fp16, exact_row_wise_adagrad, batch 512, pooling 50)
    expressed in the same schema, plus a 4-table fp32 SGD build"""
    from param_amd.compute.python import run_benchmark

    def arg(name, typ, value):
        return {"type": typ, "name": name, "value": value}

    cfg = {"SplitTableBatchedEmbeddingBagsCodegen": {
        "build_iterator": "RangeConfigIterator", "input_iterator": "SplitTableBatchedEmbeddingBagsCodegenInputIterator",
        "config": [
            {"build": [{"args": [arg("num_tables", "int", 1), arg("rows", "int", 228582), arg("dim", "int", 128),
                                 arg("pooling", "int", 0), arg("weighted", "bool", False), arg("weights_precision", "str", "fp16")],
                        "kwargs": {"optimizer": {"type": "str", "value": "exact_row_wise_adagrad"}}}],
             "input": [{"args": [arg("batch_size", "int", 512), arg("pooling_factor", "int", 50)]}]},
            {"build": [{"args": [arg("num_tables", "int", 4), arg("rows", "int", 50000), arg("dim", "int", 64),
                                 arg("pooling", "int", 0), arg("weighted", "bool", True), arg("weights_precision", "str", "fp32")],
                        "kwargs": {"optimizer": {"type": "str", "value": "sgd"}, "lr": {"type": "float", "value": 0.05}}}],
             "input": [{"args": [arg("batch_size", "int", 256), arg("pooling_factor", "int", 10)]},
                       {"args": [arg("batch_size", "int", 1024), arg("pooling_factor", "int", 3)]}]}]}}
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(cfg))
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = run_benchmark.main(["-c", str(path), "-d", "cuda", "-b", "--warmup", "2", "--iteration", "3"])
    assert [r["id"] for r in res] == ["0|0_0|0_0", "1|0_0|0_0", "1|0_0|0_0"]   # the operator's input iterator restarts per input
    for r in res:
        assert r["op_name"] == "SplitTableBatchedEmbeddingBagsCodegen"
        assert len(r["metric"]["forward"]["gpu.time"]) == 3 and len(r["metric"]["backward"]["gpu.time"]) == 3
        assert all(0 < t < 1000 for t in r["metric"]["forward"]["gpu.time"] + r["metric"]["backward"]["gpu.time"])
    lines = [json.loads(ln) for ln in buf.getvalue().splitlines() if ln.startswith("{")]
    assert [ln["id"] for ln in lines] == [r["id"] for r in res] and lines[0]["config"]["build"]["args"][1] == 228582
    assert all(len(r["metric"]["forward"]["gpu.memory"]) == 3 for r in res)

    # ranged build + ranged / listed inputs, the two other execution modes, cache flush between calls
    rng = {"SplitTableBatchedEmbeddingBagsCodegen": {
        "build_iterator": "RangeConfigIterator", "input_iterator": "SplitTableBatchedEmbeddingBagsCodegenInputIterator",
        "config": [{"build": [{"args": [arg("num_tables", "int", 2), arg("rows", "int", 20000),
                                        dict(arg("dim", "int", [64, 128, 64]), __range__=["value"]), arg("pooling", "int", 0),
                                        arg("weighted", "bool", False),
                                        dict(arg("weights_precision", "str", ["fp16", "fp32"]), __range__=["value"])]}],
                    "input": [{"args": [dict(arg("batch_size", "int", [128, 256, 128]), __range__=["value"]),
                                        dict(arg("pooling_factor", "int", [5, 20]), __list__=["value"])]}]}]}}
    path.write_text(json.dumps(rng))
    with contextlib.redirect_stdout(io.StringIO()):
        ev = run_benchmark.main(["-c", str(path), "-d", "cuda", "-b", "-w", "1", "-i", "4", "--exec-mode", "continuous_events"])
        co = run_benchmark.main(["-c", str(path), "-d", "cuda", "-b", "-w", "1", "-i", "4", "--exec-mode", "continuous",
                                 "-o", str(tmp_path / "res")])
        fl = run_benchmark.main(["-c", str(path), "-d", "cuda", "-w", "1", "-i", "2", "--cuda-l2-cache", "off"])
        gr = run_benchmark.main(["-c", str(path), "-d", "cuda", "-b", "-w", "1", "-i", "3", "--cuda-graph", "--exec-mode", "continuous_events"])
    assert len(gr) == 16 and all(min(r["metric"]["forward"]["gpu.time"] + r["metric"]["backward"]["gpu.time"]) > 0 for r in gr)
    assert [r["id"] for r in ev] == [f"0|0_{b}|0_{i}" for b in range(4) for i in range(4)]
    assert [r["config"]["build"]["args"][2] for r in ev][::4] == [64, 64, 128, 128]
    assert [r["config"]["build"]["args"][5] for r in ev][::4] == ["fp16", "fp32", "fp16", "fp32"]
    assert [r["config"]["input"]["args"] for r in ev][:4] == [[128, 5], [128, 20], [256, 5], [256, 20]]
    assert all(len(r["metric"]["backward"]["gpu.time"]) == 4 and min(r["metric"]["backward"]["gpu.time"]) > 0 for r in ev)
    assert all(len(r["metric"]["forward"]["gpu.time"]) == 1 and len(r["metric"]["backward"]["gpu.time"]) == 1 for r in co)
    lines = (tmp_path / "res.json").read_text().splitlines()      # header line (run options + system information) + one line per run
    assert len(lines) == 17 and "run_options" in json.loads(lines[0]) and all("id" in json.loads(ln) for ln in lines[1:])
    assert len(fl) == 16 and "backward" not in fl[0]["metric"] and len(fl[0]["metric"]["forward"]["gpu.time"]) == 2


def test_quantised_sweep_single_gpu():
    """``comms.py --bitwidth {16,8,4,2}`` on one GPU (1-rank RCCL group): the payload really goes through the HIP row
    quantisers -- after the exchange the output holds restore(quantise(input)), checked against the numpy oracle -- and the
    report carries the quant / comms / de-quant split"""
    from oracle import rowquant as orq
    from param_amd.comms.pt import comms, comms_utils
    from param_amd.comms.pt.pytorch_backend_utils import collectiveArgsHolder

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_SIZE"):
        os.environ.pop(k, None)
    for bits, dim in ((8, 128), (16, 32), (4, 64), (2, 256)):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            res = comms.main(["--master-ip", "127.0.0.1", "--master-port", str(_port()), "--b", "64K", "--e", "16M", "--f", "16",
                              "--n", "4", "--w", "2", "--z", "1", "--collective", "all_to_allv,all_to_all", "--device", "rocm",
                              "--bitwidth", str(bits), "--quant-a2a-embedding-dim", str(dim)])
        assert [r["memSize"] for r in res] == [64 << 10, 1 << 20, 16 << 20] * 2
        assert all(r["bitwidth"] == bits and r["quant_p95_us"] > 0 and r["dequant_p95_us"] > 0 for r in res)
        assert buf.getvalue().count("COMMS-RES-QUANT-all_to_all") == 6
    # payload check at the backend level, GPU tensors, uneven "peer" chunks collapse to one chunk on 1 rank
    import torch.distributed as dist

    from param_amd.comms.pt.mi355_backend import MI355XBackend
    info = comms_utils.bootstrap_info_holder("127.0.0.1", str(_port()), 0,
                                             {"world_size": 1, "local_size": 1, "global_rank": 0, "local_rank": 0})
    bf = MI355XBackend(info, types.SimpleNamespace(device="cuda", backend="nccl"))
    bf.initialize_backend("127.0.0.1", info.master_port, backend="nccl")
    try:
        for bits in (16, 8, 4, 2):
            ca = collectiveArgsHolder()
            ca.group, ca.asyncOp, ca.world_size = bf.get_default_group(), False, 1
            comms_utils.initQuantCommCtx(ca, types.SimpleNamespace(bitwidth=bits, quant_a2a_embedding_dim=128))
            x = torch.randn(8192 * 4, 128, device=DEV) * 5
            ca.ipTensor, ca.opTensor = x.reshape(-1), torch.zeros(x.numel(), device=DEV)
            ca.ipTensor_split = ca.opTensor_split = [x.numel()]
            bf.all_to_allv(ca)
            want = orq.dequantize_rows(orq.quantize_rows(x.cpu().numpy(), bits), 128, bits)
            assert np.array_equal(ca.opTensor.cpu().numpy().reshape(-1, 128), want), bits
            ca.ipTensor, ca.opTensor = [x[:100].reshape(-1)], [torch.zeros(100 * 128, device=DEV)]
            bf.all_to_all(ca)
            assert np.array_equal(ca.opTensor[0].cpu().numpy().reshape(-1, 128), want[:100]), bits
    finally:
        bf.shutdown()
        assert not dist.is_initialized()


def test_graph_launches_sweep_single_gpu():
    """``comms.py --graph-launches N`` on one GPU (1-rank RCCL group): the collectives of a size are captured into one hipGraph
    and replayed (reference run_coll_cuda_graph, comms.py:375-450) -- all_to_allv / all_to_all_single / all_reduce survive stream
    capture through MI355XBackend, ``--c 1`` validates what the replays left, and the small-message end costs less per collective
    than the eager loop (one graph launch instead of numIters collective launches)."""
    from param_amd.comms.pt import comms

    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_SIZE"):
        os.environ.pop(k, None)
    common = ["--master-ip", "127.0.0.1", "--b", "1K", "--e", "4M", "--f", "64", "--n", "20", "--w", "3", "--z", "1", "--device", "rocm",
              "--collective", "all_to_allv,all_to_all_single,all_reduce", "--c", "1"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        eager = comms.main(common + ["--master-port", str(_port())])
        graph = comms.main(common + ["--master-port", str(_port()), "--graph-launches", "10"])
    assert [r["memSize"] for r in graph] == [r["memSize"] for r in eager] and len(graph) == 9
    assert all(r["p50_us"] > 0 for r in graph)
    small_e = [r["p50_us"] for r in eager if r["memSize"] <= 65536]
    small_g = [r["p50_us"] for r in graph if r["memSize"] <= 65536]
    assert sum(small_g) < sum(small_e), (small_g, small_e)


@pytest.mark.parametrize("n,extra,split,force", [(2, ["--tables", "16", "--rows", "1000000"], [8, 8], "224"),
                                                 (4, ["--tables", "26", "--rows", "400000"], [7, 7, 6, 6], "256"),
                                                 (2, ["--tables", "10", "--rows", "1000000", "--send-layout", "blocked"], [5, 5], ""),
                                                 (2, ["--workload", "criteo", "--mixed-dims"], [13, 13], "")])
def test_bench_multi_rank_flow_on_one_gpu(n, extra, split, force, tmp_path):
    """bench.py's N > 1 flow with REAL ranks: `torch.distributed.run` starts n processes, PARAM_AMD_BENCH_SHARED_GPU=1 puts all of
    them on GPU 0 and lets them talk over gloo (a flow check, and the line says so) -- table partition (the reference's
    `get_split_lengths_by_len`, dlrm.py:390-398: 26 tables on 4 ranks = [7, 7, 6, 6]), split lists, the exchange self-check (every rank
    rebuilds every peer's block from seeds: bit-equal), max-over-ranks clocks, ONE JSON line from rank 0."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["PARAM_AMD_BENCH_SHARED_GPU"] = "1"
    if force:                       # round 6: the compute stream (224 CUs / all) is selected by a trial inside the run; take either branch
        env["PARAM_AMD_BENCH_FORCE_CUS"] = force
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_port()), os.path.join(root, "bench.py"), "--gpus", str(n), "--steps", "5", "--warmup", "2",
           "--full", "--no-cpu-baseline", "--no-extra", "--batch", "2048"] + extra
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["steps"] == 5 and d["warmup"] == 2 and d["scaling"] == "weak" and d["value"] > 0
    assert d["config"]["tables_per_gpu"] == split and "shared_gpu_debug" in d["config"]
    sc = d["all_to_all"]["selfcheck"]
    assert sc["a2a_selfcheck"] == "ok" and sc["ranks"] == n and sc["min_peers_checked_over_ranks"] == n and sc["max_abs_diff"] == 0.0, sc
    assert d["fwd_bwd_step"]["lookups_per_s"] > 0
    # round 6: the stream choice is made in the run and recorded, with both trial times; the line ends with the compact summary
    sel = d["overlap"]["cu_mask_selection"]
    assert isinstance(sel, dict) and sel["step_s_224_cus"] > 0 and sel["step_s_256_cus"] > 0, sel
    assert d["overlap"]["cu_mask_selected"] == sel["selected"] and sel["selected"] in (224, 256)
    assert d["overlap"]["lookup_cus"] == sel["selected"]
    if force:
        assert sel["selected"] == int(force) and sel["forced_by_env"] == force, sel
    assert d["all_to_all"]["rccl"]["nranks"] == n
    assert list(d)[-1] == "summary" and d["config"]["requests_rotated"] >= 4
    if "--mixed-dims" in extra:
        assert d["config"]["dim"] == {"16": 9, "32": 9, "64": 3, "128": 5}, d["config"]["dim"]


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """A run without --full times the headline step only and prints the headline keys; --dump-outputs writes the last timed step's
    pooled embeddings, the same bits for the same arguments in two processes, and equal to the same tables and request looked up
    once more (the request of step W + K - 1 is request (W + K - 1) mod 4 of the rotation)."""
    import subprocess
    import sys

    import param_amd
    from param_amd.indices import tbe_request

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["--steps", "6", "--warmup", "1", "--tables", "8", "--rows", "200000", "--batch", "1024"]
    lines = []
    for k in range(2):
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args + ["--dump-outputs", str(tmp_path / f"d{k}")],
                           cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout[-2000:]
        lines.append(json.loads(out[0]))
    d = lines[0]
    assert d["steps"] == 6 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "lookups/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f32"
    for key in ("bwd_scatter_add", "fwd_bwd_step", "other_layout", "uniform", "bf16_T64", "criteo"):
        assert key not in d, key
    assert d["cpu_baseline"] is None and d["outputs"]["files"] == {"pooled_embeddings.npy": [8, 1024, 128]}
    a0, a1 = np.load(tmp_path / "d0" / "pooled_embeddings.npy"), np.load(tmp_path / "d1" / "pooled_embeddings.npy")
    assert a0.dtype == np.float32 and a0.shape == (8, 1024, 128) and np.array_equal(a0, a1)
    m = param_amd.BatchedEmbeddingBagMI355([200000] * 8, 128, device=DEV, layout="tbd", init="normal", seed=1000,
                                       fused_update=False)
    idx, off = tbe_request([200000] * 8, 1024, 20, alpha=1.05, device=DEV, seed=1 + 1000 * ((1 + 6 - 1) % 4))
    assert np.array_equal(m.lookup(idx, off).cpu().numpy(), a0)
