"""bench.py --gpus N starts its own ranks (no torchrun around it) and runs the path's exchange: here with world size 2 under gloo
on CPU tensors (`--exchange-only`: the launch, the pass-1 histogram all-reduce + finalize + broadcast, the BarcodesAssigned
counters' all-reduce; no kernels).  On the GPU box the same launcher runs the real two-pass leg over RCCL."""
import json
import os
import subprocess
import sys

import __graft_entry__ as graft


def _run(extra, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(graft.ROOT, "bench.py")] + extra, capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_launches_two_ranks_itself_and_exchanges():
    graft.build()
    r = _run(["--gpus", "2", "--exchange-only", "--backend", "gloo", "--whitelist", "50000", "--cells", "300"])
    assert r["n_gpus"] == 2 and r["backend"] == "gloo"
    assert r["same_used_list_on_all_ranks"] is True and 100 <= r["used_list"] <= 300
    # counters of rank 0 (1 per used barcode) + rank 1 (2 per used barcode) summed before the file is formatted
    assert r["assigned_rows"] == r["used_list"] and r["first_row_total"] == 3


def test_bench_launches_eight_ranks_and_counts_them():
    """the driver's first 8-GPU run rehearsed as far as a CPU box can: eight ranks (gloo), the process group reports 8, a collective sums over 8
    ranks, every rank holds the same used list, and each rank took its share of the host's CPU quota"""
    r = _run(["--gpus", "8", "--exchange-only", "--backend", "gloo", "--whitelist", "50000", "--cells", "300"])
    assert r["n_gpus"] == 8 and r["backend"] == "gloo"
    c = r["collective"]
    assert c["backend"] == "gloo" and c["world_size"] == 8 and c["ranks_counted"] == 8
    assert c["host_threads_per_rank"] >= 1
    assert r["same_used_list_on_all_ranks"] is True and r["first_row_total"] == sum(range(1, 9))


def test_single_rank_exchange_only_needs_no_process_group():
    r = _run(["--gpus", "1", "--exchange-only", "--whitelist", "20000", "--cells", "100"])
    assert r["n_gpus"] == 1 and r["backend"] == "none" and r["first_row_total"] == 1


def test_strong_scaling_split_sums_to_the_one_rank_run():
    """--total-reads: the same 200,000 reads (20 chunks with global seeds) on one rank and sharded over two: the all-reduced histogram, the
    used list after finalize and its ranks are identical (BASELINE configs[3]'s split, distributed.shard_range)"""
    common = ["--exchange-only", "--backend", "gloo", "--whitelist", "50000", "--cells", "300", "--total-reads", "200000"]
    one = _run(["--gpus", "1"] + common)
    two = _run(["--gpus", "2"] + common)
    three = _run(["--gpus", "3"] + common)
    assert one["scaling"] == two["scaling"] == "strong" and one["total_reads"] == 200_000
    assert one["hist_sum"] == two["hist_sum"] == three["hist_sum"] > 90_000
    assert one["used_list"] == two["used_list"] == three["used_list"] > 100
    assert one["used_list_digest"] == two["used_list_digest"] == three["used_list_digest"]
    assert two["same_used_list_on_all_ranks"] is True and three["same_used_list_on_all_ranks"] is True


def test_dump_outputs_sample_and_layout(tmp_path):
    """--dump-outputs without a GPU: the sampled reads are fixed, ascending and distinct (all reads up to the sample size); one float64 array
    per field of the three result structs, the 64-bit window bases split exactly into halves, within the 64 MiB bound at the full sample"""
    import importlib.util

    import numpy as np
    import torch

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(graft.ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert (bench.dump_rows(5) == np.arange(5)).all()
    rows = bench.dump_rows(10_000_000)
    assert rows.size == bench.DUMP_SAMPLE_READS and (np.diff(rows) > 0).all() and 0 <= rows[0] and rows[-1] < 10_000_000
    assert (rows == bench.dump_rows(10_000_000)).all()
    k = bench.DUMP_SAMPLE_READS
    g = torch.Generator().manual_seed(3)
    scan = torch.randint(-2 ** 31, 2 ** 31 - 1, (k, 8), dtype=torch.int32, generator=g)
    win = torch.randint(-2 ** 62, 2 ** 62, (k, 2), dtype=torch.int64, generator=g)
    out = torch.randint(-2 ** 31, 2 ** 31 - 1, (k, 4), dtype=torch.int32, generator=g)
    bench.dump_outputs(str(tmp_path), rows, scan, win, out, extra={"used_keys": np.arange(7, dtype=np.uint64)})
    lib = graft.load_package().lib
    want = {"read_index.npy", "used_keys.npy", "window_bases_lo.npy", "window_bases_hi.npy"}
    want |= {f"scan_{f}.npy" for f in lib.SCAN_RESULT_DTYPE.names if f != "reserved"}
    want |= {f"window_{f}.npy" for f in lib.BC_WINDOW_DTYPE.names if f != "bases"} | {f"bc_{f}.npy" for f in lib.BC_RESULT_DTYPE.names}
    assert set(os.listdir(tmp_path)) == want
    a = {n[:-4]: np.load(os.path.join(tmp_path, n)) for n in want}
    assert all(v.dtype == np.float64 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    w = win.numpy().view(lib.BC_WINDOW_DTYPE).reshape(-1)
    assert ((a["window_bases_hi"].astype(np.uint64) << np.uint64(32)) | a["window_bases_lo"].astype(np.uint64) == w["bases"]).all()
    s = scan.numpy().view(lib.SCAN_RESULT_DTYPE).reshape(-1)
    assert (a["scan_adapter_end"] == s["adapter_end"]).all() and (a["scan_flags"] == s["flags"]).all() and (a["read_index"] == rows).all()
    r = out.numpy().view(lib.BC_RESULT_DTYPE).reshape(-1)
    assert (a["bc_bc"] == r["bc"]).all() and (a["bc_found"] == r["found"]).all()
