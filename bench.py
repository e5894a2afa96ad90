#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on BASELINE.json configs[1]:
10 M synthetic Nanopore reads (16-bp BC + 12-bp UMI, ~Q12 error profile), ed <= 1 against the 3.6 M whitelist,
one MI355X per rank.  A step = one pass of the hot path over the rank's batch, inputs resident in HBM.

  python bench.py --gpus N --steps K --warmup W

N > 1 without WORLD_SIZE in the environment: this process starts the N ranks itself (`python -m torch.distributed.run
--nproc-per-node N bench.py ...` as a child, before anything here touches the GPU) and exits with the child's code; under
torch.distributed.run it is one of the ranks (one per GPU, RCCL).  Prints ONE JSON line on rank 0 (contract in the task
statement) with `config` and `roofline` (from the timed steps' own kernel times).  A plain run does only that: set-up, warm-up,
the timed steps, --dump-outputs, the line.

--full adds what is measured beside the step, never part of `value`: `cpu_baseline`, the one-time set build (`set_build_ms`,
`value_one_shot`), `hbm_measured`, `two_pass` (pass 1 -> RCCL all-reduce of the used-barcode histogram -> finalize -> pass 2 ->
all-reduce of the BarcodesAssigned counters: the one exchange of the path), `value_full_pass2` (the whole of pass 2 from
FASTQ text in HBM), `umi_stage` (the second half of BASELINE's metric: assignumis' UMI stage on the device, fed with names from a real
pass 2 of the same generator behind synthetic alignments), `value_bc_umi` (both stages in sequence), `host_to_host` (pass 2 through
the packed boundary: host FASTQ text in, `passed` / `failed` text out, PCIe and host threads included) and `file_to_file` (a directory
of *.fastq.gz through both passes to *_passed.fastq.gz / *_failed.fastq.gz + the two TSVs), bounded so that such a run stays within
minutes.

  --total-reads N: strong scaling (BASELINE configs[3]): N reads in all, sharded over the ranks in 1 M-read chunks with global seeds, so
                   every world size processes the same reads; `scaling` is then "strong".
  --config 2: BASELINE configs[2] (ed <= 2, two-pass, reads streamed in 10 M batches; K-BC2 in `roofline`).
  --config 4: BASELINE configs[4] (5' protocol --noPolyARequired, 737,280-key whitelist, ed <= 1; K-UMI leg in `umi`).
  --exchange-only: just the launch + the two exchanges on synthetic histograms (gloo on CPU tensors when no GPU is visible);
                   what tests/test_bench_launch.py runs on the CPU.
"""
import argparse
import importlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

# algorithmic bytes per read of the ed <= 1 matcher = 16 (window) + 16 (result) + 4 x 620 probes
ALG_BYTES_PER_READ_BC1 = 2512
# K-PA + K-AD scan: 2 x 175 bases (1 B/base as the reference holds them) + 32 B result
ALG_BYTES_PER_READ_SCAN = 382
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec
# K-BC2: 16 + 16 + 4 x ~56,000 probes
ALG_BYTES_PER_READ_BC2 = 224_032


def valu_peaks():
    """measured integer VALU issue ceilings of the chip (tools/valu_peak.hip -> profiles/r02/valu_peak.json), G wave-instructions/s:
    the 2-cycle forms (v_and/or/xor/add/sub/lshr/ashr/mov/not with VGPR or constant operands, only in runs of their own kind) and
    the 4-cycle forms (every three-operand op, v_max/v_min, v_lshl, anything with an SGPR operand, v_cmp, DPP, readlane ...)"""
    path = os.path.join(ROOT, "profiles", "r02", "valu_peak.json")
    try:
        d = json.load(open(path))
        return {"two_cycle_forms": float(d["peak_int_ginst_s"]), "four_cycle_forms": float(d["peak_vop3_ginst_s"]),
                "source": "profiles/r02/valu_peak.json (tools/valu_peak.hip, measured on this GPU model)"}
    except Exception:
        return {"two_cycle_forms": 256 * 4 * 2.4 / 2, "four_cycle_forms": 256 * 4 * 2.4 / 4, "source": "nominal 2.4 GHz (profiles/r02/valu_peak.json missing)"}


def host_cpu_quota():
    """CPUs this process may use: the cgroup quota (cpu.max) where there is one, else the affinity mask"""
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        if q[0] != "max":
            return max(1, int(round(int(q[0]) / int(q[1]))))
    except Exception:
        pass
    return len(os.sched_getaffinity(0))


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps (200 x 5 ms: a second of the step for whoever watches the GPU from outside)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reads", type=int, default=10_000_000, help="reads per GPU per step (configs[1]: 10 M)")
    ap.add_argument("--whitelist", type=int, default=3_600_000)
    ap.add_argument("--cells", type=int, default=5000)
    ap.add_argument("--cpu-sample", type=int, default=200_000, help="reads of the same workload timed on the host")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--e2e-reads", type=int, default=500_000,
                    help="reads of the bounded end-to-end leg (FASTQ text -> passed/failed text), reported beside `value`; 0 = skip")
    ap.add_argument("--e2e-lanes", default="1,2,4", help="worker lanes the end-to-end leg is run on, one run per count (a profile wants 1)")
    ap.add_argument("--two-pass-reads", type=int, default=200_000, help="reads per rank of the two-pass leg with the RCCL exchange; 0 = skip")
    ap.add_argument("--config", type=int, default=1, choices=(1, 2, 4), help="BASELINE configs[1] (default), configs[2] (ed<=2 two-pass) or configs[4] (5' --noPolyARequired, 737K whitelist, UMI clustering)")
    ap.add_argument("--batch", type=int, default=10_000_000, help="--config 2: reads per batch resident in HBM")
    ap.add_argument("--total-reads", type=int, default=0, help="strong scaling: this many reads in ALL, sharded over the ranks (configs[3]: 100000000 with --gpus 8)")
    ap.add_argument("--umi-molecules", type=int, default=50_000, help="molecules of the UMI-stage leg (each read six times); 0 = skip")
    ap.add_argument("--overlap", action="store_true",
                    help="run the timed steps as a two-stage pipeline: K-BC1 of a step on a second stream while K-SCAN of the next step runs")
    ap.add_argument("--assignumis-file-records", type=int, default=100_000,
                    help="records of the BAM -> tagged BAM leg (assignumis_file_to_file; 0 = off; needs the UMI leg)")
    ap.add_argument("--h2h-reads", type=int, default=500_000, help="reads per chunk of the host-to-host leg (packed boundary); 0 = skip")
    ap.add_argument("--f2f-reads", type=int, default=2_000_000, help="reads of the file-to-file leg (64 *.fastq.gz, both passes, gzip out); 0 = skip")
    ap.add_argument("--f2f-dir", default=None, help="scratch directory of the file-to-file leg (default: a temporary directory under /dev/shm or /tmp)")
    ap.add_argument("--single-process-gpus", type=int, default=0,
                    help="two-pass leg: ONE process drives this many GPUs (a context each, host threads) and sums the pass-1 histograms with "
                         "smi_hist_allreduce (RCCL inside the library) -- the shape of a JVM host; 0 = off (one process per GPU, torch.distributed)")
    ap.add_argument("--pack-kernel", action="store_true",
                    help="build the step's packed read ends with K-PACK (smi_pack_ends_device) from ASCII reads materialised on the device, instead of "
                         "the generator's own torch packer (same ends; outside the timed region either way)")
    ap.add_argument("--full", action="store_true",
                    help="also run what is measured beside the timed step: CPU baseline, set build, HBM probe and the two-pass, end-to-end, UMI, "
                         "host-to-host and file-to-file legs (without it: set-up, warm-up, the timed steps, --dump-outputs, the line)")
    ap.add_argument("--exchange-only", action="store_true")
    ap.add_argument("--backend", default=None, help="torch.distributed backend (default: nccl with GPUs, gloo without)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last step computed (rank 0) as DIR/<name>.npy, float64: scan results, barcode "
                         "windows and barcode results of every read, or of a fixed seeded sample of %d reads when there are more" % DUMP_SAMPLE_READS)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


# --dump-outputs: reads of a step written at most (24 float64 columns, 48 MiB), and the seed of the sample when a step has more
DUMP_SAMPLE_READS = 1 << 18
DUMP_SEED = 20240607
DUMP_MAX_BYTES = 64 << 20


def dump_rows(n):
    """the reads --dump-outputs writes, ascending: all n of them, or a fixed seeded sample when n > DUMP_SAMPLE_READS"""
    if n <= DUMP_SAMPLE_READS:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_SAMPLE_READS, replace=False)).astype(np.int64)


def dump_outputs(path, rows, scan_rows, win_rows, out_rows, extra=None):
    """write the step's results at `rows` (read indices) as float64 arrays, one per field of the C structs: scan_<field> (scan_result),
    window_<field> (bc_window; the 64-bit bases as two 32-bit halves so that float64 holds them exactly), bc_<field> (bc_result) and
    read_index; `extra`: further named arrays of the step.  *_rows: the device tensors of the step gathered at `rows`."""
    lib = graft.load_package().lib
    cols = {"read_index": np.asarray(rows, dtype=np.float64)}
    for prefix, t, dt in (("scan", scan_rows, lib.SCAN_RESULT_DTYPE), ("window", win_rows, lib.BC_WINDOW_DTYPE), ("bc", out_rows, lib.BC_RESULT_DTYPE)):
        a = t.cpu().numpy().view(dt).reshape(-1)
        assert a.size == len(rows), (prefix, a.size, len(rows))
        for f in dt.names:
            if f == "reserved":
                continue
            if a[f].dtype == np.uint64:
                cols[f"{prefix}_{f}_lo"] = (a[f] & np.uint64(0xFFFFFFFF)).astype(np.float64)
                cols[f"{prefix}_{f}_hi"] = (a[f] >> np.uint64(32)).astype(np.float64)
            else:
                cols[f"{prefix}_{f}"] = a[f].astype(np.float64)
    for name, v in (extra or {}).items():
        cols[name] = np.asarray(v, dtype=np.float64)
    total = sum(v.nbytes for v in cols.values())
    if total > DUMP_MAX_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_MAX_BYTES}-byte bound")
    os.makedirs(path, exist_ok=True)
    for name, v in cols.items():
        np.save(os.path.join(path, name + ".npy"), v)


def free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(args):
    """--gpus N > 1 and no WORLD_SIZE: start the ranks as a CHILD of this process (which has not touched the GPU and never
    replaces itself) and hand its exit code on"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(rank_threads(args.gpus)))     # a rank's share of the host (the set build and the generator run host-side torch ops)
    return subprocess.call(cmd, env=env)


def rank_threads(world):
    """host threads of one rank when `world` ranks share this host's CPU quota"""
    return max(1, host_cpu_quota() // max(1, world))


def end_to_end_leg(ctx, synth, dev, used, n, lane_counts=(1, 2, 3)):
    """Whole pass 2 of `scanfastq` for one chunk, FASTQ text resident in HBM -> finished `passed` / `failed` FASTQ text in
    HBM, every stage on the device: K-FQ (record index; bases and qualities are read in place), K-PACKR + K-CHIM + fragment offsets, K-PACK, K-SCAN,
    K-BC1 (same 3.6 M whitelist as the step), K-WRITE.  10 % of the input records are ligation chimeras (two molecules in one
    record), so the splitter has real work.  Reported beside `value`, never part of it.

    One lane = one chunk at a time (`ms`: what a chunk takes from its first kernel to its last).  A job is many chunks: with several
    worker lanes (a context lane, a stream and a set of buffers each, one host thread per lane, as WorkerReadscanner runs nCPU chunks side by
    side) the chunks of different lanes overlap on the GPU -- the splitter's filter and K-SCAN are bound by integer issue, K-FQ / K-PACKR / K-WRITE
    by HBM, and the host's short waits between the library calls of one lane are filled by the other lanes' kernels.  `lanes` has the runs."""
    import threading

    rd = synth.gen_reads(n, used, seed=77, device=dev)
    text, _buf, offs0 = synth.fastq_text_device(rd, chimera_frac=0.10)   # 10 % of the records are two molecules joined
    del rd
    n = int(offs0.numel()) - 1
    total_text, total_bases = int(text.numel()), int(offs0[-1])

    class Lane:
        """one worker lane: a context lane (stream, arena) and ONE library call per chunk -- smi_scanfastq_pass2_chunk with the text read in place
        and the two output texts left in the lane's arena (device_output): four waits for the host per chunk (line count, record index, fragment
        count, output sizes)"""

        def __init__(self, c):
            self.c, self.stream = c, torch.cuda.Stream(device=dev)
            self.out_p = self.out_f = None
            self.tot, self.m, self.t_call = None, 0, 0.0

        def run(self):
            t0 = time.perf_counter()
            p, f, info = self.c.scanfastq_pass2_chunk(text, max_ed=1, device_output=True, copy=False)
            self.t_call += time.perf_counter() - t0
            assert info["n_records_in"] == n
            self.out_p, self.out_f = p, f
            self.tot, self.m = (len(p), len(f), int(info["n_passed"])), int(info["n_records_out"])

        def repeat(self, k):
            for _ in range(k):
                self.run()          # (returns when the lane's stream has drained)

    torch.cuda.synchronize()
    lanes = [Lane(ctx)]
    reps = 20
    runs, first = [], None
    for k in lane_counts:
        while len(lanes) < k:
            lanes.append(Lane(ctx.lane()))
        for L in lanes[:k]:
            L.repeat(3)
        for L in lanes[:k]:
            L.t_call = 0.0
        th = [threading.Thread(target=L.repeat, args=(reps,)) for L in lanes[:k]]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        dt_k = (time.perf_counter() - t0) / reps
        if first is None:
            first = (lanes[0].out_p.tensor().clone(), lanes[0].out_f.tensor().clone())
        same = all(L.tot == lanes[0].tot and torch.equal(L.out_p.tensor(), first[0]) and torch.equal(L.out_f.tensor(), first[1]) for L in lanes[:k])
        runs.append({"lanes": k, "ms_per_chunk_and_lane": dt_k * 1e3, "reads_per_s": n * k / dt_k, "same_text_on_every_lane": bool(same),
                     "ms_inside_the_call": max(L.t_call for L in lanes[:k]) / reps * 1e3})
    dt = runs[0]["ms_per_chunk_and_lane"] * 1e-3
    best = max(runs, key=lambda r: r["reads_per_s"])
    state = {"tot": lanes[0].tot, "m": lanes[0].m}
    # the stages with HIP events of their own (library timing switch), one more pass; K-CHIM = the splitter's whole launch sequence
    ctx.set_timing(True)
    lanes[0].repeat(1)
    torch.cuda.synchronize()
    stage_ms = {"K-CHIM (filter + select/align/fold + walk/gate/align/rules)": ctx.kernel_ms(ctx.K_CHIMERA), "K-SCAN": ctx.kernel_ms(ctx.K_SCAN),
                "K-BC1": ctx.kernel_ms(ctx.K_BC_MATCH)}
    ctx.set_timing(False)
    for L in lanes[1:]:
        L.c.close()
    moved = total_text + state["tot"][0] + state["tot"][1]
    ach = moved * best["lanes"] / (best["ms_per_chunk_and_lane"] * 1e-3) / 1e9
    return {"reads": n, "chimeric_input_frac": 0.10, "records_out": state["m"], "passed": state["tot"][2], "text_in_bytes": total_text,
            "text_out_bytes": state["tot"][0] + state["tot"][1], "ms": dt * 1e3, "reads_per_s_one_lane": n / dt, "repetitions": reps,
            "lanes": runs, "lanes_at_best": best["lanes"], "reads_per_s": n / dt, "reads_per_s_best_lanes": best["reads_per_s"],
            "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": None,
                         "basis": "FASTQ text in + passed / failed text out per chunk (the least a text-to-text pass must move) over the job's time "
                                  "(`lanes_at_best` chunks side by side)",
                         "stage_ms": stage_ms,
                         "limiter": "the splitter's filter (K-CHIM-A: 4-mer gates + a Levenshtein bound for every gated position of every read) is integer VALU "
                                    "issue; then the writer (K-WRITE beside K-WNAME), K-FQ's sweep, K-PACKR; with one lane also the four waits for "
                                    "the host inside the call (line count, record index, fragment count, output sizes)",
                         "kernel_trace": "profiles/r06/e2e_kernel_stats.csv (one lane)"},
            "stages": "K-FQ, K-PACKR, K-CHIM, fragment offsets, K-PACK, K-SCAN, K-BC1 (3.6M whitelist), K-WRITE; FASTQ text in HBM -> "
                      "passed/failed FASTQ text in HBM; ONE library call per chunk (smi_scanfastq_pass2_chunk: device text read in place, device_output)"}



def hbm_probe(dev):
    """What this GPU's memory system delivers, measured beside the 8 TB/s of the data sheet (SURVEY 8d asks for the copy rate next to the peak):
    a device-to-device copy of 2 GiB (read + write) and dependent-free random 4-byte gathers into a 512 MiB table
    (the size of K-BC1's offset filter) and into an 8 GiB one (the size of its neighbourhood table) -- the ceiling a kernel of random sector reads
    can reach, whatever its arithmetic.  torch kernels, timed with events; a few hundred milliseconds in all."""
    def timed(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e-3

    out = {}
    try:
        n = 1 << 29                                          # 2 GiB of int32
        a = torch.empty(n, dtype=torch.int32, device=dev).fill_(1)
        b = torch.empty_like(a)
        t = timed(lambda: b.copy_(a))
        out["copy_GBps"] = 2 * 4 * n / t / 1e9
        del b
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        m = 1 << 26                                          # 64 M gathers per call
        for name, words in (("gather_512MiB", 1 << 27), ("gather_8GiB", 1 << 31)):
            table = a[:words] if words <= n else torch.empty(words, dtype=torch.int32, device=dev).fill_(1)
            idx = torch.randint(0, words, (m,), device=dev, generator=g, dtype=torch.int64)
            t = timed(lambda: torch.take(table, idx), reps=3)
            out[name + "_G_per_s"] = m / t / 1e9
            del idx, table
        out["note"] = ("torch copy_ / take; the gathers are independent 4-byte reads at random addresses (one 64-B sector each), 64 M per call")
    except RuntimeError as e:                                # (not enough free memory beside the bench's own buffers: the probe is optional)
        out["error"] = str(e)[:200]
    return out


def pmc_table():
    """profiles/pmc_traffic.json: HBM bytes per launch from the rocprofv3 FETCH_SIZE / WRITE_SIZE passes (tools/pmc_traffic.py)"""
    try:
        return json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
    except Exception:
        return {}


def roofline_entry(name, key, ms, alg_bytes_per_unit, units, tj):
    """HBM roofline fields of one kernel launch set.  `algorithmic` always carries SURVEY 8d's model (bytes per unit x units / time).
    `achieved` / `frac` are that figure as long as it describes the kernel (frac <= 1); where the kernel answers the model's probes without
    moving its bytes (K-BC1's neighbourhood table, K-BC2's filters) the model exceeds the peak and `achieved` / `frac` are the COUNTER
    traffic (FETCH_SIZE + WRITE_SIZE, scaled per unit from the profiled launch) over the measured time instead -- what the HBM really moved."""
    ach_alg = alg_bytes_per_unit * units / (ms * 1e-3) / 1e9
    e = tj.get(key, {})
    traffic = None
    if e.get("hbm_bytes_per_launch") and e.get("reads_per_launch"):
        traffic = int(e["hbm_bytes_per_launch"] * (units / e["reads_per_launch"]))
    d = {"kernel": name, "kernel_ms": ms, "peak": HBM_PEAK_GBS, "unit": "GB/s", "traffic": traffic,
         "algorithmic": {"achieved": ach_alg, "frac": ach_alg / HBM_PEAK_GBS, "bytes_per_unit": alg_bytes_per_unit}}
    if ach_alg / HBM_PEAK_GBS > 1.0 and traffic:
        ach = traffic / (ms * 1e-3) / 1e9
        d.update(achieved=ach, frac=ach / HBM_PEAK_GBS, basis="counter traffic (the algorithmic model exceeds the HBM peak for this kernel)",
                 counters_from=e.get("source"), counters_commit=e.get("commit", tj.get("commit")))
    else:
        d.update(achieved=ach_alg, frac=ach_alg / HBM_PEAK_GBS, basis="algorithmic bytes (SURVEY 8d)")
        if traffic:
            d.update(counters_from=e.get("source"), counters_commit=e.get("commit", tj.get("commit")))
    vi = e.get("valu_insts_per_launch")
    if vi and e.get("reads_per_launch"):
        vp = valu_peaks()
        rate = vi * (units / e["reads_per_launch"]) / (ms * 1e-3) / 1e9
        d["valu_issue"] = {"achieved_ginst_s": rate, "peak_ginst_s": vp["four_cycle_forms"], "frac": rate / vp["four_cycle_forms"],
                           "peak_2cycle_forms_ginst_s": vp["two_cycle_forms"], "frac_of_2cycle_peak": rate / vp["two_cycle_forms"],
                           "peaks_from": vp["source"]}
    return d


def umi_stage_leg(pkg, synth, ctx, used, n_mol, copies=6, genes_per=10):
    """BASELINE's "+UMI": assignumis' UMI stage (smi_assignumis_chunk: K-UPARSE, region grouping, key sort, K-UMI, K-UCLUST, K-UTAG) on
    names that come out of a real pass 2 of the same synthetic generator, every molecule read `copies` times with an error now and then,
    aligned to synthetic loci.  One chunk per call, host arrays in, tags out (the PCIe transfers and the host's region grouping are inside);
    several chunks side by side on worker lanes, as UmiFinderWorker runs several batches."""
    import ctypes
    import threading

    scanfastq = importlib.import_module(graft.PKG_NAME + ".scanfastq")
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    rng = np.random.default_rng(5)
    genes = max(1, n_mol // genes_per)
    ctx.set_barcode_set(used.cpu().numpy().astype(np.uint64), mode=0)
    mol = synth.gen_reads(n_mol, used, seed=77, err=0.0, q_mean=20.0)
    seqs, quals = zip(*(synth.materialize(mol, i) for i in range(n_mol)))
    text = "".join(f"@m{i} ch=1\n{s_}\n+\n{q}\n" for i, (s_, q) in enumerate(zip(seqs, quals))).encode()
    passed, _failed, _info = ctx.scanfastq_pass2_chunk(text, max_ed=1, split_chimeras=False)
    names = [ln[1:].split(b" ")[0].decode() for ln in bytes(passed).split(b"\n")[0::4] if b"_bc=" in ln]
    gene = rng.integers(0, genes, len(names))
    rows = []
    for m, q in enumerate(names):
        head, x_rest = q.split("_X=")
        x, rest = x_rest.split("_", 1)
        for c in range(copies):
            xs = list(x)
            if rng.random() < 0.3:  # a sequencing error inside the window
                xs[int(rng.integers(0, len(xs)))] = "ACGT"[int(rng.integers(0, 4))]
            rows.append((int(gene[m]) * 5_000 + int(rng.integers(-100, 100)), f"{head.replace('m', 'r%d_' % c, 1)}_X={''.join(xs)}_{rest}", 16 if gene[m] & 1 else 0))
    rows.sort(key=lambda t: t[0])
    umi_stage_leg.rows = rows          # the same records as a BAM file: assignumis_file_leg
    n = len(rows)
    enc = [t[1].encode() for t in rows]
    noff = np.zeros(n + 1, dtype=np.uint32)
    noff[1:] = np.cumsum([len(e) for e in enc])
    nbuf = np.frombuffer(b"".join(enc) + b"\0" * 16, dtype=np.uint8)
    coff = np.arange(n + 1, dtype=np.uint32)
    cbuf = np.full(n + 1, 1200 << 4, dtype=np.uint32)  # one M operation per record
    fl = np.array([t[2] for t in rows], dtype=np.uint16)
    p0 = np.array([max(t[0], 0) + 1_000_000 for t in rows], dtype=np.int32)

    def pinned(a):
        """a copy of the array in page-locked memory (smi_host_alloc), as the host hands its chunk over: uploads at link speed and side by side
        on several lanes (pageable memory goes through the runtime's one staging path)"""
        pb = lib.PinnedBuffer(max(a.nbytes, 1))
        v = pb.array[:a.nbytes].view(a.dtype)
        v[:] = a.reshape(-1)
        return pb, v

    keep_pinned = []

    def make_call(c, o):
        cfg = lib.AssignUmisConfig()
        c._check(c._lib.smi_assignumis_default_config(ctypes.byref(cfg)))
        cfg.n_threads = 2
        nd = ctypes.c_int32(0)
        arrs = [pinned(a) for a in (nbuf, noff, fl, p0, cbuf, coff)]      # every lane's own chunk buffers
        keep_pinned.extend(pb for pb, _ in arrs)
        a_n, a_no, a_f, a_p, a_c, a_co = (v for _, v in arrs)

        def call():
            c._check(c._lib.smi_assignumis_chunk(c._h, a_n.ctypes.data, a_no.ctypes.data, a_f.ctypes.data, a_p.ctypes.data, a_c.ctypes.data, a_co.ctypes.data,
                                                 n, ctypes.byref(cfg), o.ctypes.data, ctypes.byref(nd)))
        return call

    runs, first = [], None
    for lanes in (1, 4, 8, 16):
        ctxs = [ctx] + [ctx.lane() for _ in range(lanes - 1)]
        out_pins = [lib.PinnedBuffer(n * lib.UMI_TAG_DTYPE.itemsize) for _ in ctxs]
        keep_pinned.extend(out_pins)
        outs = [pb.array.view(lib.UMI_TAG_DTYPE) for pb in out_pins]
        calls = [make_call(c, o) for c, o in zip(ctxs, outs)]
        for f in calls:
            f()
        per = 4
        th = [threading.Thread(target=lambda f=f: [f() for _ in range(per)]) for f in calls]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        dt = time.perf_counter() - t0
        first = outs[0].copy() if first is None else first
        runs.append({"lanes": lanes, "records_per_s": n * lanes * per / dt, "ms_per_chunk": dt / per * 1e3,
                     "same_tags_on_every_lane": all(o.tobytes() == first.tobytes() for o in outs)})
        for c in ctxs[1:]:
            c.close()
        for pb in keep_pinned:
            pb.close()
        keep_pinned.clear()
    best = max(runs, key=lambda r: r["records_per_s"])
    return {"records_per_chunk": n, "molecules": len(names), "copies": copies, "loci": genes, "clustered": int((first["flags"] & 4 != 0).sum()),
            "with_region": int((first["region"] >= 0).sum()), "runs": runs, "records_per_s": best["records_per_s"], "lanes_at_best": best["lanes"],
            "stages": "K-UPARSE (names, UMI windows, clustering positions), region grouping (sort on the device, chains and their refinement on the host), key sort, K-UMI, K-UCLUST "
                      "(groups <= 100 reads; larger ones on the host), K-UTAG; host arrays (page-locked) in, tags out"}


def assignumis_file_leg(pkg, synth, ctx, rows, n_threads):
    """`assignumis` BAM -> tagged BAMs + gene-count tables with no per-record Python (assignumis.write_tagged_bams_native): BGZF inflate and
    record index on host threads, BamReader's chunks through smi_assignumis_chunk (device), the writer (tags, htsjdk's attribute order,
    coordinate-comparator order per batch, gene counts) on host threads, BGZF by K-DEFLATE.  Input: the records of the UMI leg as a BAM with
    1,200-base reads and minimap2's aux fields, BGZF-compressed by the host at level 1.  Never part of `value`."""
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    au = importlib.import_module(graft.PKG_NAME + ".assignumis")
    rows = [(max(p, 0) + 1_000_000, nm, fl) for p, nm, fl in rows]
    t0 = time.perf_counter()
    raw = synth.bam_from_rows(rows)
    data = lib.bgzf_deflate(raw, level=1, n_threads=n_threads).tobytes()
    gen_s = time.perf_counter() - t0
    gc = lib.GeneCounts()
    au.write_tagged_bams_native(ctx, data, n_threads=n_threads, chunk_size=250_000)       # warm-up (allocations, first launches)
    best = None
    for _ in range(2):
        gc.close()
        gc = lib.GeneCounts()
        z_bc, z_umi, info = au.write_tagged_bams_native(ctx, data, n_threads=n_threads, chunk_size=250_000, gene_counts=gc)
        if best is None or info["wall_s"] < best[2]["wall_s"]:
            best = (len(z_bc), len(z_umi), info)
    n_bc, n_umi, info = best
    res = {"records": info["records"], "clustered": info["clustered"], "batches": info["batches"], "wall_s": info["wall_s"],
           "records_per_s": info["records"] / info["wall_s"], "seconds": info["seconds"], "bam_in_bytes": len(data), "bam_inflated_bytes": info["bam_bytes"],
           "bam_out_bytes": n_bc, "umifound_out_bytes": n_umi, "gene_count_entries": gc.info()["region_entries"], "host_threads": n_threads,
           "generate_input_s": gen_s, "note": "chunk size 250,000 records as shipped (config.xml:78); the whole input is one chromosome"}
    gc.close()
    return res


def host_to_host_leg(pkg, synth, ctx, dev, used, n):
    """pass 2 of one chunk from host FASTQ text to host `passed` / `failed` text through the PACKED boundary (bit-planes up, decisions down,
    records written by host threads): what a JNI host obtains, PCIe and host cores included.  Never part of `value`.  Three ways to spend the
    host's cores (lanes x threads per lane) are run, the best is reported (all of them are in `runs`)."""
    import threading

    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q[0] == "max" else float(q[0]) / float(q[1])
    except Exception:
        quota = None
    cpus = max(1, min(int(quota) if quota else 16, len(os.sched_getaffinity(0))))
    ctx.set_barcode_set_device(used.to(torch.int32), mode=0)
    rd = synth.gen_reads(n, used, seed=9, device=dev)
    text = synth.fastq_text_device(rd)[0]
    total = int(text.numel())
    host_text = text.cpu().numpy()
    del rd, text
    max_lanes = 8
    ctxs = [ctx] + [ctx.lane() for _ in range(max_lanes - 1)]
    pins = [lib.PinnedBuffer(total) for _ in range(max_lanes)]
    for pb in pins:
        pb.array[:] = host_text
    runs, out_bytes = [], 0
    # (lanes, threads): one lane's host stages overlap another's device side; more lanes with fewer threads each need no barrier between threads
    for lanes, threads in ((2, cpus), (4, max(1, cpus // 2)), (8, max(1, cpus // 4))):
        for c, pb in zip(ctxs[:lanes], pins):
            p, f, _ = c.scanfastq_pass2_chunk(pb.array, copy=False, packed=True, n_threads=threads)   # warm-up: arena, pinned buffers
            out_bytes = int(p.size + f.size)
        per = 3
        th = [threading.Thread(target=lambda c=c, pb=pb, threads=threads: [c.scanfastq_pass2_chunk(pb.array, copy=False, packed=True, n_threads=threads)
                                                                             for _ in range(per)]) for c, pb in zip(ctxs[:lanes], pins)]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        dt = time.perf_counter() - t0
        runs.append({"lanes": lanes, "host_threads_per_lane": threads, "reads_per_s": n * lanes * per / dt, "ms_per_chunk": dt / per * 1e3})
    for c in ctxs[1:]:
        c.close()
    for pb in pins:
        pb.close()
    best = max(runs, key=lambda r: r["reads_per_s"])
    return {"reads_per_chunk": n, "lanes": best["lanes"], "host_threads_per_lane": best["host_threads_per_lane"], "reads_per_s": best["reads_per_s"],
            "ms_per_chunk": best["ms_per_chunk"], "runs": runs,
            "text_in_bytes": total, "text_out_bytes": out_bytes, "link_bytes_per_read": "~0.7 KB up (bit-planes), ~80 B down (decisions)",
            "host_cpus_visible": len(os.sched_getaffinity(0)), "host_cpu_quota": quota,
            "note": "smi_scanfastq_pass2_chunk_packed on worker lanes of one GPU; host-bound (index, planes and records are written by the host's "
                    "cores): ~1 M reads/s per core on this box, against 14.5 M reads/s for the text worker, which the link bounds"}


def file_to_file_leg(pkg, synth, ctx, dev, wl, used, n_reads, scratch=None, n_files=64, workers=int(os.environ.get("SMI_BENCH_F2F_WORKERS", "16"))):
    """`scanfastq -d <dir> -o <dir> --bcEditDistance 1 --compress` (quickrun-2.1.sh:35) on n_files synthetic *.fastq.gz, both passes, gzip
    out (K-DEFLATE on the device; beside it a quarter of the files with zlib level 6 on the host), wall clock from the first byte read to the last byte written (inputs in the page cache).  The README's figure for the
    Java reference: 20.8 k reads/s on 96 cores (README.md:106)."""
    import shutil
    import tempfile

    run_files = importlib.import_module(graft.PKG_NAME + ".run_files")
    base = scratch or tempfile.mkdtemp(prefix="smi_f2f_", dir="/dev/shm" if os.path.isdir("/dev/shm") and scratch is None else None)
    in_dir, out_dir = os.path.join(base, "in"), os.path.join(base, "out")
    try:
        t0 = time.perf_counter()
        n = run_files.write_synthetic_dir(synth, in_dir, n_files, max(1, n_reads // n_files), used, dev, seed=9000, chimera_frac=0.05)
        t_gen = time.perf_counter() - t0
        keys = np.sort(wl.cpu().numpy().astype(np.uint64))
        info = run_files.run(ctx, in_dir, out_dir, max_ed=1, n_workers=workers, reads_per_chunk=100_000, whitelist_keys=keys, gz="device")
        info["gz_in_bytes"] = sum(os.path.getsize(os.path.join(in_dir, f)) for f in os.listdir(in_dir))
        info["generate_inputs_s"] = t_gen
        info["scratch"] = "/dev/shm (RAM)" if base.startswith("/dev/shm") else base
        info["host_cpus_visible"] = len(os.sched_getaffinity(0))
        info["reference_readme_reads_per_s"] = 20_800
        info["note"] = ("inflate (host zlib) with pass 1 of every inflated file behind it (text worker, whole whitelist) -> finalize / rank -> pass 2 (text worker, used list; records written "
                        "in HBM and deflated there by K-DEFLATE, one gzip member per chunk and stream) -> files + BarcodeList.tsv + BarcodesAssigned.tsv + "
                        "ReadScanner.tsv; %d worker threads, one GPU lane each; qualities uniform per base (incompressible, as real ones nearly are)" % workers)
        # the same run with the output deflated by zlib level 6 on the host's threads (what round 2 could do): smaller sample, it is 5 - 10 x slower
        shutil.rmtree(out_dir, ignore_errors=True)
        keep = sorted(os.listdir(in_dir))[: max(1, n_files // 4)]
        sub = os.path.join(base, "in_zlib")
        os.makedirs(sub)
        for f in keep:
            os.link(os.path.join(in_dir, f), os.path.join(sub, f))
        z = run_files.run(ctx, sub, out_dir, max_ed=1, n_workers=workers, reads_per_chunk=100_000, gz_level=6, whitelist_keys=keys, gz="zlib")
        info["host_zlib6"] = {k: z[k] for k in ("files", "reads", "wall_s", "reads_per_s", "inflate_and_pass1_s", "pass2_and_gzip_s", "gz_out_bytes",
                                                 "text_out_bytes")}
        assert info["reads"] == n
        return info
    finally:
        if scratch is None:
            shutil.rmtree(base, ignore_errors=True)


def init_dist(args, dev=None):
    """-> (dist module or None, rank, local_rank, world)"""
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return None, rank, local_rank, world
    import torch.distributed as dist

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    # (torch.distributed.run exports OMP_NUM_THREADS=1 when the caller set none: a rank then takes its share of the quota for its host-side torch work)
    if os.environ.get("OMP_NUM_THREADS", "1") == "1":
        torch.set_num_threads(rank_threads(world))
    backend = args.backend or ("nccl" if torch.cuda.is_available() else "gloo")
    if backend == "nccl":
        dist.init_process_group(backend="nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    else:
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return dist, rank, local_rank, world


def collective_report(dist, dev):
    """what the process group says about itself, and a count the collective made: every rank adds 1 (and its device ordinal) -- `ranks_counted`
    is the number of ranks the backend (RCCL under "nccl") really summed over, `devices_seen` the number of distinct devices among them"""
    if dist is None:
        return {"backend": "none (1 rank)", "world_size": 1, "ranks_counted": 1, "devices_seen": 1}
    on = dev if dist.get_backend() == "nccl" else torch.device("cpu")
    ones = torch.ones(1, dtype=torch.int64, device=on)
    dist.all_reduce(ones, op=dist.ReduceOp.SUM)
    mask = torch.zeros(64, dtype=torch.int64, device=on)
    mask[(dev.index or 0) % 64] = 1
    dist.all_reduce(mask, op=dist.ReduceOp.MAX)
    return {"backend": dist.get_backend(), "world_size": dist.get_world_size(), "ranks_counted": int(ones.item()), "devices_seen": int(mask.sum().item()),
            "host_threads_per_rank": torch.get_num_threads()}


def exchange_only(args):
    """the launch and the two exchanges of the path on synthetic counters: every rank draws its own pass-1 histogram over the same
    key list, `distributed.pass1_finalize` all-reduces it (RCCL on device tensors / gloo on CPU tensors), finalizes, broadcasts;
    then the BarcodesAssigned counters are all-reduced.  No kernel runs: this is what the CPU test can exercise."""
    dist, rank, local_rank, world = init_dist(args)
    on_gpu = torch.cuda.is_available() and (args.backend or "nccl") == "nccl"
    dev = torch.device("cuda", local_rank) if on_gpu else torch.device("cpu")
    if on_gpu:
        torch.cuda.set_device(local_rank)
    pkg = graft.load_package()
    distributed = importlib.import_module(graft.PKG_NAME + ".distributed")
    n_keys = min(args.whitelist, 200_000)
    g = np.random.default_rng(5)
    keys = np.sort(g.choice(1 << 32, size=n_keys, replace=False).astype(np.uint64))      # identical on every rank
    cells = g.choice(n_keys, size=min(args.cells, n_keys // 4), replace=False)
    h = np.zeros(n_keys, dtype=np.int32)
    if args.total_reads > 0:
        # strong scaling: --total-reads in all, as 10,000-read chunks (FastqFileReader's) with GLOBAL seeds dealt to the ranks in contiguous
        # runs -- the split of the main bench; whatever the world size, the sum over the ranks is the same histogram
        n_chunks = (args.total_reads + 9_999) // 10_000
        lo, hi = distributed.shard_range(n_chunks, rank, world)
        for cid in range(lo, hi):
            gc = np.random.default_rng(1000 + cid)
            m = min(10_000, args.total_reads - cid * 10_000)
            np.add.at(h, cells[gc.integers(0, cells.size, size=m // 2)], 1)              # half of the reads carry a whitelisted barcode
            h[gc.choice(n_keys, size=3, replace=False)] += 1                              # background
        record_count = hi - lo
    else:
        gr = np.random.default_rng(100 + rank)
        h[cells] = gr.poisson(40, size=cells.size)                                        # this rank's share of the reads
        h[gr.choice(n_keys, size=200, replace=False)] += 1                                # background
        record_count = 50
    hist = torch.from_numpy(h).to(dev)
    t0 = time.perf_counter()
    k, c, r = distributed.pass1_finalize(hist, keys, record_count=record_count)
    if on_gpu:
        torch.cuda.synchronize()
    t_ex = time.perf_counter() - t0
    counts = torch.zeros((n_keys, 3), dtype=torch.int32, device=dev)
    counts[torch.from_numpy(np.searchsorted(keys, k)).to(dev), 0] = 1 + rank
    tsv = distributed.assigned_counts_tsv(counts, keys, max_ed=1)
    digest = int(np.bitwise_xor.reduce(k)) ^ int(c.sum()) ^ k.size
    same = True
    if dist is not None:
        t = torch.tensor([digest & 0x7FFFFFFFFFFFFFFF, -(digest & 0x7FFFFFFFFFFFFFFF)], dtype=torch.int64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        same = int(t[0].item()) == -int(t[1].item())
        dist.barrier()
    coll = collective_report(dist, dev if on_gpu else torch.device("cpu"))      # (collectives: every rank takes part)
    if rank == 0:
        rows = tsv.splitlines()
        print(json.dumps({"metric": "exchange only (no kernels): pass-1 histogram all-reduce + finalize + broadcast, counters all-reduce",
                          "n_gpus": world, "backend": (args.backend or ("nccl" if on_gpu else "gloo")) if world > 1 else "none",
                          "collective": coll,
                          "device": str(dev), "keys": n_keys, "used_list": int(k.size), "same_used_list_on_all_ranks": same,
                          "scaling": "strong" if args.total_reads > 0 else "weak", "total_reads": args.total_reads,
                          "hist_sum": int(hist.sum().item()), "used_list_digest": digest & 0x7FFFFFFFFFFFFFFF,
                          "exchange_ms": t_ex * 1e3, "assigned_rows": len(rows) - 1,
                          "first_row_total": int(rows[1].split("\t")[1].replace(",", "")) if len(rows) > 1 else 0}))
    if dist is not None:
        dist.destroy_process_group()


def two_pass_leg(pkg, synth, dev, dist, rank, world, wl, used, n, max_ed=1):
    """The default two-pass flow of scanfastq on `n` reads per rank, with the path's one exchange on the GPUs:
    pass 1 (FASTQ text -> K-FQ, K-PACK, K-SCAN<22> + quality filter, K-HIST on the whole whitelist) -> all-reduce of the dense
    histogram (RCCL) -> host finalize (filter / collision merge / rank) -> broadcast -> pass 2 on the used list through the native
    chunk worker -> per-(barcode, ed) counters all-reduced -> BarcodesAssigned.tsv.  Not part of `value`."""
    scanfastq = importlib.import_module(graft.PKG_NAME + ".scanfastq")
    distributed = importlib.import_module(graft.PKG_NAME + ".distributed")
    ctx2 = pkg.Context(dev.index)
    keys = np.sort(wl.cpu().numpy().astype(np.uint64))
    rd = synth.gen_reads(n, used, seed=5000 + rank, device=dev, q_mean=20.0)
    text_d, _buf, _offs = synth.fastq_text_device(rd)
    text = text_d.cpu().numpy().tobytes()
    del rd, text_d, _buf
    ctx2.set_barcode_set(keys, mode=1)
    hist = torch.zeros(keys.size, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # pass 1 through the native chunk worker (host text in, histogram increment on the device); the reference's recordCount is the
    # number of 10,000-read chunks FastqFileReader cuts
    chunk_reads = ctx2.scanfastq_pass1_chunk(text, hist)
    n_chunks = (chunk_reads + 9_999) // 10_000
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    k, c, r = distributed.pass1_finalize(hist, keys, record_count=n_chunks)          # all-reduce (RCCL) + finalize + broadcast
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    hist2 = torch.zeros(keys.size, dtype=torch.int32, device=dev)
    hist2.copy_(hist)
    ta = time.perf_counter()
    if dist is not None:
        dist.all_reduce(hist2, op=dist.ReduceOp.SUM)                                  # the collective alone, timed once more
    torch.cuda.synchronize()
    allreduce_ms = (time.perf_counter() - ta) * 1e3
    order = np.argsort(k)
    ctx2.set_barcode_set(k, mode=0)
    t3 = time.perf_counter()
    passed, failed, info = ctx2.scanfastq_pass2_chunk(text, max_ed=max_ed, rank_keys=k[order], rank_values=r[order].astype(np.int32),
                                                      want_results=True, copy=False)
    t4 = time.perf_counter()
    bc = info["bc"]
    ok = bc["found"] == 1
    counts = np.zeros((k.size, 3), dtype=np.int32)
    np.add.at(counts, (np.searchsorted(k[order], bc["bc"][ok].astype(np.uint64)), bc["ed"][ok].astype(np.int64)), 1)
    tsv = distributed.assigned_counts_tsv(torch.from_numpy(counts).to(dev), k[order], max_ed=max_ed)
    digest = (int(np.bitwise_xor.reduce(k)) ^ int(c.sum()) ^ int(k.size)) & 0x7FFFFFFFFFFFFFFF
    same = True
    if dist is not None:
        t = torch.tensor([digest, -digest], dtype=torch.int64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        same = int(t[0].item()) == -int(t[1].item())
    rows = tsv.splitlines()
    planted = set(used.cpu().numpy().astype(np.uint64).tolist())
    out = {"reads_per_rank": n, "ranks": world, "pass1_reads": chunk_reads, "pass1_ms": (t1 - t0) * 1e3,
           "exchange_finalize_broadcast_ms": (t2 - t1) * 1e3, "allreduce_ms": allreduce_ms, "allreduce_bytes": int(keys.size * 4),
           "backend": (dist.get_backend() if dist is not None else "none (1 rank)"), "collective": collective_report(dist, dev), "used_list": int(k.size),
           "used_list_planted_frac": float(np.mean([int(x) in planted for x in k])) if k.size else 0.0,
           "same_used_list_on_all_ranks": same, "pass2_ms": (t4 - t3) * 1e3, "pass2_records_out": int(info["n_records_out"]),
           "pass2_passed": int(info["n_passed"]), "pass2_assigned": int(ok.sum()), "assigned_tsv_rows": len(rows) - 1,
           "assigned_tsv_total": sum(int(x.split("\t")[1].replace(",", "")) for x in rows[1:]),
           "note": "pass 1 through smi_scanfastq_pass1_chunk, pass 2 through smi_scanfastq_pass2_chunk (host text in, text out, chimera "
                   "splitter on); the BarcodesAssigned counters are summed over the ranks before the file is formatted"}
    ctx2.close()
    return out



def two_pass_single_process(pkg, synth, wl, used, n, n_dev, max_ed=1):
    """The two-pass flow when ONE process owns several GPUs (a JNI host): a context per GPU, a host thread per context, each GPU its own
    share of the reads; the pass-1 histograms are summed in place by smi_hist_allreduce (RCCL over xGMI, communicators cached in the
    library), every context then loads the same used list."""
    import threading

    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    keys = np.sort(wl.cpu().numpy().astype(np.uint64))
    ctxs, texts, hists = [], [], []
    for d in range(n_dev):
        dv = torch.device("cuda", d)
        rd = synth.gen_reads(n, used.to(dv), seed=5000 + d, device=dv, q_mean=20.0)
        texts.append(synth.fastq_text_device(rd)[0].cpu().numpy())
        del rd
        c = pkg.Context(d)
        c.set_barcode_set(keys, mode=1)
        ctxs.append(c)
        hists.append(torch.zeros(keys.size, dtype=torch.int32, device=dv))
    for d in range(n_dev):
        torch.cuda.synchronize(d)
    reads = [0] * n_dev

    def p1(d):
        reads[d] = ctxs[d].scanfastq_pass1_chunk(texts[d], hists[d], packed=True, n_threads=4)

    def run_all(fn):
        th = [threading.Thread(target=fn, args=(d,)) for d in range(n_dev)]
        for t in th:
            t.start()
        for t in th:
            t.join()

    t0 = time.perf_counter()
    run_all(p1)
    t1 = time.perf_counter()
    lib.hist_allreduce(ctxs, hists)                       # the one exchange of the path, inside the library
    t2 = time.perf_counter()
    lib.hist_allreduce(ctxs, hists)                       # once more: the communicators are cached now (the counts double; undone below)
    t3 = time.perf_counter()
    h = hists[0].cpu().numpy() // 2
    nz = np.nonzero(h)[0]
    record_count = sum((r + 9_999) // 10_000 for r in reads)
    k, c, r = lib.finalize_used_list(keys[nz], h[nz].astype(np.uint32), record_count, max_ed, 10, 500)
    order = np.argsort(k)
    for cx in ctxs:
        cx.set_barcode_set(k, mode=0)
    passed = [0] * n_dev

    def p2(d):
        _p, _f, info = ctxs[d].scanfastq_pass2_chunk(texts[d], max_ed=max_ed, rank_keys=k[order], rank_values=r[order].astype(np.int32), copy=False, packed=True,
                                                     n_threads=4)
        passed[d] = int(info["n_passed"])

    t4 = time.perf_counter()
    run_all(p2)
    t5 = time.perf_counter()
    same = all(bool((hh.cpu() == hists[0].cpu()).all()) for hh in hists)
    lib.hist_allreduce_release()
    for cx in ctxs:
        cx.close()
    return {"gpus_in_one_process": n_dev, "reads_per_gpu": n, "pass1_ms": (t1 - t0) * 1e3, "smi_hist_allreduce_first_ms": (t2 - t1) * 1e3,
            "smi_hist_allreduce_cached_ms": (t3 - t2) * 1e3, "allreduce_bytes": int(keys.size * 4), "same_histogram_on_every_gpu": same,
            "used_list": int(k.size), "pass2_ms": (t5 - t4) * 1e3, "pass2_passed": int(sum(passed))}


def config2(args, dist, rank, local_rank, world, dev):
    """BASELINE configs[2]: ed <= 2, default two-pass flow, --reads reads per GPU streamed through HBM-resident batches of --batch.
    A step = pass 1 over every batch (K-SCAN<22> with qualities + K-HIST on the 3.6 M whitelist) -> histogram all-reduce + finalize
    -> pass 2 over every batch (K-SCAN<10> + K-BC2 on the used list).  Inputs (packed read ends + quality tails) are generated once
    and stay resident; `roofline` describes K-BC2."""
    pkg = graft.load_package()
    synth = importlib.import_module(graft.PKG_NAME + ".synth")
    distributed = importlib.import_module(graft.PKG_NAME + ".distributed")
    ctx1, ctx2 = pkg.Context(local_rank), pkg.Context(local_rank)
    n, B = args.reads, min(args.batch, args.reads)
    wl = synth.make_whitelist(args.whitelist, seed=1, device=dev)
    used = synth.pick_used(wl, args.cells, seed=2)
    keys = np.sort(wl.cpu().numpy().astype(np.uint64))
    ctx1.set_barcode_set_device(wl.to(torch.int32), mode=1)
    batches = []
    for b0 in range(0, n, B):
        m = min(B, n - b0)
        ends = torch.empty((28, 2 * m), dtype=torch.int32, device=dev)
        lens = torch.empty(m, dtype=torch.int32, device=dev)
        qt = torch.empty((m, 224), dtype=torch.uint8, device=dev)
        qs = torch.empty(m, dtype=torch.int32, device=dev)
        for c0 in range(0, m, 1_000_000):
            k = min(1_000_000, m - c0)
            rd = synth.gen_reads(k, used, seed=3000 + 97 * rank + (b0 + c0) // 1_000_000, device=dev, q_mean=20.0)
            ends[:, 2 * c0:2 * (c0 + k)] = synth.pack_ends(rd["head"], rd["tail"])
            lens[c0:c0 + k] = (2 * synth.END_BASES + rd["mid_len"]).to(torch.int32)
            qt[c0:c0 + k] = rd["qtail"]
            qs[c0:c0 + k] = (rd["qhead"].to(torch.int32) - 33).sum(1) + (rd["qtail"].to(torch.int32) - 33).sum(1) + \
                (rd["qmid"].to(torch.int32) - 33) * rd["mid_len"].to(torch.int32)
            del rd
        batches.append((m, ends, lens, qt, qs))
    cfg_p1, cfg_p2 = ctx1.scan_config(1), ctx2.scan_config(2)
    Bmax = max(b[0] for b in batches)
    scan = torch.zeros((Bmax, 8), dtype=torch.int32, device=dev)
    win = torch.zeros((Bmax, 2), dtype=torch.int64, device=dev)
    out = torch.zeros((Bmax, 4), dtype=torch.int32, device=dev)
    hist = torch.zeros(keys.size, dtype=torch.int32, device=dev)
    state = {}
    dump = None
    if args.dump_outputs and rank == 0:
        # the pass-2 buffers are reused batch by batch: the last timed step gathers the sampled reads of each batch as it goes
        rows = dump_rows(n)
        dump = {"rows": rows, "idx": [torch.from_numpy(rows[(rows >= b0) & (rows < b0 + B)] - b0).to(dev) for b0 in range(0, n, B)]}

    def step(timed, keep=None):
        hist.zero_()
        for m, ends, lens, qt, qs in batches:
            ctx1.scan_device(ends, lens, m, cfg_p1, scan, win, qt, qs)
            ctx1.hist_windows_device(win, scan, m, hist)
        k, c, r = distributed.pass1_finalize(hist, keys, record_count=(n + 9_999) // 10_000)
        ctx2.set_barcode_set(k, mode=0)
        n_assigned, ms_bc2, ms_scan = 0, 0.0, 0.0
        for j, (m, ends, lens, qt, qs) in enumerate(batches):
            ctx2.scan_device(ends, lens, m, cfg_p2, scan, win)
            ctx2.bc_match_device(win, out, m, max_ed=2, five_prime=False)
            if timed:
                ms_scan += ctx2.kernel_ms(ctx2.K_SCAN)
                ms_bc2 += ctx2.kernel_ms(ctx2.K_BC_MATCH)
            if keep is not None:
                for name, t in (("scan", scan), ("win", win), ("out", out)):
                    keep.setdefault(name, []).append(t.index_select(0, keep["idx"][j]))
            n_assigned += int(((out[:m, 2] & 0xFF) == 1).sum().item())
        if keep is not None:
            keep.update(used_keys=k, used_counts=c, used_ranks=r)
        state.update(used=int(k.size), assigned=n_assigned, ms_bc2=ms_bc2, ms_scan=ms_scan)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step(False)
    barrier()
    ctx2.set_timing(True)
    t0 = time.perf_counter()
    bc2_ms = []
    for s in range(args.steps):
        step(True, keep=dump if s == args.steps - 1 else None)
        bc2_ms.append(state["ms_bc2"])
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        dist.destroy_process_group()
    if rank != 0:
        return
    if dump is not None:
        dump_outputs(args.dump_outputs, dump["rows"], torch.cat(dump["scan"]), torch.cat(dump["win"]), torch.cat(dump["out"]),
                     extra={"used_keys": dump["used_keys"], "used_counts": dump["used_counts"], "used_ranks": dump["used_ranks"]})
    k_bc2 = float(np.mean(bc2_ms))
    rf = roofline_entry("k_bc_match_ed2", "k_bc_match_ed2", k_bc2, ALG_BYTES_PER_READ_BC2, n, pmc_table())
    rf.update({"bound": "instruction issue (round 6: seven waves per SIMD; VALU + SALU fill the SIMD cycles, `valu_issue` has the vector share; `frac` is the counter "
                        "traffic over the HBM peak, as the contract asks)",
               "launches_per_step": len(batches),
               "note": "SURVEY 8d prices a read at ~56,000 probes x 4 B; against a short used list K-BC2 dismisses ~98 % of the level-1 items with one "
                       "load each (the inverse one-step neighbourhood of the list, P.n1) and never enumerates their children, so the algorithmic "
                       "figure (in `algorithmic`) exceeds the HBM peak: it measures probes answered, not bytes moved",
               "limiter": "1,672 VALU + 1,081 SALU wave instructions per read (per-offset set-up: children, filter bits, LDS dedup table, creation order; the scalar "
                          "bit loops) at ~ 97 % of the SIMD cycles; 0.5 G L2 misses per 10 M reads (profiles/r06/cfg2_pmc.json)",
               "kernels_ms": {"k_bc_match_ed2": k_bc2, "k_scan<10>": state["ms_scan"]}})
    print(json.dumps({
        "metric": "Nanopore reads/sec BC-assigned at ed<=2, two-pass (whitelist-build + assign), 3.6M whitelist",
        "value": n * world * args.steps / elapsed, "unit": "reads/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32",
        "data": f"synthetic ({synth.GENERATOR_VERSION}, seeds wl=1 used=2 reads=3000+97*rank+chunk), packed read ends + quality tails resident in HBM",
        "config": {"workload": "configs[2]: ed<=2, two-pass: pass 1 = K-SCAN<22> + quality filter + K-HIST on the 3.6M whitelist, "
                               "histogram all-reduce + host finalize, pass 2 = K-SCAN<10> + K-BC2 on the used list; not in the step: FASTQ "
                               "decode/packing, chimera split, writer",
                   "reads_per_gpu": n, "batch": B, "whitelist": int(wl.numel()), "cells": args.cells, "used_list": state["used"],
                   "bc_assigned_frac": state["assigned"] / n},
        "roofline": rf}))


def config4(args, dist, rank, local_rank, world, dev):
    """BASELINE configs[4]: 5' protocol with --noPolyARequired (scanfastq -h -y), the 737K-august-2016 whitelist size (737,280 keys) as the
    search set, ed <= 1, plus the UMI stage: per-(cell, region) UMI edit distances (K-UMI) and clustering (host, smi_umi_cluster_groups).
    A step = pass 2 per read from packed read ends in HBM (K-SCAN in its 5' mode + K-BC1 on 5' windows); the UMI leg is timed beside it
    on synthetic (cell, region) groups, as in tools/microbench.py (it runs on aligned reads, i.e. behind an external aligner)."""
    pkg = graft.load_package()
    synth = importlib.import_module(graft.PKG_NAME + ".synth")
    ctx = pkg.Context(local_rank)
    n = args.reads
    wl = synth.make_whitelist(737_280, seed=401, device=dev)
    used = synth.pick_used(wl, args.cells, seed=402)
    ctx.set_barcode_set_device(wl.to(torch.int32), mode=1)
    ends = torch.empty((28, 2 * n), dtype=torch.int32, device=dev)
    lens = torch.empty(n, dtype=torch.int32, device=dev)
    truth = torch.empty(n, dtype=torch.int64, device=dev)
    chunk = 1_000_000
    for c0 in range(0, n, chunk):
        m = min(chunk, n - c0)
        rd = synth.gen_reads_5p(m, used, seed=4000 + 97 * rank + c0 // chunk, device=dev)
        ends[:, 2 * c0:2 * (c0 + m)] = synth.pack_ends(rd["head"], rd["tail"])
        lens[c0:c0 + m] = (2 * synth.END_BASES + rd["mid_len"]).to(torch.int32)
        truth[c0:c0 + m] = rd["truth"]
        del rd
    cfg = ctx.scan_config_5p(2, dont_search_polya=True)
    scan_out = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    win = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def step():
        ctx.scan_device(ends, lens, n, cfg, scan_out, win)
        ctx.bc_match_device(win, out, n, max_ed=1, five_prime=True)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    ctx.set_timing(True)
    scan_ms, match_ms = [], []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
        scan_ms.append(ctx.kernel_ms(ctx.K_SCAN))
        match_ms.append(ctx.kernel_ms(ctx.K_BC_MATCH))
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ctx.set_timing(False)
    if args.dump_outputs and rank == 0:
        rows = dump_rows(n)
        idx = torch.from_numpy(rows).to(dev)
        dump_outputs(args.dump_outputs, rows, scan_out.index_select(0, idx), win.index_select(0, idx), out.index_select(0, idx))
    found = (out[:, 2] & 0xFF) == 1
    n_found = int(found.sum().item())
    acc = float(((out[:, 0].to(torch.int64) & 0xFFFFFFFF)[found] == truth[found]).float().mean().item())
    # ---- UMI leg: Zipf-sized (cell, region) groups, K-UMI on the device, clustering on the host --------------------------------
    rng = np.random.default_rng(1 + rank)
    sizes = np.minimum(rng.zipf(1.6, 200_000), 400).astype(np.int64) + 1
    go, po, mo = ctx.umi_offsets(sizes)
    n_umi = int(go[-1])
    w = torch.randint(0, 4, (n_umi, 14), device=dev)
    packed = (torch.tensor([1, 2, 4, 8], device=dev)[w] << (4 * torch.arange(14, device=dev))).sum(1)
    d_go, d_po, d_mo = (torch.from_numpy(a.view(np.int32 if a is go else np.int64)).to(dev) for a in (go, po, mo))
    d_dist = torch.zeros(int(mo[-1]), dtype=torch.uint8, device=dev)
    ctx.umi_dist_device(packed, d_go, d_po, d_mo, len(sizes), int(po[-1]), d_dist)
    torch.cuda.synchronize()
    tu = time.perf_counter()
    ctx.umi_dist_device(packed, d_go, d_po, d_mo, len(sizes), int(po[-1]), d_dist)
    torch.cuda.synchronize()
    umi_ms = (time.perf_counter() - tu) * 1e3
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return
    k_scan, k_match = float(np.mean(scan_ms)), float(np.mean(match_ms))
    dom_name, dom_ms, alg = ("k_scan<10, 5'>", k_scan, ALG_BYTES_PER_READ_SCAN) if k_scan >= k_match else ("k_bc_match_ed1 (5')", k_match, ALG_BYTES_PER_READ_BC1)
    ach = alg * n / (dom_ms * 1e-3) / 1e9
    print(json.dumps({
        "metric": "Nanopore reads/sec BC-assigned at ed<=1, 5' protocol --noPolyARequired, 737K whitelist", "value": n * world * args.steps / elapsed,
        "unit": "reads/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32",
        "data": f"synthetic ({synth.GENERATOR_VERSION}, 5' reads, seeds wl=401 used=402 reads=4000+97*rank+chunk), packed read ends resident in HBM",
        "config": {"workload": "configs[4]: 5' protocol, --noPolyARequired, ed<=1 vs the 737,280-key whitelist (-g semantics); timed = pass 2 per read "
                               "from packed read ends in HBM (K-SCAN 5' mode + K-BC1 on 5' windows); the UMI stage (K-UMI + clustering) beside it in `umi`",
                   "reads_per_gpu": n, "whitelist": int(wl.numel()), "cells": args.cells, "bc_assigned_frac": n_found / n, "bc_assigned_accuracy": acc},
        "roofline": {"bound": "hbm" if dom_name.startswith("k_bc") else "valu-issue (HBM figures as the contract asks)", "kernel": dom_name, "kernel_ms": dom_ms,
                     "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "alg_bytes_per_read": alg, "traffic": None,
                     "kernels_ms": {"k_scan<10, 5'>": k_scan, "k_bc_match_ed1 (5')": k_match}},
        "umi": {"groups": int(len(sizes)), "reads": n_umi, "pairs": int(po[-1]), "k_umi_ms": umi_ms, "pairs_per_s": int(po[-1]) / (umi_ms * 1e-3),
                "levenshtein_per_s": 9 * int(po[-1]) / (umi_ms * 1e-3),
                "note": "K-UMI over Zipf-sized (cell, region) groups; clustering and the BAM side: tools/microbench.py assignumis (5.4 M records/s per chunk call)"}}))
    if dist is not None:
        dist.destroy_process_group()


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))          # nothing above has touched the GPU; the ranks are children, never an exec
    if args.exchange_only:
        return exchange_only(args)
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible (the hot path has no CPU fallback)", file=sys.stderr)
        sys.exit(2)
    if os.environ.get("SMI_BENCH_SHARE_GPU"):
        # rehearsal of the N-rank launch on a box with fewer GPUs than ranks (use with --backend gloo: RCCL refuses two ranks on one
        # device): rank r runs on device r mod device_count.  Not a measurement mode.
        os.environ["LOCAL_RANK"] = str(int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist, rank, local_rank, world = init_dist(args, dev)
    if args.config == 2:
        return config2(args, dist, rank, local_rank, world, dev)
    if args.config == 4:
        return config4(args, dist, rank, local_rank, world, dev)

    pkg = graft.load_package()
    synth = importlib.import_module(graft.PKG_NAME + ".synth")
    ctx = pkg.Context(local_rank)

    # ---- inputs (synthetic, seeded; built on the device in chunks, resident in HBM before the timed region) ----
    chunk = 1_000_000
    strong = args.total_reads > 0
    if strong:
        # strong scaling (configs[3]): --total-reads in all, cut into 1 M-read chunks whose seeds are GLOBAL, dealt to the ranks in
        # contiguous runs (distributed.shard_range): every world size processes exactly the same reads
        distributed = importlib.import_module(graft.PKG_NAME + ".distributed")
        n_chunks_all = (args.total_reads + chunk - 1) // chunk
        c_lo, c_hi = distributed.shard_range(n_chunks_all, rank, world)
        chunk_ids = list(range(c_lo, c_hi))
        chunk_sizes = [min(chunk, args.total_reads - c * chunk) for c in chunk_ids]
        seed_of = lambda c: 1000 + c                                                  # noqa: E731
    else:
        chunk_ids = list(range((args.reads + chunk - 1) // chunk))
        chunk_sizes = [min(chunk, args.reads - c * chunk) for c in chunk_ids]
        seed_of = lambda c: 1000 + 97 * rank + c                                      # noqa: E731  (weak scaling: each rank its own reads)
    n = int(sum(chunk_sizes))
    wl = synth.make_whitelist(args.whitelist, seed=1, device=dev)           # same list on every rank
    used = synth.pick_used(wl, args.cells, seed=2)
    ctx.set_barcode_set_device(wl.to(torch.int32), mode=1)                   # -g semantics: search set = whole list
    set_cold = ctx.set_stats()                                                # the first build of the process: with the allocation of its 18.5 GB
    if args.full:
        ctx.set_barcode_set_device(wl.to(torch.int32), mode=1)               # ... and once more into the structures that now exist
        set_warm = ctx.set_stats()
    ends = torch.empty((28, 2 * max(n, 1)), dtype=torch.int32, device=dev)   # packed read ends (bit-planes)
    lens = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    truth = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    cpu_reads = None
    c0 = 0
    for cid, m in zip(chunk_ids, chunk_sizes):
        rd = synth.gen_reads(m, used, seed=seed_of(cid), device=dev)
        if args.pack_kernel:
            ascii_, offs_ = synth.materialize_device(rd, seed=seed_of(cid))
            e_ = torch.zeros((28, 2 * m), dtype=torch.int32, device=dev)
            l_ = torch.zeros(m, dtype=torch.int32, device=dev)
            ctx.pack_ends_device(ascii_, None, offs_, m, e_, l_)
            torch.cuda.synchronize()
            ends[:, 2 * c0:2 * (c0 + m)] = e_
            lens[c0:c0 + m] = l_
            del ascii_, offs_, e_, l_
        else:
            ends[:, 2 * c0:2 * (c0 + m)] = synth.pack_ends(rd["head"], rd["tail"])
            lens[c0:c0 + m] = (2 * synth.END_BASES + rd["mid_len"]).to(torch.int32)
        truth[c0:c0 + m] = rd["truth"]
        if c0 == 0 and rank == 0 and args.full and not args.no_cpu_baseline:
            k = min(args.cpu_sample, m)
            cpu_reads = {key: (v[:k].cpu() if torch.is_tensor(v) else v) for key, v in rd.items()}
        del rd
        c0 += m
    scan_cfg = ctx.scan_config(2)
    scan_out = torch.zeros((max(n, 1), 8), dtype=torch.int32, device=dev)
    win = torch.zeros((max(n, 1), 2), dtype=torch.int64, device=dev)
    out = torch.zeros((max(n, 1), 4), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def step():
        # pass 2 of scanfastq for one batch: polyA/adapter scan -> barcode windows -> ed<=1 match + best/second rule
        if n:
            ctx.scan_device(ends, lens, n, scan_cfg, scan_out, win)
            ctx.bc_match_device(win, out, n, max_ed=1, five_prime=False)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    scan_ms, match_ms = [], []
    if args.overlap and n:
        # the same steps as a two-stage pipeline: K-SCAN of step k + 1 on one stream while K-BC1 of step k runs on another (two window
        # buffers, events between the stages).  Kernel durations: events around each launch on its own stream, read after the loop
        s_scan, s_bc = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        wins = [win, torch.zeros_like(win)]
        scanned = [torch.cuda.Event() for _ in range(2)]
        matched = [None, None]
        marks = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.steps):
            b = k & 1
            with torch.cuda.stream(s_scan):
                if matched[b] is not None:
                    s_scan.wait_event(matched[b])            # K-BC1 of step k - 2 has read this window buffer
                a0, a1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a0.record()
                ctx.scan_device(ends, lens, n, scan_cfg, scan_out, wins[b])
                a1.record()
                scanned[b] = a1
            with torch.cuda.stream(s_bc):
                s_bc.wait_event(scanned[b])
                b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                b0.record()
                ctx.bc_match_device(wins[b], out, n, max_ed=1, five_prime=False)
                b1.record()
                matched[b] = b1
            marks.append((a0, a1, b0, b1))
        barrier()
        t1 = time.perf_counter()
        scan_ms = [a0.elapsed_time(a1) for a0, a1, _, _ in marks]
        match_ms = [b0.elapsed_time(b1) for _, _, b0, b1 in marks]
        win = wins[(args.steps - 1) & 1]             # the window buffer of the last step
    else:
        ctx.set_timing(True)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
            # HIP events were recorded on the launch stream around each kernel; reading them waits for this step's
            # kernels (one sync per step inside the timed region -- conservative)
            if n:
                scan_ms.append(ctx.kernel_ms(ctx.K_SCAN))
                match_ms.append(ctx.kernel_ms(ctx.K_BC_MATCH))
        barrier()
        t1 = time.perf_counter()
    elapsed = t1 - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ctx.set_timing(False)
    if args.dump_outputs and rank == 0:
        rows = dump_rows(n)
        idx = torch.from_numpy(rows).to(dev)
        dump_outputs(args.dump_outputs, rows, scan_out.index_select(0, idx), win.index_select(0, idx), out.index_select(0, idx))

    found = (out[:n, 2] & 0xFF) == 1
    n_found = int(found.sum().item())
    acc = float(((out[:n, 0].to(torch.int64) & 0xFFFFFFFF)[found] == truth[:n][found]).float().mean().item()) if n_found else 0.0
    n_all, found_all = n * world, n_found
    if dist is not None:
        # job-wide counts (outside the timed region): reads in all (strong scaling: the shards differ by at most one chunk) and assigned reads
        t = torch.tensor([n, n_found], dtype=torch.int64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        n_all, found_all = int(t[0].item()), int(t[1].item())
    elif strong:
        n_all = n

    two_pass = None
    if args.full and args.two_pass_reads > 0:
        two_pass = two_pass_leg(pkg, synth, dev, dist, rank, world, wl, used, args.two_pass_reads)   # collective: every rank takes part

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    ms_per_step = elapsed / args.steps * 1e3
    value = n_all * args.steps / elapsed
    k_scan, k_match = float(np.mean(scan_ms)), float(np.mean(match_ms))
    # dominant kernel = the longer of the two.  K-SCAN (bit-parallel gates + Needleman-Wunsch cells on packed read ends) is
    # bound by integer VALU issue, a bound the contract's enum has no name for: its HBM figures are reported as asked
    # (algorithmic bytes) and the issue-rate figure beside them; K-BC1, the memory-side kernel the
    # metric is named after, is in `roofline.other` with the same fields.
    tj = pmc_table()
    f_scan = roofline_entry("k_scan<10>", "k_scan", k_scan, ALG_BYTES_PER_READ_SCAN, n, tj)
    f_bc1 = roofline_entry("k_bc_match_ed1<1> (k_bc_codes_ed1t + k_bc_pick_ed1t)", "k_bc_match_ed1", k_match, ALG_BYTES_PER_READ_BC1, n, tj)
    f_scan["limiter"] = "integer VALU issue (bit-parallel gates, Needleman-Wunsch cells): not hbm, not mfma"
    f_bc1["limiter"] = ("dependent gathers into the offset filter and the neighbourhood table (L2 / Infinity Cache / HBM request rate) together with "
                        "integer VALU issue (the keys, the bucket's eight entries): since round 5's layout neither alone")
    f_bc1["note"] = ("SURVEY 8d prices a read at 620 probes x 4 B; K-BC1 asks an exact bitmap of the set's inverse one-step neighbourhood once per "
                     "offset -- laid out by the 12 bases the five windows of a read share (P.nb5, 2.5 GiB), so the five bits of a read are three "
                     "64-byte sectors instead of five -- and, where a barcode is in reach (1.6 of 5 offsets per read against the 3.6 M list), reads "
                     "the matching mutation steps off one bucket of a table of that neighbourhood (P.nt, three slots per entry: a second bucket "
                     "is rare) instead of making the 124 probes: the algorithmic figure counts probes answered, not bytes moved, so `frac` is "
                     "the counter traffic over the HBM peak")
    probe = hbm_probe(dev) if args.full and world == 1 else None
    if probe and "gather_512MiB_G_per_s" in probe and tj and "k_bc_match_ed1" in tj and tj["k_bc_match_ed1"].get("l2_misses_per_launch"):
        # K-BC1 against what random sector reads can reach on this GPU: its L2 misses per second beside the measured gather rates
        miss_rate = tj["k_bc_match_ed1"]["l2_misses_per_launch"] * (n / tj["k_bc_match_ed1"]["reads_per_launch"]) / (k_match * 1e-3) / 1e9
        f_bc1["random_access"] = {"l2_misses_G_per_s": miss_rate, "measured_gather_512MiB_G_per_s": probe["gather_512MiB_G_per_s"],
                                  "measured_gather_8GiB_G_per_s": probe["gather_8GiB_G_per_s"],
                                  "frac_of_512MiB_gather_rate": miss_rate / probe["gather_512MiB_G_per_s"]}
    dom, oth = (f_scan, f_bc1) if k_scan >= k_match else (f_bc1, f_scan)
    n_adapter = int(((scan_out[:n, 6] >> 16) & 0xFF).eq(1).sum().item())
    res = {
        "metric": "Nanopore reads/sec BC+UMI-assigned at ed<=1, 3.6M whitelist; % HBM roofline",
        "metric_note": "`value` = the barcode-assignment step (pass 2 per read: K-SCAN + K-BC1) over the batch, inputs resident in HBM; the UMI "
                       "stage of the same metric runs on ALIGNED reads, i.e. behind an external aligner, and is measured on names from a real "
                       "pass 2 of the same generator in `umi_stage` (records/s, PCIe and host region grouping included); `value_bc_umi` = reads/s "
                       "when every assigned read of a batch then goes through that stage: reads / (t_step + assigned reads / umi_stage rate)",
        "value": value,
        "unit": "reads/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_per_step,
        "higher_is_better": True,
        "scaling": "strong" if strong else "weak",
        "vs_baseline": None,
        "dtype": "u32",
        "data": f"synthetic ({synth.GENERATOR_VERSION}, seeds wl=1 used=2 reads={'1000+global chunk' if strong else '1000+97*rank+chunk'}, "
                "err=6.3% 40/30/30 sub/ins/del, 50% reverse strand, read length 448..1948)",
        "config": {
            "workload": ("configs[3]: %d synthetic Nanopore reads in all, sharded over the GPUs (strong scaling), " % args.total_reads if strong else
                         "configs[1]: 10M synthetic Nanopore reads, ") +
                        "ed<=1 vs 3.6M whitelist (-g semantics), 3' protocol; "
                        "timed = pass 2 per read from packed read ends in HBM: polyA/T finder + k-mer gated NW adapter scan "
                        "+ TSO scan + strand decision (K-SCAN) -> 5-offset barcode match + best/second rule (K-BC1); "
                        "beside the step: FASTQ ingest / planes / writer (end_to_end, host_to_host, file_to_file), chimera split, UMI stage (umi_stage)",
            "reads_per_gpu": n,
            "reads_total": n_all,
            "whitelist": int(wl.numel()),
            "cells": args.cells,
            "adapter_found_frac": n_adapter / max(n, 1),
            "bc_assigned_frac": n_found / max(n, 1),
            "bc_assigned_accuracy": acc,
            "bc_assigned_total": found_all,
            "ends_packed_by": "K-PACK (smi_pack_ends_device) from ASCII reads" if args.pack_kernel else "the generator's torch packer (same bit-planes; --pack-kernel uses K-PACK)",
        },
        "roofline": dict({"bound": "hbm" if dom is f_bc1 else "valu-issue (the HBM figures are what the contract asks for; the binding resource "
                                   "of this kernel is integer VALU issue, in `valu_issue`)"}, **dom,
                         **{"kernels_ms": {"k_scan<10>": k_scan, "k_bc_match_ed1<1>": k_match}, "other": {oth["kernel"]: oth},
                            "kernel_trace": "profiles/r06/step_kernel_stats.csv (rocprofv3 --kernel-trace --stats of `bench.py --steps 5` with every side "
                                            "leg off: AverageNs of k_scan<10> is kernel_ms)",
                            "probes_per_s_bc1": 620.0 * n / (k_match * 1e-3)}),
    }
    # The one-time cost behind K-BC1: the pyramid, the offset filter nb / nb5 and the neighbourhood table nt of the WHOLE list are built
    # once per job (-g semantics; the default two-pass flow loads the list as membership only, ~10 ms, and builds these for the used list, a few ms).
    # `value` repeats the step on resident structures; `value_one_shot` is the same batch as a job of its own: build (with its allocations) + one step.
    if args.full:
        res["set_build_ms"] = set_warm["build_ms"]
        res["set_build_cold_ms"] = set_cold["build_ms"]
        res["set_hbm_bytes"] = set_warm["hbm_bytes"]
        res["value_one_shot"] = n * world / (set_cold["build_ms"] * 1e-3 + ms_per_step * 1e-3)
        res["value_one_shot_warm_allocator"] = n * world / (set_warm["build_ms"] * 1e-3 + ms_per_step * 1e-3)   # (a second job of the same process: no hipMalloc)
        res["set_build_note"] = ("smi_set_barcode_set_device of the 3.6 M list: membership pyramid + nb (512 MiB, atomics) + nb5 (2.5 GiB, transposed from nb) on a "
                                 "side stream beside nt (3 slots per neighbour + bucket counters); profiles/r06/set_build_kernel_stats.csv has the kernels; "
                                 "set_build_cold_ms includes hipMalloc of set_hbm_bytes")
    if probe:
        res["hbm_measured"] = probe
    if two_pass is not None:
        res["two_pass"] = two_pass
    if args.full and world == 1 and args.single_process_gpus > 0:
        res["two_pass_single_process"] = two_pass_single_process(pkg, synth, wl, used, max(args.two_pass_reads, 50_000),
                                                                 min(args.single_process_gpus, torch.cuda.device_count()))
    if args.full and world == 1 and args.e2e_reads > 0:
        res["end_to_end"] = end_to_end_leg(ctx, synth, dev, used, args.e2e_reads, lane_counts=tuple(int(x) for x in args.e2e_lanes.split(",")))
        # the number that corresponds to "pass 2" as the reference runs it: FASTQ text in HBM -> passed / failed text in HBM,
        # chimera splitter, K-PACK and the writer included (beside `value`, never part of it)
        # (advisor, round 5: `reads_per_s` is the ONE-LANE figure again -- the one earlier rounds reported and `ms` belongs to; the run on several worker
        # lanes is `reads_per_s_best_lanes` / `value_full_pass2_lanes`, with `lanes_at_best`)
        res["value_full_pass2"] = res["end_to_end"]["reads_per_s"]
        res["value_full_pass2_lanes"] = res["end_to_end"]["reads_per_s_best_lanes"]
    if args.full and world == 1 and args.umi_molecules > 0:
        res["umi_stage"] = umi_stage_leg(pkg, synth, ctx, used, args.umi_molecules)
        r_umi = res["umi_stage"]["records_per_s"]
        res["value_bc_umi"] = n / (ms_per_step * 1e-3 + n_found / r_umi)
        if args.assignumis_file_records > 0:
            rows = umi_stage_leg.rows[:args.assignumis_file_records]
            res["assignumis_file_to_file"] = assignumis_file_leg(pkg, synth, ctx, rows, n_threads=16)
    if args.full and world == 1 and args.h2h_reads > 0:
        res["host_to_host"] = host_to_host_leg(pkg, synth, ctx, dev, used, args.h2h_reads)
        res["value_host_to_host"] = res["host_to_host"]["reads_per_s"]
    if args.full and world == 1 and args.f2f_reads > 0:
        res["file_to_file"] = file_to_file_leg(pkg, synth, ctx, dev, wl, used, args.f2f_reads, scratch=args.f2f_dir)
    if args.full and world == 1 and not args.no_cpu_baseline:
        sor = graft.load_oracle()
        sor.build()
        cores = host_cpu_quota()     # OpenMP threads = the CPUs the cgroup grants (the box shows 256, the pool grants 16)
        bset = sor.BarcodeSet(wl.cpu().numpy())
        m = int(cpu_reads["head"].shape[0])
        seqs, quals = zip(*(synth.materialize(cpu_reads, i) for i in range(m)))
        offs = np.zeros(m + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(s_) for s_ in seqs])
        ra = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
        t0 = time.perf_counter()
        st, sc = sor.scan_batch_3p(ra, None, offs, synth.ADAPTER_3P_SHORT, n_threads=cores)
        dt_scan = time.perf_counter() - t0
        # stranded barcode regions for assignBarcode: reuse the oracle on windows cut out of the stranded read
        codes = np.full((m, 64), 4, dtype=np.uint8)
        ae = np.zeros(m, dtype=np.int32)
        lut = np.full(256, 4, dtype=np.uint8)
        for ch, v in ((b"A", 0), (b"G", 1), (b"C", 2), (b"T", 3)):
            lut[ch[0]] = v
        comp = bytes.maketrans(b"ACGTN", b"TGCAN")
        for i in range(m):
            if not sc["adapter_found"][i]:
                continue
            seq = bytes(ra[int(offs[i]):int(offs[i + 1])])
            stranded = seq.translate(comp)[::-1] if sc["reverse"][i] else seq
            a = int(sc["adapter_end"][i])
            lo = max(a - 30, 0)
            seg = np.frombuffer(stranded[lo:a + 2], dtype=np.uint8)
            codes[i, :seg.size] = lut[seg]
            ae[i] = a - lo
        t1 = time.perf_counter()
        st2, exp = sor.assign_batch(bset, codes, ae, max_ed=1, n_threads=cores)
        dt = dt_scan + (time.perf_counter() - t1)   # the two OpenMP oracle calls only; the Python loop that cuts the windows is not timed
        got = out[:m].cpu().numpy().view(pkg.BC_RESULT_DTYPE).reshape(-1)
        exp_found = np.where(sc["adapter_found"] == 1, np.where(st2 < 0, -1, exp["found"]), -1)
        same = bool((got["found"] == exp_found).all() and
                    (got["bc"][exp_found == 1] == exp["bc"][exp_found == 1].astype(np.uint32)).all())
        res["cpu_baseline"] = {
            "value": m / dt,
            "unit": "reads/s",
            "cores": cores,
            "cpus_visible": os.cpu_count(),
            "kind": "port",
            "sample": f"first {m} reads of rank 0's batch (materialised as ASCII), oracle/sor_scan.c + sor_bc.c "
                      f"(C restatement, OpenMP x{cores}; timed = the two batch calls, not the Python glue between them); the Java "
                      "reference cannot run here (no JVM); README quotes 20.8k reads/s on 96 cores for the whole scan",
            "seconds": dt,
            "matches_gpu": same,
        }
    print(json.dumps(res))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
