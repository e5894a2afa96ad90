#!/usr/bin/env python3
"""Secondary kernels' throughput on one MI355X (not the headline bench): K-BC2 (ed<=2, used-list mode),
K-SCAN pass 1 (complete adapter + quality filter) + histogram, K-UMI.  Prints one JSON object."""
import importlib
import json
import os
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def timed(fn, reps=3):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    only = sys.argv[1] if len(sys.argv) > 1 else None  # e.g. "chimera": just that leg
    pkg = graft.load_package()
    synth = importlib.import_module(graft.PKG_NAME + ".synth")
    dev = torch.device("cuda:0")
    ctx = pkg.Context(0)
    res = {}
    wl = synth.make_whitelist(3_600_000, seed=1, device=dev)
    used = synth.pick_used(wl, 5000, seed=2)
    legs = {"bc2": leg_bc2, "bc": leg_bc, "pass1": leg_pass1, "umi": leg_umi, "chimera": leg_chimera, "fastq": leg_fastq, "assignumis": leg_assignumis,
            "packed": leg_packed, "deflate": leg_deflate, "inflate": leg_inflate, "tagbam": leg_tagbam,
            "consensus": leg_consensus, "isoform": leg_isoform, "snp": leg_snp, "dedup": leg_dedup, "moltag": leg_moltag, "collapse": leg_collapse, "fusion": leg_fusion, "validator": leg_validator,
            "fusionprep": leg_fusionprep, "bamindex": leg_bamindex, "bamsort": leg_bamsort, "bamsort_runs": leg_bamsort_runs, "samview": leg_samview, "bamview": leg_bamview}
    for name, fn in legs.items():
        if only == name or (only is None and name not in ("bc2", "tagbam", "consensus", "isoform", "snp", "dedup", "moltag", "collapse", "fusion", "validator", "fusionprep", "bamindex", "bamsort", "bamsort_runs", "samview", "bamview")):
            fn(pkg, synth, ctx, dev, wl, used, res)
    print(json.dumps(res))


def leg_bc(pkg, synth, ctx, dev, wl, used, res):
    # ---- K-BC2 / K-BC1 in used-list mode -------------------------------------------------------------------
    n = 2_000_000
    reg = synth.gen_bc_region(n, used, seed=3, device=dev)
    win = synth.pack_windows(reg["codes"], reg["ae"])
    out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    ctx.set_barcode_set_device(used.to(torch.int32), mode=0)
    ctx.set_barcode_set_device(used.to(torch.int32), mode=0)          # (the second load: into structures that are allocated)
    res["used_list_5k_set"] = ctx.set_stats()
    for ed in (1, 2):
        dt = timed(lambda: ctx.bc_match_device(win, out, n, max_ed=ed))
        found = ((out[:, 2] & 0xFF) == 1)
        acc = float(((out[:, 0].to(torch.int64) & 0xFFFFFFFF)[found] == reg["truth"][found]).float().mean())
        res[f"bc_match_ed{ed}_used_list_5k"] = {"reads": n, "ms": dt * 1e3, "reads_per_s": n / dt,
                                                "assigned_frac": float(found.float().mean()), "accuracy": acc}
    ctx.set_barcode_set_device(wl.to(torch.int32), mode=1)
    dt = timed(lambda: ctx.bc_match_device(win, out, n, max_ed=2))
    res["bc_match_ed2_whitelist_3p6M"] = {"reads": n, "ms": dt * 1e3, "reads_per_s": n / dt}


def leg_bc2(pkg, synth, ctx, dev, wl, used, res):
    """K-BC2 alone against the 5 k used list (configs[2]'s dominant kernel): for counters (PROFILE_PROG=tools/microbench.py tools/profile_gpu.sh <tag> bc2)"""
    n = 2_000_000
    reg = synth.gen_bc_region(n, used, seed=3, device=dev)
    win = synth.pack_windows(reg["codes"], reg["ae"])
    out = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    ctx.set_barcode_set_device(used.to(torch.int32), mode=0)
    dt = timed(lambda: ctx.bc_match_device(win, out, n, max_ed=2))
    res["bc_match_ed2_used_list_5k"] = {"reads": n, "ms": dt * 1e3, "reads_per_s": n / dt, "set": ctx.set_stats()}


def leg_pass1(pkg, synth, ctx, dev, wl, used, res):
    # ---- pass 1: scan (22-mer) + quality filter + histogram ---------------------------------------------------
    ctx.set_barcode_set_device(wl.to(torch.int32), mode=1)
    n = 2_000_000
    rd = synth.gen_reads(n, used, seed=5, device=dev, q_mean=14.0)
    ends = synth.pack_ends(rd["head"], rd["tail"])
    lens = (2 * synth.END_BASES + rd["mid_len"]).to(torch.int32)
    qtail = rd["qtail"].contiguous()
    qsum = (rd["qhead"].to(torch.int32).sum(1) + rd["qtail"].to(torch.int32).sum(1) - 33 * 2 * synth.END_BASES +
            (rd["qmid"].to(torch.int32) - 33) * rd["mid_len"].to(torch.int32)).to(torch.int32)
    cfg1 = ctx.scan_config(1)
    so = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    win = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    hist = torch.zeros(wl.numel(), dtype=torch.int32, device=dev)

    def pass1():
        ctx.scan_device(ends, lens, n, cfg1, so, win, qtail, qsum)
        ctx.hist_windows_device(win, so, n, hist)

    dt = timed(pass1)
    res["pass1_scan22_filter_hist"] = {"reads": n, "ms": dt * 1e3, "reads_per_s": n / dt,
                                       "pass1_ok_frac": float((((so[:, 7]) & 0xFF) == 1).float().mean())}


def leg_umi(pkg, synth, ctx, dev, wl, used, res):
    # ---- K-UMI ------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(1)
    sizes = np.minimum(rng.zipf(1.6, 400_000), 400).astype(np.int64) + 1
    # SMI_UMI_DENSE=1: the dense n x n layout of smi_umi_dist_device; default: the padded rows the chunk worker gives its own matrices (round 6)
    padded = not os.environ.get("SMI_UMI_DENSE")
    go, po, mo = ctx.umi_offsets(sizes, padded=padded)
    n_reads = int(go[-1])
    w = torch.randint(0, 4, (n_reads, 14), device=dev)
    codes = torch.tensor([1, 2, 4, 8], device=dev)[w]
    packed = (codes << (4 * torch.arange(14, device=dev))).sum(1)
    d_go = torch.from_numpy(go.view(np.int32)).to(dev)
    d_po = torch.from_numpy(po.view(np.int64)).to(dev)
    d_mo = torch.from_numpy(mo.view(np.int64)).to(dev)
    d_out = torch.zeros(int(mo[-1]), dtype=torch.uint8, device=dev)
    dt = timed(lambda: ctx.umi_dist_device(packed, d_go, d_po, d_mo, len(sizes), int(po[-1]), d_out, padded=padded))
    res["umi_dist"] = {"groups": int(len(sizes)), "reads": n_reads, "pairs": int(po[-1]), "ms": dt * 1e3, "layout": "padded rows" if padded else "dense",
                       "matrix_bytes": int((sizes.astype(np.int64) ** 2).sum()), "buffer_bytes": int(mo[-1]),
                       "pairs_per_s": int(po[-1]) / dt, "levenshtein_per_s": 9 * int(po[-1]) / dt}


def leg_assignumis(pkg, synth, ctx, dev, wl, used, res):
    """the second worker end to end: smi_assignumis_chunk (names parsed as getScanDatFromReadName does, clustering positions, region
    grouping, K-UMI, UMI clustering) on one BamReader chunk.  Names come out of a real pass 2 over synthetic molecules; every molecule is
    then read `copies` times (same barcode and UMI window, an error now and then), aligned to one of `genes` loci."""
    import ctypes
    scanfastq = importlib.import_module(graft.PKG_NAME + ".scanfastq")
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    rng = np.random.default_rng(5)
    n_mol, copies, genes = 20_000, 6, 2_000
    ctx.set_barcode_set(used.cpu().numpy().astype(np.uint64), mode=0)
    mol = synth.gen_reads(n_mol, used, seed=77, err=0.0, q_mean=20.0)
    seqs, quals = zip(*(synth.materialize(mol, i) for i in range(n_mol)))
    text = "".join(f"@m{i} ch=1\n{s}\n+\n{q}\n" for i, (s, q) in enumerate(zip(seqs, quals))).encode()
    rs = scanfastq.ReadScanner(ctx, max_ed=1, split_chimeras=False)
    recs = [r for r in rs.pass2_chunk(text) if "_FAILED" not in r["name"] and "bc=" in r["name"]]
    gene = rng.integers(0, genes, len(recs))
    rows = []
    for m, r in enumerate(recs):
        q = r["name"].split(" ")[0]
        head, x_rest = q.split("_X=")
        x, rest = x_rest.split("_", 1)
        for c in range(copies):
            xs = list(x)
            if rng.random() < 0.3:  # a sequencing error inside the window
                xs[int(rng.integers(0, len(xs)))] = "ACGT"[int(rng.integers(0, 4))]
            nm = f"{head.replace('m', 'r%d_' % c, 1)}_X={''.join(xs)}_{rest}"
            rows.append((int(gene[m]) * 5_000 + int(rng.integers(-100, 100)), nm, 16 if gene[m] & 1 else 0, r["length"]))
    rows.sort(key=lambda t: t[0])
    n = len(rows)
    enc = [t[1].encode() for t in rows]
    noff = np.zeros(n + 1, dtype=np.uint32)
    noff[1:] = np.cumsum([len(e) for e in enc])
    nbuf = np.frombuffer(b"".join(enc) + b"\0", dtype=np.uint8)
    coff = np.arange(n + 1, dtype=np.uint32)
    cbuf = np.array([(t[3] << 4) | 0 for t in rows] + [0], dtype=np.uint32)  # one M operation per record
    fl = np.array([t[2] for t in rows], dtype=np.uint16)
    p0 = np.array([max(t[0], 0) + 1_000_000 for t in rows], dtype=np.int32)
    out = np.zeros(n, dtype=lib.UMI_TAG_DTYPE)
    nd = ctypes.c_int32(0)
    import threading

    def make_call(c, o, ndv, threads):
        cfg = lib.AssignUmisConfig()
        c._check(c._lib.smi_assignumis_default_config(ctypes.byref(cfg)))
        cfg.n_threads = threads

        def call():
            c._check(c._lib.smi_assignumis_chunk(c._h, nbuf.ctypes.data, noff.ctypes.data, fl.ctypes.data, p0.ctypes.data, cbuf.ctypes.data,
                                                 coff.ctypes.data, n, ctypes.byref(cfg), o.ctypes.data, ctypes.byref(ndv)))
        return call

    base = {"records": n, "molecules": len(recs), "copies": copies, "loci": genes}
    for label, env in (("host_path", "1"), ("device_stage", None)):
        if env:
            os.environ["SMI_AU_HOST"] = env
        for threads in (1, 16):
            dt = timed(make_call(ctx, out, nd, threads))
            res[f"assignumis_chunk_{label}_{threads}_threads"] = dict(base, ms=dt * 1e3, records_per_s=n / dt, clustered=int((out["flags"] & 4 != 0).sum()),
                                                                     with_region=int((out["region"] >= 0).sum()))
        os.environ.pop("SMI_AU_HOST", None)
    res["assignumis_chunk_device_stage_1_threads"]["note"] = ("one smi_assignumis_chunk call: names / flags / positions / CIGARs up, K-UPARSE, region grouping on "
                                                              "the host (two threads), key sort, K-UMI, K-UCLUST, K-UTAG, tags down")
    # several chunks side by side on worker lanes of the one GPU (UmiFinderWorker runs several OneBatchExecutors the same way)
    runs = []
    for lanes in (1, 2, 4, 8, 16):
        ctxs = [ctx] + [ctx.lane() for _ in range(lanes - 1)]
        outs = [np.zeros(n, dtype=lib.UMI_TAG_DTYPE) for _ in ctxs]
        calls = [make_call(c, o, ctypes.c_int32(0), 2) for c, o in zip(ctxs, outs)]
        for f in calls:
            f()
        per = 6

        def worker(f):
            for _ in range(per):
                f()
        th = [threading.Thread(target=worker, args=(f,)) for f in calls]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        dt = time.perf_counter() - t0
        same = all(o.tobytes() == outs[0].tobytes() for o in outs)
        runs.append({"lanes": lanes, "records_per_s": n * lanes * per / dt, "ms_per_chunk": dt / per * 1e3, "same_tags_on_every_lane": same})
        for c in ctxs[1:]:
            c.close()
    res["assignumis_device_stage_lanes"] = {"records_per_chunk": n, "runs": runs, "best": max(runs, key=lambda r: r["records_per_s"])}


def leg_chimera(pkg, synth, ctx, dev, wl, used, res):
    # ---- chimera splitter: K-PACKR + K-CHIM on whole reads; 10 % of the records are two molecules joined -----------
    n = 1_000_000
    rd = synth.gen_reads(n, used, seed=7, device=dev)
    buf, offs = synth.materialize_device(rd)
    keep = torch.ones(n + 1, dtype=torch.bool, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    keep[1:n][torch.rand(n - 1, device=dev, generator=g) < 0.1] = False  # dropping an offset joins two neighbouring reads
    offs = offs[keep].contiguous()
    n = offs.numel() - 1
    total = int(offs[-1])
    planes = torch.zeros(ctx.read_planes_words(total, n), dtype=torch.int32, device=dev)
    cres = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    ccfg = ctx.chimera_config()
    dt_pack = timed(lambda: ctx.pack_reads_device(buf, offs, n, total, planes))
    # K-PACK (read ends for K-SCAN), without and with the quality string (pass 1 sums every quality)
    ends = torch.zeros((28, 2 * n), dtype=torch.int32, device=dev)
    lens = torch.zeros(n, dtype=torch.int32, device=dev)
    dt_ends = timed(lambda: ctx.pack_ends_device(buf, None, offs, n, ends, lens))
    qt = torch.zeros((n, 224), dtype=torch.uint8, device=dev)
    qs = torch.zeros(n, dtype=torch.int32, device=dev)
    dt_ends_q = timed(lambda: ctx.pack_ends_device(buf, buf, offs, n, ends, lens, qt, qs))
    res["pack_ends"] = {"reads": n, "ms": dt_ends * 1e3, "reads_per_s": n / dt_ends, "with_quals_ms": dt_ends_q * 1e3,
                        "with_quals_GBps": 2 * total / dt_ends_q / 1e9}
    del ends, lens, qt, qs
    dt = timed(lambda: ctx.chimera_device(planes, offs, n, total, ccfg, cres))
    cr = cres.cpu().numpy().view(pkg.CHIMERA_RESULT_DTYPE).reshape(-1)
    res["chimera"] = {"reads": n, "bases": total, "pack_ms": dt_pack * 1e3, "ms": dt * 1e3, "reads_per_s": n / dt,
                      "bases_per_s": total / dt, "pack_GBps": total / dt_pack / 1e9,
                      "split_frac": float((cr["n_split"] > 0).mean()), "multi_frac": float((cr["flags"] & 1).mean()),
                      "overflow": int((cr["flags"] & 4).sum()),
                      "n_matches_bit0_frac": float((cr["n_matches"] & 1).mean()), "n_matches_bit1_frac": float(((cr["n_matches"] >> 1) & 1).mean())}


def leg_fastq(pkg, synth, ctx, dev, wl, used, res):
    from sicelore_amd import lib as libmod

    # ---- K-FQ: FASTQ text -> record index -> contiguous reads; text built on the device from synthetic reads -----------
    n = 500_000
    rd = synth.gen_reads(n, used, seed=9, device=dev)
    text, buf, offs = synth.fastq_text_device(rd)
    total = int(text.numel())
    cap = n + 2
    line = torch.zeros(4 * cap + 8, dtype=torch.int64, device=dev)
    ns, ss, qs = (torch.zeros(cap, dtype=torch.int64, device=dev) for _ in range(3))
    nl, sl = (torch.zeros(cap, dtype=torch.int32, device=dev) for _ in range(2))
    o = torch.zeros(cap + 1, dtype=torch.int64, device=dev)
    out = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=dev)
    state = {}

    def run():
        state["n"], state["err"] = ctx.fastq_index_device(text, total, line, ns, nl, ss, sl, qs, o, cap)
        ctx.fastq_gather_device(text, ss, o, state["n"], out)

    dt = timed(run)
    assert state["n"] == n and state["err"] == 0 and bool((out == buf).all())
    res["fastq_ingest"] = {"reads": n, "text_bytes": total, "ms": dt * 1e3, "text_GBps": total / dt / 1e9,
                           "reads_per_s": n / dt}
    # ---- K-WRITE: scan + barcode results of the same chunk -> `passed` / `failed` FASTQ text on the device ---------
    quals = torch.zeros(int(offs[-1]), dtype=torch.uint8, device=dev)
    ctx.fastq_gather_device(text, qs, o, n, quals)
    ends = torch.zeros((28, 2 * n), dtype=torch.int32, device=dev)
    lens32 = torch.zeros(n, dtype=torch.int32, device=dev)
    qt = torch.zeros((n, 224), dtype=torch.uint8, device=dev)
    qsum = torch.zeros(n, dtype=torch.int32, device=dev)
    ctx.pack_ends_device(out, quals, o[:n + 1], n, ends, lens32, qt, qsum)
    scan = torch.zeros((n, 8), dtype=torch.int32, device=dev)
    win = torch.zeros((n, 2), dtype=torch.int64, device=dev)
    ctx.scan_device(ends, lens32, n, ctx.scan_config(2), scan, win, qt, qsum)
    bc = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    ctx.set_barcode_set_device(used.to(torch.int32), mode=0)
    ctx.bc_match_device(win, bc, n, max_ed=1)
    capw = 2 * int(offs[-1]) + total + 320 * n
    out_p = torch.empty(capw, dtype=torch.uint8, device=dev)
    out_f = torch.empty(capw, dtype=torch.uint8, device=dev)
    rec_off_w = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    is_p = torch.zeros(n, dtype=torch.uint8, device=dev)

    def write():
        state["tot"] = ctx.fastq_write_device(text, line, out, quals, o[:n + 1], None, None, scan, bc, None, n, 1, out_p, out_f,
                                              rec_off_w, is_p)

    dtw = timed(write)
    wb = state["tot"][0] + state["tot"][1]
    # ---- the native chunk worker: host FASTQ text -> passed / failed text on the host (PCIe in both directions included) ----
    pin = libmod.PinnedBuffer(total)
    pin.array[:] = text.cpu().numpy()
    ctx.scanfastq_pass2_chunk(pin.array, copy=False)  # warm-up: arena and pinned output buffers of this size
    t0 = time.perf_counter()
    pp, ff, inf = ctx.scanfastq_pass2_chunk(pin.array, copy=False)
    dth = time.perf_counter() - t0
    n_out_bytes = int(pp.size + ff.size)
    t0 = time.perf_counter()
    ctx.scanfastq_pass2_chunk(pin.array.copy(), copy=False)  # the same from pageable memory
    dtp = time.perf_counter() - t0
    # three worker threads, each with its own context (stream, arena, pinned output) on the same GPU, as the reference runs
    # nCPU Parser workers: the transfers of one chunk overlap the kernels of another
    import threading

    n_ctx, per_thread = int(os.environ.get("SMI_MB_LANES", "3")), 3
    # worker LANES of the one context (smi_ctx_create_lane): own stream / arena / pinned buffers, the owner's barcode set
    extra = [ctx.lane() for _ in range(n_ctx - 1)]
    ctxs = [ctx] + extra
    pins = [pin] + [libmod.PinnedBuffer(total) for _ in extra]
    for pb in pins[1:]:
        pb.array[:] = pin.array
    for c, pb in zip(ctxs, pins):
        c.scanfastq_pass2_chunk(pb.array, copy=False)  # warm-up
    def worker(c, pb):
        for _ in range(per_thread):
            c.scanfastq_pass2_chunk(pb.array, copy=False)
    th = [threading.Thread(target=worker, args=(c, pb)) for c, pb in zip(ctxs, pins)]
    t0 = time.perf_counter()
    for t in th:
        t.start()
    for t in th:
        t.join()
    dtm = time.perf_counter() - t0
    for c in extra:
        c.close()
    for pb in pins[1:]:
        pb.close()
    pin.close()
    res["pass2_chunk_host_to_host_lanes"] = {"lanes": n_ctx, "reads": n * n_ctx * per_thread, "ms": dtm * 1e3,
                                             "reads_per_s": n * n_ctx * per_thread / dtm,
                                             "GB_per_s_both_directions": (total + n_out_bytes) * n_ctx * per_thread / dtm / 1e9,
                                             "note": f"{n_ctx} host threads, one worker lane each (one context, one barcode set) on one GPU, 3 chunks each"}
    res["pass2_chunk_host_to_host"] = {"reads": n, "text_in_bytes": total, "text_out_bytes": n_out_bytes,
                                       "records_out": inf["n_records_out"], "ms": dth * 1e3, "reads_per_s": n / dth,
                                       "pageable_input_ms": dtp * 1e3,
                                       "note": "one smi_scanfastq_pass2_chunk call: H2D of the text (page-locked buffer from smi_host_alloc), "
                                               "every kernel incl. the chimera splitter, D2H of both streams into the context's pinned buffers"}
    res["fastq_write"] = {"reads": n, "passed": state["tot"][2], "out_bytes": wb, "ms": dtw * 1e3, "out_GBps": wb / dtw / 1e9,
                          "reads_per_s": n / dtw}


def leg_deflate(pkg, synth, ctx, dev, wl, used, res):
    """K-DEFLATE on the FASTQ text of a pass-2 chunk (qualities drawn uniformly from 29 values per base, as run_files.write_synthetic_dir
    does): GB/s of text, size against zlib level 6 and level 1 on a 64 MB sample of the same text"""
    import zlib

    n = int(os.environ.get("SMI_MB_READS", "500000"))
    rd = synth.gen_reads(n, used, seed=9, device=dev, q_mean=20.0)
    text = synth.fastq_text_device(rd)[0]
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    is_q = text == ord("I")
    text[is_q] = torch.randint(35, 64, (int(is_q.sum()),), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
    del rd, is_q
    total = int(text.numel())
    d_out = torch.empty(int(ctx._lib.smi_deflate_bound(total)), dtype=torch.uint8, device=dev)
    state = {}

    def run():
        state["z"] = ctx.gzip_device(text, total, d_out=d_out)

    dt = timed(run, reps=5)
    z = state["z"]
    sample = text[:64 << 20].cpu().numpy().tobytes()
    zs = ctx.gzip_device(text[:64 << 20].contiguous(), len(sample)).cpu().numpy().tobytes()
    assert zlib.decompress(zs, wbits=31) == sample
    t0 = time.perf_counter()
    z6 = len(zlib.compress(sample, 6))
    t6 = time.perf_counter() - t0
    t0 = time.perf_counter()
    z1 = len(zlib.compress(sample, 1))
    t1 = time.perf_counter() - t0
    res["gzip_device"] = {"text_bytes": total, "member_bytes": int(z.numel()), "ratio": total / int(z.numel()), "ms": dt * 1e3, "text_GBps": total / dt / 1e9,
                          "sample_bytes": len(sample), "sample_member_bytes": len(zs), "sample_zlib6_bytes": z6, "sample_zlib1_bytes": z1,
                          "size_vs_zlib6": len(zs) / z6, "zlib6_MBps_one_thread": len(sample) / t6 / 1e6, "zlib1_MBps_one_thread": len(sample) / t1 / 1e6,
                          "note": "one call incl. the 16-byte read-back of size and flags; literals-only dynamic Huffman blocks of 64 KiB"}


def _tagbam_files(d, n_reads, n_recs, read_len, seed=21):
    """a FASTQ of n_reads reads (36-character UUID names with a ` runid=.. ch=..` comment, read_len bases) and a coordinate-sorted BAM of
    n_recs alignments of read_len bases (names drawn from the FASTQ with repeats = secondary / supplementary records; 1 % of them absent from
    the FASTQ, 0.5 % without a reference), both built with numpy; the BAM is written with the library's host BGZF writer"""
    from sicelore_amd import lib

    rng = np.random.default_rng(seed)
    hexd = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
    uuid = hexd[rng.integers(0, 16, (n_reads, 36))]
    uuid[:, [8, 13, 18, 23]] = ord("-")
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comment = np.frombuffer(b" runid=5f3c ch=101", dtype=np.uint8)
    L = read_len
    row = 1 + 36 + comment.size + 1 + L + 1 + 2 + L + 1
    fq = np.empty((n_reads, row), dtype=np.uint8)
    c = 0
    for part, w in ((b"@", 1), (uuid, 36), (comment, comment.size), (b"\n", 1), (None, L), (b"\n+\n", 3), ("q", L), (b"\n", 1)):
        if part is None:
            fq[:, c:c + w] = acgt[rng.integers(0, 4, (n_reads, L), dtype=np.uint8)]
        elif isinstance(part, str):
            fq[:, c:c + w] = rng.integers(35, 75, (n_reads, L), dtype=np.uint8)
        elif isinstance(part, bytes):
            fq[:, c:c + w] = np.frombuffer(part, dtype=np.uint8)
        else:
            fq[:, c:c + w] = part
        c += w
    fq.reshape(-1).tofile(os.path.join(d, "reads.fastq"))
    del fq
    src = rng.integers(0, n_reads, n_recs)
    absent = rng.random(n_recs) < 0.01
    unmapped = rng.random(n_recs) < 0.005
    names = uuid[src].copy()
    names[absent, 0] = ord("z")                      # no FASTQ name starts with z
    aux = np.frombuffer(b"NMc\x05tpAPs1i\x10\x00\x00\x00", dtype=np.uint8)
    body = 32 + 37 + 4 + (L + 1) // 2 + L + aux.size
    rec = np.zeros((n_recs, 4 + body), dtype=np.uint8)
    hdr = np.zeros(n_recs, dtype=np.dtype([("bs", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("lrn", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("ncig", "<u2"),
                                          ("flag", "<u2"), ("lseq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4")]))
    hdr["bs"], hdr["ref"], hdr["pos"] = body, np.where(unmapped, -1, 0), np.where(unmapped, -1, np.arange(n_recs) * 40)
    hdr["lrn"], hdr["mapq"], hdr["bin"], hdr["ncig"], hdr["lseq"], hdr["nref"], hdr["npos"] = 37, 60, 4680, 1, L, -1, -1
    hdr["flag"] = np.where(unmapped, 4, rng.choice(np.array([0, 16, 256, 2048], dtype=np.uint16), n_recs, p=[0.45, 0.45, 0.05, 0.05]))
    order = np.argsort(unmapped, kind="stable")         # the unplaced records last, as a coordinate sort leaves them
    rec[:, :36] = hdr.view(np.uint8).reshape(n_recs, 36)
    rec[:, 36:72] = names
    c = 73
    rec[:, c:c + 4] = np.frombuffer(np.array([(L << 4) | 0], dtype="<u4").tobytes(), dtype=np.uint8)
    c += 4
    rec[:, c:c + (L + 1) // 2] = rng.choice(np.array([0x12, 0x48, 0x84, 0x21, 0x44, 0x18], dtype=np.uint8), (n_recs, (L + 1) // 2))
    c += (L + 1) // 2
    rec[:, c:c + L] = 30
    rec[:, c + L:] = aux
    rec = rec[order]
    head = b"BAM\1" + np.array([0], dtype="<u4").tobytes() + np.array([1], dtype="<u4").tobytes() + np.array([5], dtype="<u4").tobytes() \
        + b"chr1\0" + np.array([2 ** 31 - 1], dtype="<u4").tobytes()
    bam = np.concatenate([np.frombuffer(head, dtype=np.uint8), rec.reshape(-1)])
    del rec
    lib.bgzf_deflate(bam, level=1, n_threads=16).tofile(os.path.join(d, "in.bam"))
    return int(bam.size)


def leg_tagbam(pkg, synth, ctx, dev, wl, used, res):
    """K-TAG (`tagbamwithread`) at the size of one run: SMI_MB_TAG_READS reads (2 M) of ~1 kb, 1.1 alignments per read.  File to file with the
    device BGZF writer and with 16 host threads of zlib; device ms per stage from HIP events (the kernel times of a rocprofv3 run of this leg
    are in profiles/tagbam/), each against its ceiling: build and probe as random gathers (43-48 G/s, BENCH_r06.json hbm_measured), assemble as
    streamed bytes (8 TB/s)"""
    import shutil
    import tempfile

    tb = importlib.import_module(graft.PKG_NAME + ".tagbamwithread")
    n = int(os.environ.get("SMI_MB_TAG_READS", "2000000"))
    m = int(n * 1.1)
    d = tempfile.mkdtemp(prefix="tagbam_")
    try:
        t0 = time.perf_counter()
        bam_bytes = _tagbam_files(d, n, m, 1000)
        t_gen = time.perf_counter() - t0
        fq_bytes = os.path.getsize(os.path.join(d, "reads.fastq"))
        out = {"reads": n, "bam_records": m, "fastq_bytes": fq_bytes, "bam_inflated_bytes": bam_bytes, "bam_file_bytes": os.path.getsize(os.path.join(d, "in.bam")),
               "fixture_s": t_gen}
        for bgzf in ("device", "zlib"):
            with open(os.devnull, "w") as err:
                info = tb.tag_bam_with_reads(ctx, os.path.join(d, "reads.fastq"), os.path.join(d, "in.bam"), os.path.join(d, "out.bam"), "US", "QS",
                                             n_threads=16, bgzf=bgzf, err=err)
            out[bgzf] = {"wall_s": info["wall_s"], "records_per_s": info["records"] / info["wall_s"], "written": info["written"], "missing": info["missing"],
                         "unmapped": info["unmapped"], "seconds": info["seconds"], "stage_ms": info["stage_ms"],
                         "out_file_bytes": os.path.getsize(os.path.join(d, "out.bam"))}
        ms = out["device"]["stage_ms"]
        out_bytes = bam_bytes + 2 * 1000 * out["device"]["written"]         # (about: the records grow by their two Z strings)
        out["ceilings"] = {
            "key_GBps_text": fq_bytes / (ms["key"] * 1e6) if ms["key"] else None,
            "build_Ggathers_per_s": 4 * n / (ms["build"] * 1e6) if ms["build"] else None,
            "probe_Ggathers_per_s": 4 * m / (ms["probe"] * 1e6) if ms["probe"] else None,
            "gather_ceiling_G_per_s": "43-48",
            "assemble_TBps_streamed": (bam_bytes + out_bytes) / (ms["assemble"] * 1e9) if ms["assemble"] else None,
            "stream_ceiling_TBps": 8.0,
            "note": "4 dependent random reads per insert / probe (table word, key length, name start, name bytes); assemble streams the input records "
                    "and the FASTQ payloads in and the output out"}
        res["tagbam"] = out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def _noisy(rng, src, rate):
    """ONT-like copy of src (uint8 bases): substitutions, insertions and deletions of rate / 3 each"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    x = rng.random(src.size)
    out = src.copy()
    sub = x < rate / 3
    out[sub] = acgt[rng.integers(0, 4, int(sub.sum()))]
    reps = np.ones(src.size, dtype=np.int64)
    reps[(x >= rate / 3) & (x < 2 * rate / 3)] = 2        # the base and an inserted one
    reps[(x >= 2 * rate / 3) & (x < rate)] = 0            # deleted
    idx = np.repeat(np.arange(src.size), reps)
    res = out[idx]
    second = np.flatnonzero(idx[1:] == idx[:-1]) + 1
    res[second] = acgt[rng.integers(0, 4, second.size)]
    return res


def _consensus_molecules(n_mol, seed=31, length=1000, rate=0.07):
    """n_mol molecules of one ~1 kb cDNA each: half of them 1 or 2 reads, half 3 to 30 reads, every read a noisy copy"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    mols = []
    for m in range(n_mol):
        k = int(rng.integers(1, 3)) if m % 2 else int(rng.integers(3, 31))
        src = acgt[rng.integers(0, 4, length)]
        mols.append([_noisy(rng, src, rate).tobytes() for _ in range(k)])
    return mols


def _consensus_bam(mols, seed=32):
    """one BAM record per read: BC / U8, US = 20 bases of TSO side + cDNA + 30 of polyA side, TE / PS, de; no SEQ (ComputeConsensus reads US)"""
    import struct

    from sicelore_amd import lib

    rng = np.random.default_rng(seed)
    recs = []
    k = 0
    for m, reads in enumerate(mols):
        for r in reads:
            us = b"T" * 20 + r + b"A" * 30
            aux = (b"BCZ" + b"CELL%05d-1" % (m % 3000) + b"\0" + b"U8Z" + b"UMI%07d" % m + b"\0" + b"USZ" + us + b"\0"
                   + b"TEs" + struct.pack("<h", 20) + b"PSS" + struct.pack("<H", 20 + len(r)) + b"def" + struct.pack("<f", float(rng.integers(0, 50)) / 500))
            name = b"read%08d\0" % k
            body = struct.pack("<iiBBHHHiiii", 0, 100 + k, len(name), 60, 4680, 1, 0, 0, -1, -1, 0) + name + struct.pack("<I", (len(r) << 4) | 0) + aux
            recs.append(struct.pack("<I", len(body)) + body)
            k += 1
    head = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 1) + struct.pack("<I", 5) + b"chr1\0" + struct.pack("<I", 2 ** 31 - 1)
    bam = np.frombuffer(head + b"".join(recs), dtype=np.uint8)
    return lib.bgzf_deflate(bam, level=1, n_threads=16), k


def leg_consensus(pkg, synth, ctx, dev, wl, used, res):
    """K-POA (`ComputeConsensus`): SMI_MB_CC_MOLS molecules (4000) of a 1 kb cDNA with ~7 % ONT-like errors, 1 to 30 reads, about half with
    3 or more.  Device: smi_poa_batch over the multi-read molecules with their first 20 reads (MAXREADS), molecules/s and DP cells/s (cells
    counted against the consensus length: a lower bound, the graph has more nodes than its consensus).  File to file: compute_consensus
    on a BAM of one record per read."""
    import shutil
    import tempfile

    from sicelore_amd import lib

    cc = importlib.import_module(graft.PKG_NAME + ".computeconsensus")
    n = int(os.environ.get("SMI_MB_CC_MOLS", "4000"))
    t0 = time.perf_counter()
    mols = _consensus_molecules(n)
    out = {"molecules": n, "reads": sum(len(m) for m in mols), "fixture_s": time.perf_counter() - t0}
    multi = [m[:20] for m in mols if len(m) >= 3]
    seqs = np.frombuffer(b"".join(r for m in multi for r in m), dtype=np.uint8).copy()
    read_off = np.zeros(sum(len(m) for m in multi) + 1, dtype=np.uint64)
    read_off[1:] = np.cumsum([len(r) for m in multi for r in m])
    mol_off = np.zeros(len(multi) + 1, dtype=np.int32)
    mol_off[1:] = np.cumsum([len(m) for m in multi])
    lib.poa_batch(ctx, seqs[:int(read_off[mol_off[min(50, len(multi))]])].copy(), read_off[:mol_off[min(50, len(multi))] + 1].copy(),
                  mol_off[:min(50, len(multi)) + 1].copy())                                   # warm-up
    t0 = time.perf_counter()
    cons, _qv, ms, rerun = lib.poa_batch(ctx, seqs, read_off, mol_off)
    wall = time.perf_counter() - t0
    cells = sum(len(r) * len(c) for m, c in zip(multi, cons) for r in m[1:])
    out["device"] = {"poa_molecules": len(multi), "reads": int(mol_off[-1]), "kernel_ms": ms, "call_s": wall, "rerun": rerun,
                     "molecules_per_s": len(multi) / (ms / 1e3), "cells_lower_bound": cells, "cells_per_s": cells / (ms / 1e3),
                     "mean_consensus_len": float(np.mean([len(c) for c in cons]))}
    d = tempfile.mkdtemp(prefix="consensus_")
    try:
        t0 = time.perf_counter()
        z, n_rec = _consensus_bam(mols)
        z.tofile(os.path.join(d, "in.bam"))
        out["bam_fixture_s"] = time.perf_counter() - t0
        info = cc.compute_consensus(ctx, os.path.join(d, "in.bam"), os.path.join(d, "out.fq"), n_threads=16)
        out["file_to_file"] = {"records": info["records"], "molecules": info["molecules"], "poa_molecules": info["poa_molecules"], "wall_s": info["wall_s"],
                               "records_per_s": info["records"] / info["wall_s"], "molecules_per_s": info["molecules"] / info["wall_s"],
                               "seconds": info["seconds"], "poa_kernel_ms": info["poa_kernel_ms"]}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["consensus"] = out


def _isoform_fixture(n_genes, n_recs, n_cells, seed=41, molecule_names=False, minus1=True):
    """a seeded refFlat (n_genes genes of 1..19 transcripts, 1..40 exons each) and a BAM of n_recs records: molecules of 1..3 reads, each
    read spliced along one transcript with junction ends moved by up to 3 bases; minus1: the barcodes carry 10x's "-1", in the BAM and the list"""
    import struct

    from sicelore_amd import lib

    rng = np.random.default_rng(seed)
    lines, genes = [], []
    pos = 10_000
    for g in range(n_genes):
        n_ex = int(rng.integers(1, 41))
        span = []
        p = pos
        for _e in range(n_ex):
            ln = int(rng.integers(60, 400))
            span.append((p, p + ln))
            p += ln + int(rng.integers(200, 3000))
        txs = []
        for t in range(int(rng.integers(1, 20))):
            keep = [e for e in span if rng.random() < 0.8] or span[:1]
            txs.append(keep)
            lines.append(f"GENE{g}\tTX{g}.{t}\tchr1\t+\t{keep[0][0]}\t{keep[-1][1]}\t{keep[0][0]}\t{keep[-1][1]}\t{len(keep)}\t"
                         + "".join(f"{a}," for a, _b in keep) + "\t" + "".join(f"{b}," for _a, b in keep) + "\n")
        genes.append(txs)
        pos = p + 5000
    recs, k, m = [], 0, 0
    while k < n_recs:
        g = int(rng.integers(n_genes))
        ex = genes[g][int(rng.integers(len(genes[g])))]
        cell, umi = b"CELL%05d" % int(rng.integers(n_cells)) + (b"-1" if minus1 else b""), b"U%09d" % m
        aux_m = b"BCZ" + cell + b"\0" + b"U8Z" + umi + b"\0" + b"GEZ" + b"GENE%d" % g + b"\0"
        for _r in range(int(rng.integers(1, 4))):
            cig, cur, p1 = [], None, ex[0][0] + 1
            for i, (a, b) in enumerate(ex):
                s0, e0 = a + 1, b
                if i:
                    s0 += int(rng.integers(-3, 4))
                if i < len(ex) - 1:
                    e0 += int(rng.integers(-3, 4))
                if cur is not None:
                    cig.append((s0 - cur - 1) << 4 | 3)
                cig.append(max(1, e0 - s0 + 1) << 4 | 0)
                cur = s0 + max(1, e0 - s0 + 1) - 1
            name = b"r%09d\0" % k
            if molecule_names:                       # what DeduplicateMolecule leaves: BC-U8-rn
                name = cell[:-2] + b"-" + umi + b"-%d\0" % int(rng.integers(1, 60))
            aux = aux_m + b"def" + struct.pack("<f", float(rng.integers(0, 50)) / 500)
            body = struct.pack("<iiBBHHHiiii", 0, p1 - 1, len(name), 60, 4680, len(cig), 0, 0, -1, -1, 0) + name + struct.pack(f"<{len(cig)}I", *cig) + aux
            recs.append(struct.pack("<I", len(body)) + body)
            k += 1
        m += 1
    head = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 1) + struct.pack("<I", 5) + b"chr1\0" + struct.pack("<I", 2 ** 31 - 1)
    bam = np.frombuffer(head + b"".join(recs), dtype=np.uint8)
    csv = "".join(f"CELL{c:05d}{'-1' if minus1 else ''}\n" for c in range(n_cells))
    return "".join(lines), csv, lib.bgzf_deflate(bam, level=1, n_threads=16), k, m


def leg_isoform(pkg, synth, ctx, dev, wl, used, res):
    """K-ISO + K-MTX (`IsoformMatrix`): a seeded refFlat of SMI_MB_ISO_GENES genes (20,000; about 10 transcripts each, up to 40 exons), 5,000
    cells, SMI_MB_ISO_RECS records (2,000,000).  File to file with ISOBAM: device ms of K-ISO, sort + RLE and render (HIP events), wall
    seconds per phase, bytes written per second."""
    import shutil
    import tempfile

    iso = importlib.import_module(graft.PKG_NAME + ".isoformmatrix")
    n_genes = int(os.environ.get("SMI_MB_ISO_GENES", "20000"))
    n_recs = int(os.environ.get("SMI_MB_ISO_RECS", "2000000"))
    t0 = time.perf_counter()
    ref, csv, z, n_rec, n_mol = _isoform_fixture(n_genes, n_recs, 5000)
    out = {"genes": n_genes, "records": n_rec, "molecules_generated": n_mol, "cells": 5000, "fixture_s": time.perf_counter() - t0}
    d = tempfile.mkdtemp(prefix="isoform_")
    try:
        z.tofile(os.path.join(d, "in.bam"))
        with open(os.path.join(d, "r.refFlat"), "w") as f:
            f.write(ref)
        with open(os.path.join(d, "c.csv"), "w") as f:
            f.write(csv)
        info = iso.isoform_matrix(ctx, os.path.join(d, "in.bam"), os.path.join(d, "r.refFlat"), os.path.join(d, "c.csv"), d, n_threads=16,
                                  isobam=True)
        keys = ("records", "molecules", "onematch", "ambiguous", "nomatch", "monoexon", "matrix_isoforms", "matrix_genes", "matrix_junctions",
                "spill", "render_blocks")
        out["file_to_file"] = dict({k: info[k] for k in keys}, stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"],
                                   bytes_written=info["bytes_written"], bytes_per_s=info["bytes_written"] / info["wall_s"],
                                   records_per_s=info["records"] / info["wall_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["isoform"] = out


def leg_moltag(pkg, synth, ctx, dev, wl, used, res):
    """K-NAME / K-GENE / K-EDIT (`AddBamMoleculeTags`, then `AddGeneNameTag` on its output): the isoform leg's seeded refFlat and spliced
    records (SMI_MB_MOLTAG_GENES genes, SMI_MB_MOLTAG_RECS records, 2,000,000) under names BC-U8-rn.  File to file: device ms per stage
    (HIP events, summed over the segments), seconds in the device calls (copies included), in deflate and in file writes, wall seconds;
    beside K-GENE the wall time of smi_gene_tag_bam, the host code it restates, on the same records."""
    import shutil
    import tempfile

    mt = importlib.import_module(graft.PKG_NAME + ".moltags")
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    n_genes = int(os.environ.get("SMI_MB_MOLTAG_GENES", "20000"))
    n_recs = int(os.environ.get("SMI_MB_MOLTAG_RECS", "2000000"))
    t0 = time.perf_counter()
    ref, _csv, z, n_rec, n_mol = _isoform_fixture(n_genes, n_recs, 5000, molecule_names=True)
    out = {"genes": n_genes, "records": n_rec, "molecules_generated": n_mol, "fixture_s": time.perf_counter() - t0}
    d = tempfile.mkdtemp(prefix="moltag_")
    try:
        z.tofile(os.path.join(d, "in.bam"))
        with open(os.path.join(d, "r.refFlat"), "w") as f:
            f.write(ref)
        for name, run in (("AddBamMoleculeTags", lambda: mt.add_bam_molecule_tags(ctx, os.path.join(d, "in.bam"), os.path.join(d, "tags.bam"), n_threads=16)),
                          ("AddGeneNameTag", lambda: mt.add_gene_name_tag(ctx, os.path.join(d, "tags.bam"), os.path.join(d, "ge.bam"),
                                                                          os.path.join(d, "r.refFlat"), n_threads=16))):
            info = run()
            kernel_s = sum(info["stage_ms"].values()) / 1e3
            out[name] = dict({k: info[k] for k in lib.MOLTAG_COUNTS}, stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"],
                             bytes_written=info["bytes_written"], records_per_s=info["records"] / info["wall_s"],
                             copy_share_of_wall=max(0.0, info["seconds"]["device"] - kernel_s) / info["wall_s"])
        bam, _used = lib.bgzf_inflate(np.fromfile(os.path.join(d, "tags.bam"), dtype=np.uint8), n_threads=16)
        _text, refs, start = lib.bam_header(bam)
        recs, _end = lib.bam_index_records(bam, start, cap=n_rec + 1)
        tagger = lib.GeneTagger(ref, [r[0] for r in refs])
        t0 = time.perf_counter()
        tagger.tag_bam_raw(bam, recs)
        out["smi_gene_tag_bam_wall_s"] = time.perf_counter() - t0
        out["k_gene_device_s"] = out["AddGeneNameTag"]["stage_ms"]["gene"] / 1e3
        tagger.close()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["moltag"] = out


def leg_collapse(pkg, synth, ctx, dev, wl, used, res):
    """K-COLLAPSE / K-COLSTAT / K-FILTER / K-CLASS (`CollapseModel`): the isoform leg's fixture (SMI_MB_COL_GENES genes, 20,000;
    SMI_MB_COL_RECS records, 2,000,000) run through `IsoformMatrix ISOBAM=true`, then CollapseModel file to file on that ISOBAM: device ms
    per stage (HIP events), seconds in parse, in the device calls and in file writes, wall seconds, and beside K-COLLAPSE the wall time of the
    reference's single-thread collapse() loop on the same arrays (smi_collapse_host_loop), with the records on which the two differ (0)."""
    import shutil
    import tempfile

    iso = importlib.import_module(graft.PKG_NAME + ".isoformmatrix")
    col = importlib.import_module(graft.PKG_NAME + ".collapsemodel")
    n_genes = int(os.environ.get("SMI_MB_COL_GENES", "20000"))
    n_recs = int(os.environ.get("SMI_MB_COL_RECS", "2000000"))
    t0 = time.perf_counter()
    ref, csv, z, n_rec, n_mol = _isoform_fixture(n_genes, n_recs, 5000, minus1=False)   # ISOBAM and CollapseModel look the RAW barcode up (8d, 8h)
    out = {"genes": n_genes, "records": n_rec, "molecules_generated": n_mol, "cells": 5000, "fixture_s": time.perf_counter() - t0}
    d = tempfile.mkdtemp(prefix="collapse_")
    try:
        z.tofile(os.path.join(d, "in.bam"))
        with open(os.path.join(d, "r.refFlat"), "w") as f:
            f.write(ref)
        with open(os.path.join(d, "c.csv"), "w") as f:
            f.write(csv)
        t0 = time.perf_counter()
        iso.isoform_matrix(ctx, os.path.join(d, "in.bam"), os.path.join(d, "r.refFlat"), os.path.join(d, "c.csv"), d, n_threads=16, isobam=True)
        out["isobam_s"] = time.perf_counter() - t0
        info = col.collapse_model(ctx, os.path.join(d, "sicelore_isobam.bam"), os.path.join(d, "r.refFlat"), os.path.join(d, "c.csv"), d,
                                  n_threads=16, host_loop=True)
        lib = importlib.import_module(graft.PKG_NAME + ".lib")
        out["file_to_file"] = dict({k: info[k] for k in lib.COLLAPSE_COUNTS}, stage_ms=info["stage_ms"], seconds=info["seconds"],
                                   wall_s=info["wall_s"], bytes_written=info["bytes_written"], records_per_s=info["records"] / info["wall_s"])
        out["k_collapse_device_s"] = info["stage_ms"]["collapse"] / 1e3
        out["host_collapse_loop_wall_s"] = info["host_loop_s"]
        out["host_loop_mismatches"] = info["host_loop_mismatches"]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["collapse"] = out


def _short_fixture(junctions, n_recs, span, seed=71, spliced_share=0.2):
    """a seeded SHORT of n_recs 100-base records on chr1, a fifth of them spliced over `junctions` ((donor, acceptor) rows): a third of the
    junctions supported exactly, a third off by one, a third by a junction nearby; groups of four unspliced records and a spliced one
    -> (BGZF bytes, records, spliced records)"""
    from sicelore_amd import lib

    rng = np.random.default_rng(seed)
    fixed = [("block_size", "<u4"), ("ref_id", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"),
             ("flag", "<u2"), ("l_seq", "<i4"), ("next_ref", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("name", "S11")]
    tail = [("seq", "u1", (50,)), ("qual", "u1", (100,))]
    plain = np.dtype(fixed + [("cigar", "<u4", (1,))] + tail)
    splic = np.dtype(fixed + [("cigar", "<u4", (3,))] + tail)
    n_grp = n_recs // 5
    grp = np.zeros(n_grp, dtype=np.dtype([("u", plain, (4,)), ("s", splic)]))
    for part, dt, n_op in ((grp["u"], plain, 1), (grp["s"], splic, 3)):
        part["block_size"] = dt.itemsize - 4
        part["l_read_name"], part["mapq"], part["bin"], part["n_cigar"], part["l_seq"] = 11, 60, 4680, n_op, 100
        part["next_ref"] = part["next_pos"] = -1
        part["seq"], part["qual"] = 0x11, 30
    ids = np.arange(n_grp * 5, dtype=np.int64).reshape(n_grp, 5)
    grp["u"]["name"] = np.char.add("u", np.char.zfill(ids[:, :4].astype("U9"), 9)).astype("S11")
    grp["s"]["name"] = np.char.add("s", np.char.zfill(ids[:, 4].astype("U9"), 9)).astype("S11")
    grp["u"]["pos"] = rng.integers(10_000, span, size=(n_grp, 4))
    grp["u"]["cigar"][..., 0] = 100 << 4
    grp["u"]["flag"] = 16 * rng.integers(0, 2, size=(n_grp, 4))
    k = rng.integers(0, len(junctions), size=n_grp)
    d, a = junctions[k, 0].copy(), junctions[k, 1].copy()
    side, step = rng.integers(0, 2, size=n_grp), rng.choice((-1, 1), size=n_grp)
    off = k % 3 == 1
    d[off & (side == 0)] += step[off & (side == 0)]
    a[off & (side == 1)] += step[off & (side == 1)]
    d[k % 3 == 2] += 7
    a[k % 3 == 2] += 9
    left = rng.integers(10, 91, size=n_grp)
    grp["s"]["pos"] = d - left
    grp["s"]["cigar"][:, 0] = left << 4
    grp["s"]["cigar"][:, 1] = np.maximum(a - d - 1, 0) << 4 | 3
    grp["s"]["cigar"][:, 2] = (100 - left) << 4
    grp["s"]["flag"] = rng.choice((0, 16, 0x100, 0x400), size=n_grp)
    head = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 1) + struct.pack("<I", 5) + b"chr1\0" + struct.pack("<I", 2 ** 31 - 1)
    bam = np.concatenate([np.frombuffer(head, dtype=np.uint8), grp.view(np.uint8)])
    return lib.bgzf_deflate(bam, level=1, n_threads=16), n_grp * 5, n_grp


def leg_validator(pkg, synth, ctx, dev, wl, used, res):
    """K-JSUP (the validator of `CollapseModel`): the collapse leg's fixture (SMI_MB_VAL_GENES genes, 20,000; SMI_MB_VAL_RECS records,
    2,000,000) through `IsoformMatrix ISOBAM=true` and CollapseModel; then a seeded SHORT of SMI_MB_VAL_SHORT 100-base records (3,000,000, a
    fifth spliced over the novel junctions that run printed) and two BED files of one feature per 50th transcript end, through
    smi_collapse_validate_*: K-JSUP device ms (HIP events, summed over segments), seconds waiting for inflate + index (the reader thread
    works one segment ahead), in upload + kernel (validate_segment) and in read-back + rendering (validate_end)."""
    import shutil
    import tempfile

    iso = importlib.import_module(graft.PKG_NAME + ".isoformmatrix")
    segments = importlib.import_module(graft.PKG_NAME + ".bamsegments").segments
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    n_genes = int(os.environ.get("SMI_MB_VAL_GENES", "20000"))
    n_recs = int(os.environ.get("SMI_MB_VAL_RECS", "2000000"))
    n_short = int(os.environ.get("SMI_MB_VAL_SHORT", "3000000"))
    seg_bytes = int(os.environ.get("SMI_MB_VAL_SEGMENT", str(64 << 20)))
    t0 = time.perf_counter()
    ref, csv, z, n_rec, n_mol = _isoform_fixture(n_genes, n_recs, 5000, minus1=False)
    out = {"genes": n_genes, "records": n_rec, "cells": 5000, "fixture_s": time.perf_counter() - t0}
    print("validator: fixture built", file=sys.stderr, flush=True)
    d = tempfile.mkdtemp(prefix="validator_")
    h = None
    try:
        z.tofile(os.path.join(d, "in.bam"))
        with open(os.path.join(d, "r.refFlat"), "w") as f:
            f.write(ref)
        with open(os.path.join(d, "c.csv"), "w") as f:
            f.write(csv)
        iso.isoform_matrix(ctx, os.path.join(d, "in.bam"), os.path.join(d, "r.refFlat"), os.path.join(d, "c.csv"), d, n_threads=16, isobam=True)
        print("validator: ISOBAM written", file=sys.stderr, flush=True)
        t0 = time.perf_counter()
        for bam, recs, hdr in segments(os.path.join(d, "sicelore_isobam.bam"), 256 << 20, 16):
            if hdr is not None:
                h = lib.Collapse(ctx, ref.encode(), csv.encode(), [r[0] for r in lib.bam_header(bam)[1]], n_threads=16)
            if recs.size:
                h.add_segment(bam, recs)
        txt = h.run()[".txt"].decode()
        out["collapse_s"] = time.perf_counter() - t0
        rows = [ln.split("\t") for ln in txt.split("\n")[1:-1]]
        junc = np.array(sorted(set(tuple(int(x) for x in j.split("-")) for r in rows if r[11] != "-" for j in r[11].split(","))), dtype=np.int64)
        span = max(int(r[5]) for r in rows)
        bed = ["".join(f"chr1\t{int(r[c]) + 20 * (i % 7 - 3)}\t{int(r[c]) + 60}\tf{i}\t0\t{r[3]}\n" for i, r in enumerate(rows) if i % 50 == 0)
               for c in (4, 5)]
        t0 = time.perf_counter()
        zs, n_s, n_spl = _short_fixture(junc, n_short, span)
        zs.tofile(os.path.join(d, "short.bam"))
        out.update(transcripts=len(rows), novel_junctions=int(len(junc)), short_records=n_s, short_spliced=n_spl, short_bgzf_bytes=int(zs.size),
                   short_fixture_s=time.perf_counter() - t0)
        print("validator: SHORT written", file=sys.stderr, flush=True)
        sec = dict(inflate_index_wait=0.0, upload_kernel=0.0, begin=0.0, end_render=0.0)
        inflated = 0
        t_all = t0 = time.perf_counter()
        for bam, recs, hdr in segments(os.path.join(d, "short.bam"), seg_bytes, 16):
            sec["inflate_index_wait"] += time.perf_counter() - t0
            if hdr is not None:
                t0 = time.perf_counter()
                h.validate_begin(bed[0].encode(), bed[1].encode(), [r[0] for r in lib.bam_header(bam)[1]])
                sec["begin"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            if recs.size:
                h.validate_segment(bam, recs)
            sec["upload_kernel"] += time.perf_counter() - t0
            inflated += int(bam.size)
            t0 = time.perf_counter()
        t0 = time.perf_counter()
        outs = h.validate_end()
        sec["end_render"] = time.perf_counter() - t0
        out["validate"] = dict(h.validate_counts(), k_jsup_device_ms=h.stage_ms["jsup"], seconds=sec, wall_s=time.perf_counter() - t_all,
                               segment_bytes=seg_bytes, inflated_bytes=inflated, text_bytes=sum(len(v) for v in outs.values()))
    finally:
        if h is not None:
            h.close()
        shutil.rmtree(d, ignore_errors=True)
    res["validator"] = out


def _fusion_fixture(n_recs, n_cells, n_genes, seed=61):
    """a seeded tagged BAM of n_recs records as the plumbing of step 6 leaves it: molecules of 1..3 reads of 1..2 records (the second one
    supplementary, now and then without UMI), barcodes with 10x's "-1", GE of one gene or, for about a tenth of the molecules, of a second
    gene on some records (a handful of recurrent pairs among them), RN on a third of the records, de on all -> (cell list, BGZF bytes,
    records, molecules)"""
    import struct

    from sicelore_amd import lib

    rng = np.random.default_rng(seed)
    recurrent = [(b"BCR", b"ABL1"), (b"EML4", b"ALK"), (b"TMPRSS2", b"ERG"), (b"KIF5B", b"RET")]
    recs, k, m = [], 0, 0
    cig = struct.pack("<3I", 40 << 4 | 4, 900 << 4 | 0, 60 << 4 | 4)
    while k < n_recs:
        cell, umi = b"CELL%05d-1" % int(rng.integers(n_cells)), b"U%09d" % m
        g0 = b"GENE%d" % int(rng.integers(n_genes))
        p = rng.random()
        g1 = None if p < 0.9 else b"GENE%d" % int(rng.integers(n_genes))
        if p > 0.98:
            g0, g1 = recurrent[int(rng.integers(len(recurrent)))]
        for _r in range(int(rng.integers(1, 4))):
            name = b"r%09d\0" % k
            for j in range(int(rng.integers(1, 3))):
                ge = g0 if g1 is None or (j == 0 and rng.random() < 0.5) else g1 if rng.random() < 0.5 else g0 + b"," + g1
                aux = b"BCZ" + cell + b"\0" + (b"" if j and rng.random() < 0.3 else b"U8Z" + umi + b"\0") + b"GEZ" + ge + b"\0"
                if rng.random() < 0.33:
                    aux += b"RNC" + bytes([int(rng.integers(1, 9))])
                aux += b"def" + struct.pack("<f", float(rng.integers(0, 50)) / 500)
                body = struct.pack("<iiBBHHHiiii", 0, int(rng.integers(10_000, 100_000_000)), len(name), 60, 4680, 3, 0x800 if j else 0, 0, -1, -1, 0) + name + cig + aux
                recs.append(struct.pack("<I", len(body)) + body)
                k += 1
        m += 1
    head = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 1) + struct.pack("<I", 5) + b"chr1\0" + struct.pack("<I", 2 ** 31 - 1)
    bam = np.frombuffer(head + b"".join(recs), dtype=np.uint8)
    csv = "".join(f"CELL{c:05d}-1\n" for c in range(n_cells))
    return csv, lib.bgzf_deflate(bam, level=1, n_threads=16), k, m


def leg_fusion(pkg, synth, ctx, dev, wl, used, res):
    """K-FUS-INSERT / K-FUS-READ / K-FUS-MOL / K-FUS-GENES + K-MTX (`FusionDetector`): a seeded tagged BAM of SMI_MB_FUS_RECS records
    (500,000: the clipped reads are a small share of a run), 5,000 cells, SMI_MB_FUS_GENES gene names (20,000), file to file: device ms per
    stage (HIP events), seconds in parse, in the device calls and in file writes, wall seconds, and beside the device's grouping the wall
    time of the reference's single-thread loops over the same pools (smi_fusion_host_loop), with the molecules on which the two differ (0)."""
    import shutil
    import tempfile

    fus = importlib.import_module(graft.PKG_NAME + ".fusiondetector")
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    n_recs = int(os.environ.get("SMI_MB_FUS_RECS", "500000"))
    n_genes = int(os.environ.get("SMI_MB_FUS_GENES", "20000"))
    t0 = time.perf_counter()
    csv, z, n_rec, n_mol = _fusion_fixture(n_recs, 5000, n_genes)
    out = {"records": n_rec, "molecules_generated": n_mol, "cells": 5000, "gene_names": n_genes, "fixture_s": time.perf_counter() - t0}
    d = tempfile.mkdtemp(prefix="fusion_")
    try:
        z.tofile(os.path.join(d, "in.bam"))
        with open(os.path.join(d, "c.csv"), "w") as f:
            f.write(csv)
        fus.fusion_detector(ctx, os.path.join(d, "in.bam"), os.path.join(d, "c.csv"), d, n_threads=16)          # the first run loads the code objects
        info = fus.fusion_detector(ctx, os.path.join(d, "in.bam"), os.path.join(d, "c.csv"), d, n_threads=16, host_loop=True)
        out["file_to_file"] = dict({k: info[k] for k in lib.FUSION_COUNTS}, stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"],
                                   bytes_written=info["bytes_written"], records_per_s=info["records"] / info["wall_s"])
        out["device_grouping_s"] = sum(info["stage_ms"][k] for k in ("insert", "read", "mol", "genes")) / 1e3
        out["host_loop_wall_s"] = info["host_loop_s"]
        out["host_loop_mismatches"] = info["host_loop_mismatches"]
        out["top_fusions"] = sorted(info["fusions"], key=lambda kv: -kv[1])[:4]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["fusion"] = out


def _fusionprep_fixture(n_recs, seed=81, clipped_share=4):
    """a seeded BAM of n_recs long reads as tagbamwithread leaves them: GE / BC / U8, US and QS of 400 .. 800 bytes cut from one random
    text, names <read>_<n>; one record in `clipped_share` carries a soft clip above MINCLIP; the reads come in groups of 1 .. 3 records of
    one name and tags (supplementary alignments), so the keys have duplicates -> (BGZF bytes, records, clipped records)"""
    import struct

    from sicelore_amd import lib

    rng = np.random.default_rng(seed)
    seq = bytes(b"ACGT"[int(x)] for x in rng.integers(0, 4, 1 << 16))
    qual = bytes(33 + int(x) for x in rng.integers(0, 40, 1 << 16))
    recs, k, r, n_clip = [], 0, 0, 0
    while k < n_recs:
        name = b"read%08d_%d\0" % (r, r % 7)
        tags = b"GEZGENE%d\0BCZCELL%05dACGTAC\0U8ZUMI%09d\0" % (r % 20000, r % 5000, r)
        for j in range(int(rng.integers(1, 4))):
            L, at = int(rng.integers(400, 801)), int(rng.integers(0, (1 << 16) - 800))
            clip = int(rng.integers(clipped_share)) == 0
            n_clip += clip
            cig = struct.pack("<3I", (int(rng.integers(151, 400)) if clip else int(rng.integers(1, 151))) << 4 | 4, 300 << 4 | 0, 20 << 4 | 4)
            aux = tags + b"USZ" + seq[at:at + L] + b"\0QSZ" + qual[at:at + L] + b"\0"
            body = struct.pack("<iiBBHHHiiii", 0, int(rng.integers(10_000, 100_000_000)), len(name), 60, 4680, 3, 0x800 if j else 0, 0, -1, -1, 0) + name + cig + aux
            recs.append(struct.pack("<I", len(body)) + body)
            k += 1
        r += 1
    head = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 1) + struct.pack("<I", 5) + b"chr1\0" + struct.pack("<I", 2 ** 31 - 1)
    return lib.bgzf_deflate(np.frombuffer(head + b"".join(recs), dtype=np.uint8), level=1, n_threads=16), k, n_clip, head


def leg_fusionprep(pkg, synth, ctx, dev, wl, used, res):
    """K-CLIP-FLAG / K-CLIP-KEY / K-CLIP-INSERT / K-CLIP-WRITE (`ExportClippedReads`) and K-NAME's '_' form + K-EDIT (`AddBamReadTags`), file
    to file: a seeded BAM of SMI_MB_FP_RECS records (100,000) with US / QS, a quarter of them clipped, the keys with duplicates, in
    segments of SMI_MB_FP_SEGMENT compressed bytes (8 MiB, so that the key table is carried over segments); then one record per written
    FASTQ name, standing in for the mapper, through AddBamReadTags.  Device ms per stage (HIP events), seconds in parse, in the device calls,
    in deflate and in file writes, wall seconds, and beside the device's decisions the wall time of the reference's single-thread loop over
    the same records (smi_clipexport_host_loop), with the records on which the two differ (0)."""
    import shutil
    import struct
    import tempfile

    fp = importlib.import_module(graft.PKG_NAME + ".fusionprep")
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    n_recs = int(os.environ.get("SMI_MB_FP_RECS", "100000"))
    seg = int(os.environ.get("SMI_MB_FP_SEGMENT", str(8 << 20)))
    t0 = time.perf_counter()
    z, n_rec, n_clip, head = _fusionprep_fixture(n_recs)
    out = {"records": n_rec, "clipped_generated": n_clip, "bam_bytes": int(z.size), "segment_bytes": seg, "fixture_s": time.perf_counter() - t0}
    d = tempfile.mkdtemp(prefix="fusionprep_")
    try:
        src, fq = os.path.join(d, "in.bam"), os.path.join(d, "clipped.fastq")
        z.tofile(src)
        fp.export_clipped_reads(ctx, src, fq, segment_bytes=seg, n_threads=16)          # the first run loads the code objects
        info = fp.export_clipped_reads(ctx, src, fq, segment_bytes=seg, n_threads=16, host_loop=True)
        out["export_clipped_reads"] = dict({k: info[k] for k in lib.CLIPEXPORT_COUNTS}, stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"],
                                           bytes_written=info["bytes_written"], records_per_s=info["records"] / info["wall_s"])
        out["host_loop_wall_s"] = info["host_loop_s"]
        out["host_loop_mismatches"] = info["host_loop_mismatches"]
        names = open(fq, "rb").read().split(b"\n")[0::4]
        recs = []
        for k, nm in enumerate(n[1:] + b"\0" for n in names if n):
            body = struct.pack("<iiBBHHHiiii", 0, 1000 + k, len(nm), 60, 4680, 1, 0, 0, -1, -1, 0) + nm + struct.pack("<I", 500 << 4) + b"NMC\1"
            recs.append(struct.pack("<I", len(body)) + body)
        lib.bgzf_deflate(np.frombuffer(head + b"".join(recs), dtype=np.uint8), level=1, n_threads=16).tofile(os.path.join(d, "mapped.bam"))
        fp.add_bam_read_tags(ctx, os.path.join(d, "mapped.bam"), os.path.join(d, "tags.bam"), segment_bytes=seg, n_threads=16)
        info = fp.add_bam_read_tags(ctx, os.path.join(d, "mapped.bam"), os.path.join(d, "tags.bam"), segment_bytes=seg, n_threads=16)
        out["add_bam_read_tags"] = dict(records=info["records"], tagged=info["tagged"], stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"],
                                        bytes_written=info["bytes_written"], records_per_s=info["records"] / info["wall_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["fusionprep"] = out


def _bamindex_fixture(n_recs, seed=91, n_ref=25, n_ops=32):
    """a seeded, coordinate-sorted BAM of n_recs records over n_ref references: names of the molecule form (<16 bases>-<12 bases>-<n>), a
    spliced CIGAR of n_ops operations (M of 20 .. 200 alternating with I, D or an N of 100 .. 5000), no sequence, one record in 500 without
    a reference at the end -> (BGZF bytes, records)"""
    from sicelore_amd import lib

    rng = np.random.default_rng(seed)
    n_un = n_recs // 500
    n = n_recs - n_un
    key = np.sort(rng.integers(0, n_ref << 27, n, dtype=np.int64))
    rec = np.zeros(n_recs, dtype=[("bs", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cig", "<u2"),
                                  ("flag", "<u2"), ("l_seq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4"), ("name", "u1", (38,)),
                                  ("cigar", "<u4", (n_ops,))])
    rec["bs"] = rec.dtype.itemsize - 4
    rec["ref"][:n], rec["pos"][:n] = key >> 27, key & ((1 << 27) - 1)
    rec["ref"][n:], rec["pos"][n:] = -1, -1
    rec["flag"][n:] = 4
    rec["l_name"], rec["mapq"], rec["bin"], rec["n_cig"], rec["nref"], rec["npos"] = 38, 60, 4680, n_ops, -1, -1
    rec["n_cig"][n:] = 0
    rec["name"][:, :30] = np.frombuffer(b"ACGTACGTACGTACGT-TTTTGGGGCCCC-", dtype=np.uint8)
    k = np.arange(n_recs, dtype=np.int64)
    for j in range(7):
        rec["name"][:, 36 - j] = 48 + (k // 10 ** j) % 10
    ops = np.where(np.arange(n_ops) % 2 == 0, 0, rng.integers(1, 4, (n_recs, n_ops)))            # M, then I / D / N
    length = np.where(ops == 0, rng.integers(20, 201, (n_recs, n_ops)), np.where(ops == 3, rng.integers(100, 5001, (n_recs, n_ops)), rng.integers(1, 6, (n_recs, n_ops))))
    rec["cigar"] = (length << 4 | ops).astype(np.uint32)
    rec["cigar"][n:] = 0                                       # (the bytes stay: records of one size; n_cigar says 0 -> they are attribute bytes no one reads)
    body = rec.view(np.uint8).reshape(n_recs, -1)
    # records without a reference carry no CIGAR: cut their rows to the 74 bytes of the fixed part and the name
    placed = body[:n].reshape(-1)
    tail = body[n:, :74].copy()
    tail[:, :4] = np.frombuffer(struct.pack("<I", 70), dtype=np.uint8)
    refs = b"".join(struct.pack("<I", len(nm) + 1) + nm + b"\0" + struct.pack("<I", 1 << 28) for nm in (b"chr%d" % (r + 1) for r in range(n_ref)))
    head = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", n_ref) + refs
    data = np.concatenate([np.frombuffer(head, dtype=np.uint8), placed, tail.reshape(-1)])
    return lib.bgzf_deflate(data, level=1, n_threads=16), n_recs


def leg_bamindex(pkg, synth, ctx, dev, wl, used, res):
    """K-BAI (`bamindex.py`, in the place of `samtools index`), file to file: a seeded, sorted BAM of SMI_MB_BAI_RECS records (2,000,000) in
    segments of SMI_MB_BAI_SEGMENT compressed bytes (64 MiB); index_bam once (after a run that loads the code objects): device ms per
    stage (HIP events), the seconds in read and inflate, in the record index, in the device calls and in the write, wall seconds.  Then
    AddBamMoleculeTags on the same file with index=False and with index=True: the difference is what the index costs as a by-product of
    the write."""
    import shutil
    import tempfile

    bi = importlib.import_module(graft.PKG_NAME + ".bamindex")
    mt = importlib.import_module(graft.PKG_NAME + ".moltags")
    n_recs = int(os.environ.get("SMI_MB_BAI_RECS", "2000000"))
    seg = int(os.environ.get("SMI_MB_BAI_SEGMENT", str(64 << 20)))
    t0 = time.perf_counter()
    z, n_rec = _bamindex_fixture(n_recs)
    out = {"records": n_rec, "bam_bytes": int(z.size), "segment_bytes": seg, "fixture_s": time.perf_counter() - t0}
    d = tempfile.mkdtemp(prefix="bamindex_")
    try:
        src = os.path.join(d, "in.bam")
        z.tofile(src)
        bi.index_bam(ctx, src, segment_bytes=seg, n_threads=16)                         # the first run loads the code objects
        info = bi.index_bam(ctx, src, segment_bytes=seg, n_threads=16)
        out["index_bam"] = dict({k: info[k] for k in ("records", "refs_with_records", "chunks", "no_coor", "segments", "blocks", "bins", "windows")},
                                stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"], bytes_written=info["bytes_written"],
                                records_per_s=info["records"] / info["wall_s"])
        dst = os.path.join(d, "tags.bam")
        mt.add_bam_molecule_tags(ctx, src, dst, segment_bytes=seg, n_threads=16)
        for name, flag in (("add_bam_molecule_tags", False), ("add_bam_molecule_tags_index", True)):
            info = mt.add_bam_molecule_tags(ctx, src, dst, segment_bytes=seg, n_threads=16, index=flag)
            out[name] = dict(records=info["records"], seconds=info["seconds"], wall_s=info["wall_s"], bytes_written=info["bytes_written"])
            if flag:
                ix = info["index"]
                out[name]["index"] = None if ix is None else dict(stage_ms=ix["stage_ms"], seconds=ix["seconds"], bytes_written=ix["bytes_written"],
                                                                  chunks=ix["chunks"], segments=ix["segments"])
                out[name]["index_error"] = info["index_error"]
        out["index_by_product_wall_s"] = out["add_bam_molecule_tags_index"]["wall_s"] - out["add_bam_molecule_tags"]["wall_s"]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["bamindex"] = out


def _bamsort_fixture(n_recs, with_seq, seed=101, n_ref=25, n_ops=8, chunk=1000):
    """a seeded BAM of n_recs records in shuffled order over n_ref references: names of the molecule form, a CIGAR of n_ops operations, no
    sequence, random strand, one record in 500 without a reference; with_seq: the attributes US:Z and QS:Z of L bytes each, L seeded in
    400 .. 800 and one L per run of `chunk` records (the rows of a run are built as one array) -> (BGZF bytes, records, inflated bytes)"""
    from sicelore_amd import lib

    rng = np.random.default_rng(seed)
    refs = b"".join(struct.pack("<I", len(nm) + 1) + nm + b"\0" + struct.pack("<I", 1 << 28) for nm in (b"chr%d" % (r + 1) for r in range(n_ref)))
    parts = [np.frombuffer(b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", n_ref) + refs, dtype=np.uint8)]
    for at in range(0, n_recs, chunk):
        m = min(chunk, n_recs - at)
        L = int(rng.integers(400, 801)) if with_seq else 0
        fields = [("bs", "<u4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cig", "<u2"), ("flag", "<u2"),
                  ("l_seq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4"), ("name", "u1", (38,)), ("cigar", "<u4", (n_ops,))]
        if with_seq:
            fields += [("us_tag", "u1", (3,)), ("us", "u1", (L + 1,)), ("qs_tag", "u1", (3,)), ("qs", "u1", (L + 1,))]
        rec = np.zeros(m, dtype=fields)
        rec["bs"] = rec.dtype.itemsize - 4
        rec["ref"], rec["pos"] = rng.integers(0, n_ref, m), rng.integers(0, 1 << 27, m)
        rec["flag"] = 16 * rng.integers(0, 2, m)
        un = rng.integers(0, 500, m) == 0
        rec["ref"][un], rec["pos"][un], rec["flag"][un] = -1, -1, 4
        rec["l_name"], rec["mapq"], rec["bin"], rec["n_cig"], rec["nref"], rec["npos"] = 38, 60, 4680, n_ops, -1, -1
        rec["name"][:, :30] = np.frombuffer(b"ACGTACGTACGTACGT-TTTTGGGGCCCC-", dtype=np.uint8)
        k = np.arange(at, at + m, dtype=np.int64)
        for j in range(7):
            rec["name"][:, 36 - j] = 48 + (k // 10 ** j) % 10
        rec["cigar"] = (rng.integers(20, 201, (m, n_ops)) << 4 | (np.arange(n_ops) % 2) * 3).astype(np.uint32)      # M and N in turn
        if with_seq:
            rec["us_tag"], rec["qs_tag"] = np.frombuffer(b"USZ", dtype=np.uint8), np.frombuffer(b"QSZ", dtype=np.uint8)
            rec["us"][:, :L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (m, L))]
            rec["qs"][:, :L] = rng.integers(35, 75, (m, L), dtype=np.uint8)
        parts.append(rec.view(np.uint8).reshape(-1))
    data = np.concatenate(parts)
    return lib.bgzf_deflate(data, level=1, n_threads=16), n_recs, int(data.size)


def leg_bamsort(pkg, synth, ctx, dev, wl, used, res):
    """K-SORT (`bamsort.py`, in the place of `samtools sort` and `samtools index`), file to file: a seeded BAM of SMI_MB_SORT_RECS records
    (2,000,000) in shuffled order, once without sequence and once with US / QS of 400 .. 800 bytes, in segments of SMI_MB_SORT_SEGMENT
    compressed bytes (64 MiB) and windows of 64 MiB; sort_bam after a run that loads the code objects, without and with index=True: device
    ms per stage (HIP events), the seconds in read and inflate, in the device calls and in the write, wall seconds; the gather's bytes per
    second from its stage time, and the same run with the gather's 4-byte stores (SMI_BAMSORT_STORE_BYTES=4); then
    smi_bamsort_host_loop: the seconds of the same sort on one host thread and its mismatch count.  The file with US / QS is sorted once
    more through runs (_bamsort_runs; `microbench.py bamsort_runs` does that part alone)."""
    import shutil
    import tempfile

    bs = importlib.import_module(graft.PKG_NAME + ".bamsort")
    segs = importlib.import_module(graft.PKG_NAME + ".bamsegments")
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    n_recs = int(os.environ.get("SMI_MB_SORT_RECS", "2000000"))
    seg = int(os.environ.get("SMI_MB_SORT_SEGMENT", str(64 << 20)))
    res["bamsort"] = {}
    for case, with_seq in (("no_sequence", False), ("us_qs_400_800", True)):
        t0 = time.perf_counter()
        z, n_rec, inflated = _bamsort_fixture(n_recs, with_seq)
        out = {"records": n_rec, "bam_bytes": int(z.size), "inflated_bytes": inflated, "segment_bytes": seg, "fixture_s": time.perf_counter() - t0}
        d = tempfile.mkdtemp(prefix="bamsort_")
        try:
            src, dst = os.path.join(d, "in.bam"), os.path.join(d, "out.bam")
            z.tofile(src)
            del z
            bs.sort_bam(ctx, src, dst, segment_bytes=seg, n_threads=16)                         # the first run loads the code objects
            for name, flag in (("sort_bam", False), ("sort_bam_index", True)):
                info = bs.sort_bam(ctx, src, dst, segment_bytes=seg, n_threads=16, index=flag)
                out[name] = dict({k: info[k] for k in ("records", "segments", "windows", "arena_bytes", "arena_held", "largest_window")},
                                 stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"], bytes_written=info["bytes_written"],
                                 gather_bytes_per_s=info["arena_bytes"] / max(info["stage_ms"]["gather"], 1e-6) * 1e3)
                if flag:
                    ix = info["index"]
                    out[name]["index"] = None if ix is None else dict(stage_ms=ix["stage_ms"], seconds=ix["seconds"], bytes_written=ix["bytes_written"])
                    out[name]["index_error"] = info["index_error"]
            os.environ["SMI_BAMSORT_STORE_BYTES"] = "4"
            try:
                info = bs.sort_bam(ctx, src, dst, segment_bytes=seg, n_threads=16)
            finally:
                del os.environ["SMI_BAMSORT_STORE_BYTES"]
            out["gather_4_byte_stores"] = dict(gather_ms=info["stage_ms"]["gather"],
                                               gather_bytes_per_s=info["arena_bytes"] / max(info["stage_ms"]["gather"], 1e-6) * 1e3)
            if with_seq:
                out["sort_bam_runs"] = _bamsort_runs(bs, ctx, d, src, seg, n_rec, inflated, out["sort_bam"]["wall_s"])
            h = None
            try:
                for bam, recs, hdr in segs.segments(src, seg, 16):
                    if hdr is not None:
                        h = lib.BamSort(ctx, len(lib.bam_header(np.frombuffer(hdr, dtype=np.uint8))[1]))
                    if recs.size:
                        h.add_segment(bam, recs)
                h.finish()
                sec, bad = h.host_loop()
                out["host_loop"] = dict(seconds=sec, mismatches=bad)
            finally:
                if h is not None:
                    h.close()
        finally:
            shutil.rmtree(d, ignore_errors=True)
        res["bamsort"][case] = out


def _bamsort_runs(bs, ctx, d, src, seg, n_rec, inflated, resident_wall_s):
    """the file at `src` sorted through runs (runs_prefix) with resident_bytes a quarter of what the resident sort needs (the record bytes
    and SMI_BAMSORT_PER_RECORD per record), so four runs or more: device ms per stage, the seconds of the run files' writes and reads among
    the others, wall seconds, their ratio to the resident sort's of the same file in the same process, and whether the two files are equal"""
    need = inflated + 48 * n_rec
    dst, ref = os.path.join(d, "runs.bam"), os.path.join(d, "out.bam")
    info = bs.sort_bam(ctx, src, dst, segment_bytes=seg, n_threads=16, resident_bytes=need // 4, runs_prefix=os.path.join(d, "spill"))
    with open(dst, "rb") as a, open(ref, "rb") as b:
        same = all(x == y for x, y in iter(lambda: (a.read(1 << 24), b.read(1 << 24)), (b"", b"")))
    return dict({k: info[k] for k in ("records", "segments", "windows", "runs", "run_bytes", "largest_run", "largest_window")}, resident_bytes=need // 4,
                stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"], bytes_written=info["bytes_written"],
                wall_over_resident=info["wall_s"] / resident_wall_s, equal_to_resident=same, left_behind=sorted(f for f in os.listdir(d) if ".run" in f))


def leg_bamsort_runs(pkg, synth, ctx, dev, wl, used, res):
    """the runs part of leg_bamsort alone: the seeded BAM with US / QS, the resident sort_bam (after a run that loads the code objects) and
    the sort through runs beside it"""
    import shutil
    import tempfile

    bs = importlib.import_module(graft.PKG_NAME + ".bamsort")
    n_recs = int(os.environ.get("SMI_MB_SORT_RECS", "2000000"))
    seg = int(os.environ.get("SMI_MB_SORT_SEGMENT", str(64 << 20)))
    t0 = time.perf_counter()
    z, n_rec, inflated = _bamsort_fixture(n_recs, True)
    out = {"records": n_rec, "bam_bytes": int(z.size), "inflated_bytes": inflated, "segment_bytes": seg, "fixture_s": time.perf_counter() - t0}
    d = tempfile.mkdtemp(prefix="bamsort_runs_")
    try:
        src, dst = os.path.join(d, "in.bam"), os.path.join(d, "out.bam")
        z.tofile(src)
        del z
        bs.sort_bam(ctx, src, dst, segment_bytes=seg, n_threads=16)                             # the first run loads the code objects
        info = bs.sort_bam(ctx, src, dst, segment_bytes=seg, n_threads=16)
        out["sort_bam"] = dict({k: info[k] for k in ("records", "segments", "windows", "arena_bytes", "largest_window")}, stage_ms=info["stage_ms"],
                               seconds=info["seconds"], wall_s=info["wall_s"], bytes_written=info["bytes_written"])
        out["sort_bam_runs"] = _bamsort_runs(bs, ctx, d, src, seg, n_rec, inflated, info["wall_s"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["bamsort_runs"] = out


def _samview_fixture(path, n_recs, with_seq, seed=111, n_ref=25, n_ops=8, chunk=1000):
    """the record mix of _bamsort_fixture as SAM text at `path`: names of the molecule form, a CIGAR of n_ops operations (M and N in turn),
    random strand, one line in 500 unmapped (flag 4, placed on a reference as mappers place a mate); with_seq: SEQ and QUAL of L bases, L seeded in 400 .. 800 and one L per run of
    `chunk` lines (the rows of a run are built as one array; numbers stand zero-padded in fixed columns), else * and * -> bytes written"""
    rng = np.random.default_rng(seed)
    tab = np.uint8(9)
    written = 0

    def digits(col, v, n):
        for j in range(n):
            col[:, n - 1 - j] = 48 + (v // 10 ** j) % 10

    with open(path, "wb") as f:
        written += f.write(b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:chr%02d\tLN:%d\n" % (r + 1, 1 << 28) for r in range(n_ref)))
        for at in range(0, n_recs, chunk):
            m = min(chunk, n_recs - at)
            L = int(rng.integers(400, 801)) if with_seq else 1
            fields = [("name", "u1", (37,)), ("t0", "u1"), ("flag", "u1", (2,)), ("t1", "u1"), ("ref", "u1", (5,)), ("t2", "u1"), ("pos", "u1", (9,)), ("t3", "u1"),
                      ("mapq", "u1", (2,)), ("t4", "u1"), ("cigar", "u1", (n_ops, 4)), ("t5", "u1"), ("mate", "u1", (6,)), ("seq", "u1", (L,)), ("t9", "u1"),
                      ("qual", "u1", (L,)), ("lf", "u1")]
            row = np.zeros(m, dtype=fields)
            for t in ("t0", "t1", "t2", "t3", "t4", "t5", "t9"):
                row[t] = tab
            row["lf"] = 10
            row["name"][:, :30] = np.frombuffer(b"ACGTACGTACGTACGT-TTTTGGGGCCCC-", dtype=np.uint8)
            digits(row["name"][:, 30:], np.arange(at, at + m, dtype=np.int64), 7)
            un = rng.integers(0, 500, m) == 0
            digits(row["flag"], np.where(un, 4, 16 * rng.integers(0, 2, m)), 2)
            row["ref"][:, :3] = np.frombuffer(b"chr", dtype=np.uint8)
            digits(row["ref"][:, 3:], rng.integers(1, n_ref + 1, m), 2)
            digits(row["pos"], rng.integers(1, 1 << 27, m), 9)
            row["mapq"] = np.frombuffer(b"60", dtype=np.uint8)
            for k in range(n_ops):
                digits(row["cigar"][:, k, :3], rng.integers(20, 201, m), 3)
                row["cigar"][:, k, 3] = ord("N") if k % 2 else ord("M")
            row["mate"] = np.frombuffer(b"*\t0\t0\t", dtype=np.uint8)
            if with_seq:
                row["seq"] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (m, L))]
                row["qual"] = rng.integers(35, 75, (m, L), dtype=np.uint8)
            else:
                row["seq"] = row["qual"] = ord("*")
            written += f.write(row.view(np.uint8).tobytes())
    return written


def leg_samview(pkg, synth, ctx, dev, wl, used, res):
    """K-SAM (`samview.py`, in the place of `samtools view -bS`), file to file: a seeded SAM text of SMI_MB_VIEW_LINES lines (2,000,000), once
    without sequence and once with SEQ and QUAL of 400 .. 800 bases, in segments of SMI_MB_VIEW_SEGMENT bytes (256 MiB); sam_to_bam after a
    run that loads the code objects: device ms per stage (HIP events), the seconds in the read, in the device calls and in the write, wall
    seconds; the text bytes per second through the size and the write pass from their stage times; then smi_samview_host_loop per segment:
    the seconds of the same conversion on one host thread and its mismatch count."""
    import shutil
    import tempfile

    sv = importlib.import_module(graft.PKG_NAME + ".samview")
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    n_lines = int(os.environ.get("SMI_MB_VIEW_LINES", "2000000"))
    seg = int(os.environ.get("SMI_MB_VIEW_SEGMENT", str(256 << 20)))
    res["samview"] = {}
    for case, with_seq in (("no_sequence", False), ("seq_qual_400_800", True)):
        d = tempfile.mkdtemp(prefix="samview_")
        try:
            src, dst = os.path.join(d, "in.sam"), os.path.join(d, "out.bam")
            t0 = time.perf_counter()
            n_bytes = _samview_fixture(src, n_lines, with_seq)
            out = {"lines": n_lines, "sam_bytes": n_bytes, "segment_bytes": seg, "fixture_s": time.perf_counter() - t0}
            sv.sam_to_bam(ctx, src, dst, segment_bytes=seg)                                     # the first run loads the code objects
            info = sv.sam_to_bam(ctx, src, dst, segment_bytes=seg)
            ms = info["stage_ms"]
            out["sam_to_bam"] = dict({k: info[k] for k in ("records", "segments", "text_bytes", "record_bytes")}, stage_ms=ms, seconds=info["seconds"],
                                     wall_s=info["wall_s"], bytes_written=info["bytes_written"],
                                     size_text_bytes_per_s=info["text_bytes"] / max(ms["size"], 1e-6) * 1e3,
                                     write_text_bytes_per_s=info["text_bytes"] / max(ms["write"], 1e-6) * 1e3)
            h = None
            try:
                sec = bad = 0
                with open(src, "rb") as f:
                    pieces = sv.text_segments(f, seg)
                    h = lib.SamView(ctx, next(pieces))
                    for piece in pieces:
                        h.add_segment(piece)
                        h.convert()
                        s, b = h.host_loop()
                        sec, bad = sec + s, bad + b
                out["host_loop"] = dict(seconds=sec, mismatches=bad)
            finally:
                if h is not None:
                    h.close()
        finally:
            shutil.rmtree(d, ignore_errors=True)
        res["samview"][case] = out


def _snp_fixture(n_recs, n_lines, n_cells, seed=51):
    """a seeded molecule BAM of n_recs fixed-size records (aM bD cM over 200 bases, BC / U8 / RN, both strands, two chromosomes, unsorted)
    around n_lines sites of 1..4 positions each -> (SNP text, cell list, BGZF bytes, inflated bytes)"""
    import struct

    from sicelore_amd import lib

    rng = np.random.default_rng(seed)
    site_ref = rng.integers(0, 2, n_lines)
    site_pos = rng.integers(10_000, 50_000_000, n_lines)
    lines = []
    for i in range(n_lines):
        pos = site_pos[i] + rng.choice(150, int(rng.integers(1, 5)), replace=False)
        lines.append(f"chr{site_ref[i] + 1},{'|'.join(map(str, pos))},{'-' if rng.random() < 0.5 else '+'},site{i}\n")
    L = 200
    rec = np.zeros((n_recs, 392), dtype=np.uint8)     # 4 + 32 fixed, name 11, CIGAR 12, bases 100, qualities 200, attributes 33
    s = rng.integers(0, n_lines, n_recs)

    def put(col, values, dtype):
        rec[:, col:col + np.dtype(dtype).itemsize] = np.ascontiguousarray(np.asarray(values).astype(dtype)).view(np.uint8).reshape(n_recs, -1)

    def digits(col, values, width):
        for k in range(width):
            rec[:, col + width - 1 - k] = 48 + (values // 10 ** k) % 10
    put(0, np.full(n_recs, 388), "<u4")
    put(4, site_ref[s], "<i4")
    put(8, site_pos[s] - rng.integers(0, 150, n_recs) - 1, "<i4")
    rec[:, 12], rec[:, 13] = 11, 60
    put(14, np.full(n_recs, 4680), "<u2")
    put(16, np.full(n_recs, 3), "<u2")
    put(18, np.where(rng.random(n_recs) < 0.5, 16, 0), "<u2")
    put(20, np.full(n_recs, L), "<i4")
    put(24, np.full(n_recs, -1), "<i4")
    put(28, np.full(n_recs, -1), "<i4")
    rec[:, 36] = ord("r")
    digits(37, np.arange(n_recs), 9)
    a = rng.integers(20, 180, n_recs)
    put(47, a << 4, "<u4")
    put(51, rng.integers(1, 20, n_recs) << 4 | 2, "<u4")
    put(55, (L - a) << 4, "<u4")
    code = np.array([1, 2, 4, 8], dtype=np.uint8)
    rec[:, 59:159] = code[rng.integers(0, 4, (n_recs, 100))] << 4 | code[rng.integers(0, 4, (n_recs, 100))]
    rec[:, 159:359] = rng.integers(2, 41, (n_recs, L), dtype=np.uint8)
    rec[:, 359:366] = np.frombuffer(b"BCZCELL", dtype=np.uint8)
    digits(366, rng.integers(0, n_cells, n_recs), 5)
    rec[:, 371:373] = np.frombuffer(b"-1", dtype=np.uint8)
    rec[:, 374:378] = np.frombuffer(b"U8ZU", dtype=np.uint8)
    digits(378, rng.integers(0, 10 ** 9, n_recs), 9)
    rec[:, 388:391] = np.frombuffer(b"RNC", dtype=np.uint8)
    rec[:, 391] = rng.integers(1, 9, n_recs)
    head = b"BAM\1" + struct.pack("<I", 0) + struct.pack("<I", 2) + b"".join(struct.pack("<I", 5) + nm + struct.pack("<I", 2 ** 31 - 1)
                                                                              for nm in (b"chr1\0", b"chr2\0"))
    bam = np.concatenate([np.frombuffer(head, dtype=np.uint8), rec.reshape(-1)])
    csv = "".join(f"CELL{c:05d}-1\n" for c in range(n_cells))
    return "".join(lines), csv, lib.bgzf_deflate(bam, level=1, n_threads=16), int(bam.size)


def leg_bamview(pkg, synth, ctx, dev, wl, used, res):
    """K-VIEW (`bamview.py`, in the place of `samtools view in.bam [region ...]`), file to file: _bamsort_fixture's seeded BAMs of
    SMI_MB_VIEW_RECS records (2,000,000) over 25 references, once without sequence and once with US / QS of 400 .. 800 bytes, sorted with
    sort_bam and indexed with index_bam; view_bam after a run that loads the code objects, three ways: one reference of the 25, 1,000
    seeded regions, and no region with -F 4: device ms per stage (HIP events), the ranges, blocks and compressed bytes read against the
    file's, the seconds in read and inflate, in the record index, in the device calls and in the write, wall seconds, and wall seconds
    with index=True; then smi_bamview_host_loop on every segment of the 1,000-region query: the seconds of the same test and copy on one
    host thread and its mismatch count."""
    import shutil
    import tempfile

    bs = importlib.import_module(graft.PKG_NAME + ".bamsort")
    bi = importlib.import_module(graft.PKG_NAME + ".bamindex")
    bv = importlib.import_module(graft.PKG_NAME + ".bamview")
    segs = importlib.import_module(graft.PKG_NAME + ".bamsegments")
    lib = importlib.import_module(graft.PKG_NAME + ".lib")
    n_recs = int(os.environ.get("SMI_MB_VIEW_RECS", "2000000"))
    seg = int(os.environ.get("SMI_MB_VIEW_SEGMENT", str(64 << 20)))
    rng = np.random.default_rng(211)
    regions = []
    for _ in range(1000):
        beg = int(rng.integers(0, 1 << 27))
        regions.append((int(rng.integers(0, 25)), beg, beg + 1 + int(rng.integers(0, 1 << int(rng.integers(1, 18))))))
    queries = (("one_reference", ["chr13"], {}), ("regions_1000", regions, {}), ("no_region_F4", [], dict(exclude=4)))
    res["bamview"] = {}
    for case, with_seq in (("no_sequence", False), ("us_qs_400_800", True)):
        t0 = time.perf_counter()
        z, n_rec, inflated = _bamsort_fixture(n_recs, with_seq)
        d = tempfile.mkdtemp(prefix="bamview_")
        try:
            unsorted, src, dst = os.path.join(d, "unsorted.bam"), os.path.join(d, "in.bam"), os.path.join(d, "out.bam")
            z.tofile(unsorted)
            del z
            bs.sort_bam(ctx, unsorted, src, segment_bytes=seg, n_threads=16)
            os.remove(unsorted)
            bi.index_bam(ctx, src, segment_bytes=seg, n_threads=16)
            out = {"records": n_rec, "bam_bytes": os.path.getsize(src), "bai_bytes": os.path.getsize(src + ".bai"), "inflated_bytes": inflated,
                   "segment_bytes": seg, "fixture_s": time.perf_counter() - t0}
            bv.view_bam(ctx, src, dst, ["chr1:1-100000"], segment_bytes=seg, n_threads=16)          # the first run loads the code objects
            for name, asked, filters in queries:
                for flag in (False, True):
                    info = bv.view_bam(ctx, src, dst, asked, segment_bytes=seg, n_threads=16, index=flag, **filters)
                    if not flag:
                        out[name] = dict({k: info[k] for k in lib.BAMVIEW_COUNTS + ("ranges", "blocks_read", "compressed_bytes_read")},
                                         stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"], bytes_written=info["bytes_written"],
                                         read_fraction=info["compressed_bytes_read"] / out["bam_bytes"],
                                         gather_bytes_per_s=info["bytes_kept"] / max(info["stage_ms"]["gather"], 1e-6) * 1e3)
                    else:
                        out[name]["wall_s_with_index"] = info["wall_s"]
                        out[name]["index_error"] = info["index_error"]
            merged = bv.merge_regions(regions)
            with open(src + ".bai", "rb") as f:
                spans = bv.query_ranges(bv.read_bai(f.read()), merged)
            h = lib.BamView(ctx, 25, merged)
            try:
                sec = bad = n = 0
                for bam, recs in segs.ranges(src, spans, seg, 16):
                    h.add_segment(bam, recs)
                    h.convert()
                    s1, b1 = h.host_loop()
                    sec, bad, n = sec + s1, bad + b1, n + 1
                out["host_loop"] = dict(seconds=sec, mismatches=bad, segments=n, records=h.counts()["records"])
            finally:
                h.close()
        finally:
            shutil.rmtree(d, ignore_errors=True)
        res["bamview"][case] = out


def leg_snp(pkg, synth, ctx, dev, wl, used, res):
    """K-SNP + K-MTX (`SNPMatrix`): a seeded molecule BAM of SMI_MB_SNP_RECS records (2,000,000) against SMI_MB_SNP_LINES site lines (4,000) of
    1..4 positions, 5,000 cells, file to file: device ms of K-SNP (both launches and the scans, all segments), sorts + de-duplication + RLE and
    render (HIP events), wall seconds per phase.  snp_gbytes_per_s: the inflated BAM bytes, once per launch, over K-SNP's device time -- the
    bytes the kernel is handed, an upper bound of what it reads (it skips the bases and qualities it is not asked for)."""
    import shutil
    import tempfile

    snp = importlib.import_module(graft.PKG_NAME + ".snpmatrix")
    n_recs = int(os.environ.get("SMI_MB_SNP_RECS", "2000000"))
    n_lines = int(os.environ.get("SMI_MB_SNP_LINES", "4000"))
    t0 = time.perf_counter()
    text, csv, z, inflated = _snp_fixture(n_recs, n_lines, 5000)
    out = {"records": n_recs, "lines": n_lines, "cells": 5000, "inflated_bytes": inflated, "fixture_s": time.perf_counter() - t0}
    d = tempfile.mkdtemp(prefix="snp_")
    try:
        z.tofile(os.path.join(d, "in.bam"))
        with open(os.path.join(d, "s.csv"), "w") as f:
            f.write(text)
        with open(os.path.join(d, "c.csv"), "w") as f:
            f.write(csv)
        runs = []
        for _rep in range(2):          # the first run loads the code objects
            info = snp.snp_matrix(ctx, os.path.join(d, "in.bam"), os.path.join(d, "c.csv"), os.path.join(d, "s.csv"), d, n_threads=16)
            keys = ("records", "lines", "pairs", "hits", "lowRN", "lowQV", "kept", "rows", "total_count", "render_blocks")
            runs.append(dict({k: info[k] for k in keys}, stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"],
                             bytes_written=info["bytes_written"], records_per_s=info["records"] / info["wall_s"],
                             snp_gbytes_per_s=2 * inflated / (info["stage_ms"]["snp"] * 1e-3) / 1e9))
        out["first_run"], out["file_to_file"] = runs
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["snp"] = out


def _dedup_fixture(n_recs, seq_len, seed=61):
    """a consensus FASTQ as ComputeConsensus writes it (`@BC16-UMI12-rn`), records of one width so that numpy can lay it out: about 10 % of the
    records repeat the key of another, rn 10 .. 99, in shuffled order -> uint8 array"""
    rng = np.random.default_rng(seed)
    n_keys = n_recs - n_recs // 10
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    keys = acgt[rng.integers(0, 4, size=(n_keys, 28), dtype=np.uint8)]
    which = np.concatenate([np.arange(n_keys), rng.integers(0, n_keys, size=n_recs - n_keys)])
    rng.shuffle(which)
    width = 1 + 16 + 1 + 12 + 1 + 2 + 1 + seq_len + 3 + seq_len + 1
    text = np.empty((n_recs, width), dtype=np.uint8)
    text[:, 0] = ord("@")
    text[:, 1:17] = keys[which, :16]
    text[:, 17] = ord("-")
    text[:, 18:30] = keys[which, 16:]
    text[:, 30] = ord("-")
    rn = rng.integers(10, 100, size=n_recs)
    text[:, 31] = ord("0") + rn // 10
    text[:, 32] = ord("0") + rn % 10
    text[:, 33] = ord("\n")
    text[:, 34:34 + seq_len] = acgt[rng.integers(0, 4, size=(n_recs, seq_len), dtype=np.uint8)]
    text[:, 34 + seq_len:37 + seq_len] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    text[:, 37 + seq_len:37 + 2 * seq_len] = rng.integers(33, 74, size=(n_recs, seq_len), dtype=np.uint8)
    text[:, -1] = ord("\n")
    return text.reshape(-1), n_keys


def leg_dedup(pkg, synth, ctx, dev, wl, used, res):
    """K-DD-* (`DeduplicateMolecule`): a seeded FASTQ of SMI_MB_DEDUP_RECS records (2,000,000) of SMI_MB_DEDUP_LEN bases (300), about 10 % of them
    with the key of another record, file to file in segments of 256 MiB: device ms per stage (HIP events, all segments together) and wall
    seconds per pass.  The text goes to the device twice, once per pass; text_gbytes_per_s is the file size over the wall time."""
    import shutil
    import tempfile

    dd = importlib.import_module(graft.PKG_NAME + ".dedupmolecule")
    n_recs = int(os.environ.get("SMI_MB_DEDUP_RECS", "2000000"))
    seq_len = int(os.environ.get("SMI_MB_DEDUP_LEN", "300"))
    t0 = time.perf_counter()
    text, n_keys = _dedup_fixture(n_recs, seq_len)
    out = {"records": n_recs, "keys": n_keys, "seq_len": seq_len, "text_bytes": int(text.size), "fixture_s": time.perf_counter() - t0}
    d = tempfile.mkdtemp(prefix="dedup_")
    try:
        text.tofile(os.path.join(d, "in.fq"))
        del text
        runs = []
        for _rep in range(2):          # the first run loads the code objects
            info = dd.deduplicate_molecule(ctx, os.path.join(d, "in.fq"), os.path.join(d, "out.fq"))
            keys = ("lines", "records", "molecules", "segments", "table_slots", "probe_steps", "wraps", "bytes_written")
            runs.append(dict({k: info[k] for k in keys}, stage_ms=info["stage_ms"], seconds=info["seconds"], wall_s=info["wall_s"],
                             records_per_s=info["records"] / info["wall_s"], text_gbytes_per_s=out["text_bytes"] / info["wall_s"] / 1e9))
        out["first_run"], out["file_to_file"] = runs
    finally:
        shutil.rmtree(d, ignore_errors=True)
    res["dedup"] = out


def leg_inflate(pkg, synth, ctx, dev, wl, used, res):
    """K-INFLATE: 64 gzip files of FASTQ text (zlib level 6 and level 1, qualities uniform over 29 values per base) resident in HBM -> their
    text in HBM; against zlib on one host thread"""
    import ctypes
    import zlib
    from concurrent.futures import ThreadPoolExecutor

    n = int(os.environ.get("SMI_MB_READS", "500000"))
    n_files = int(os.environ.get("SMI_MB_FILES", "64"))
    rd = synth.gen_reads(n, used, seed=9, device=dev, q_mean=20.0)
    text = synth.fastq_text_device(rd)[0]
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    is_q = text == ord("I")
    text[is_q] = torch.randint(35, 64, (int(is_q.sum()),), device=dev, generator=g, dtype=torch.int32).to(torch.uint8)
    host = text.cpu().numpy()
    del rd, is_q, text
    cuts = np.linspace(0, host.size, n_files + 1).astype(np.int64)
    parts = [host[cuts[i]:cuts[i + 1]] for i in range(n_files)]
    for level in (6, 1):
        def gz(a, level=level):
            c = zlib.compressobj(level, zlib.DEFLATED, 31)
            return c.compress(memoryview(a)) + c.flush()

        with ThreadPoolExecutor(16) as pool:
            files = list(pool.map(gz, parts))
        t0 = time.perf_counter()
        zlib.decompress(files[0], wbits=31)
        t_zlib = time.perf_counter() - t0
        in_off, at = [], 0
        for f in files:
            in_off.append(at)
            at = (at + len(f) + 511) & ~511
        hbuf = np.zeros(at + 1024, dtype=np.uint8)
        for f, o in zip(files, in_off):
            hbuf[o:o + len(f)] = np.frombuffer(f, dtype=np.uint8)
        d_in = torch.from_numpy(hbuf).to(dev)
        out_off, at = [], 0
        for p in parts:
            out_off.append(at)
            at = (at + p.size + 255) & ~255
        d_out = torch.zeros(at, dtype=torch.uint8, device=dev)
        S = np.zeros((n_files, 4), dtype=np.uint64)
        S[:, 0], S[:, 1], S[:, 2], S[:, 3] = in_off, [len(f) for f in files], out_off, [p.size for p in parts]
        R = np.zeros(n_files, dtype=np.dtype([("out_len", "<u8"), ("status", "<u4"), ("n_members", "<u4")]))

        def run():
            ctx._check(ctx._lib.smi_gz_inflate_device(ctx._h, d_in.data_ptr(), S.ctypes.data, n_files, d_out.data_ptr(), R.ctypes.data, None))

        dt = timed(run, reps=3)
        assert (R["status"] == 0).all(), R["status"]
        got = d_out.cpu().numpy()
        assert all((got[o:o + p.size] == p).all() for o, p in zip(out_off, parts))
        res[f"gz_inflate_device_level{level}"] = {"files": n_files, "gz_bytes": int(sum(len(f) for f in files)), "text_bytes": int(host.size), "ms": dt * 1e3,
                                                  "text_GBps": host.size / dt / 1e9, "text_MBps_per_file": host.size / dt / 1e6 / n_files,
                                                  "zlib_one_thread_text_MBps": parts[0].size / t_zlib / 1e6,
                                                  "note": "one call: kernel, CRC-32 check of every member, results on the host"}


def leg_packed(pkg, synth, ctx, dev, wl, used, res):
    """host text -> host text through the PACKED boundary (smi_scanfastq_pass2_chunk_packed: index / bit-planes / records on host threads,
    0.7 KB per read over the link instead of 5 KB), one lane with T threads and several lanes sharing the box's host cores"""
    import threading

    from sicelore_amd import lib as libmod

    n = int(os.environ.get("SMI_MB_READS", "500000"))
    rd = synth.gen_reads(n, used, seed=9, device=dev)
    text, buf, offs = synth.fastq_text_device(rd)
    total = int(text.numel())
    del rd, buf
    ctx.set_barcode_set_device(used.to(torch.int32), mode=0)
    pin = libmod.PinnedBuffer(total)
    pin.array[:] = text.cpu().numpy()
    del text
    cores = len(os.sched_getaffinity(0))
    try:
        q = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q[0] == "max" else float(q[0]) / float(q[1])
    except Exception:
        quota = None
    out = {"reads_per_chunk": n, "text_bytes": total, "host_cpus_visible": cores, "host_cpu_quota": quota, "runs": []}
    pt, ft, _ = ctx.scanfastq_pass2_chunk(pin.array, copy=True)                       # the text worker: the bytes to match
    pp, fp, info = ctx.scanfastq_pass2_chunk(pin.array, copy=True, packed=True, n_threads=16)
    out["equals_text_worker"] = bool(pt == pp and ft == fp)
    out["text_out_bytes"] = len(pp) + len(fp)
    os.environ["SMI_PK_TIMING"] = "1"
    ctx.scanfastq_pass2_chunk(pin.array, copy=False, packed=True, n_threads=16)      # stages of one call on stderr
    del os.environ["SMI_PK_TIMING"]
    for lanes, threads in ((1, 16), (1, 32), (2, 8), (2, 16), (4, 4), (4, 8), (8, 2), (8, 4), (16, 1), (16, 2)):
        ctxs = [ctx] + [ctx.lane() for _ in range(lanes - 1)]
        pins = [pin] + [libmod.PinnedBuffer(total) for _ in range(lanes - 1)]
        for pb in pins[1:]:
            pb.array[:] = pin.array
        for c, pb in zip(ctxs, pins):
            c.scanfastq_pass2_chunk(pb.array, copy=False, packed=True, n_threads=threads)   # warm-up: arena, pinned buffers
        per = 3

        def worker(c, pb):
            for _ in range(per):
                c.scanfastq_pass2_chunk(pb.array, copy=False, packed=True, n_threads=threads)

        th = [threading.Thread(target=worker, args=(c, pb)) for c, pb in zip(ctxs, pins)]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        dt = time.perf_counter() - t0
        out["runs"].append({"lanes": lanes, "threads_per_lane": threads, "reads_per_s": n * lanes * per / dt, "ms_per_chunk": dt / per * 1e3})
        for c in ctxs[1:]:
            c.close()
        for pb in pins[1:]:
            pb.close()
    pin.close()
    out["best"] = max(out["runs"], key=lambda r: r["reads_per_s"])
    res["pass2_chunk_packed_host_to_host"] = out


if __name__ == "__main__":
    main()
