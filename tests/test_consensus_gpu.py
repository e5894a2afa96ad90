"""ComputeConsensus on the device (K-POA, smi_consensus.hip) against tests/consensusmodel.py: smi_poa_batch byte for byte, the file to
file path on BAMs that exercise every filter, and the sicelore-nf command lines through bin/java."""
import gzip
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bammodel
import consensusmodel as cm
import tagbammodel as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:100000\n@SQ\tSN:chr2\tLN:100000\n"
REFS = [("chr1", 100000), ("chr2", 100000)]


@pytest.fixture(scope="module")
def lib(pkg):
    return importlib.import_module("sicelore_amd.lib")


@pytest.fixture(scope="module")
def cc(pkg):
    return importlib.import_module("sicelore_amd.computeconsensus")


def batch(mols):
    seqs = b"".join(r for m in mols for r in m)
    read_off = np.zeros(sum(len(m) for m in mols) + 1, dtype=np.uint64)
    read_off[1:] = np.cumsum([len(r) for m in mols for r in m])
    mol_off = np.zeros(len(mols) + 1, dtype=np.int32)
    mol_off[1:] = np.cumsum([len(m) for m in mols])
    return np.frombuffer(seqs, dtype=np.uint8).copy(), read_off, mol_off


def check_poa(lib, ctx, mols, max_ps=20, **kw):
    cons, qvs, ms, rerun = lib.poa_batch(ctx, *batch(mols), max_ps=max_ps, **kw)
    for i, m in enumerate(mols):
        want, same = cm.poa(m)
        wq = bytes(cm.qv_byte(s, len(m), max_ps) for s in same)
        assert (cons[i], qvs[i]) == (want, wq), f"molecule {i}: {len(m)} reads of {[len(r) for r in m]} bases"
    return rerun


def noisy_molecule(rng, n_reads, length, rate=0.07, alphabet=b"ACGT"):
    src = cm.random_seq(rng, length, alphabet)
    return [cm.noisy_copy(rng, src, rate, alphabet) for _ in range(n_reads)]


def test_poa_noisy_molecules(lib, gpu_ctx):
    rng = np.random.default_rng(101)
    mols = [noisy_molecule(rng, int(rng.integers(3, 21)), int(rng.integers(50, 801))) for _ in range(12)]
    check_poa(lib, gpu_ctx, mols)


def test_poa_unequal_lengths_ns_and_tiny_reads(lib, gpu_ctx):
    rng = np.random.default_rng(102)
    src = cm.random_seq(rng, 400)
    mols = [
        [src, src[100:180], cm.noisy_copy(rng, src[:250]), src[300:], cm.random_seq(rng, 60) + src[50:350] + cm.random_seq(rng, 90)],  # local tails
        [b"A", b"A", b"C"], [b"A", b"", b"G", b"A"], [b"", b"", b""], [b"ACGTN" * 20, b"ACGTNN" * 15, b"NNNN" + b"ACGTN" * 20],
        noisy_molecule(rng, 6, 300, 0.1, b"ACGTN"), [cm.random_seq(rng, 700), cm.random_seq(rng, 50), cm.random_seq(rng, 700)],
        noisy_molecule(rng, 20, 800, 0.15), [src] * 7,
    ]
    check_poa(lib, gpu_ctx, mols, max_ps=30)


def test_poa_batch_of_2000_mixed_molecules(lib, gpu_ctx):
    rng = np.random.default_rng(103)
    mols = []
    for i in range(2000):
        k = int(rng.integers(1, 7)) if i % 50 else int(rng.integers(10, 21))
        mols.append(noisy_molecule(rng, k, int(rng.integers(20, 120)) if i % 50 else 300))
    check_poa(lib, gpu_ctx, mols)


def _outgrows_estimate(reads):
    """the model's graph sizes: True when some read is aligned against more nodes than the first pass allows (3 x the longest read)"""
    g, cap = cm.Graph(), 3 * max(len(r) for r in reads)
    grows = False
    for r in reads:
        grows |= len(g.base) > cap and len(r) > 0
        cm.add_read(g, r, cm.align(g, r))
    return grows


def test_poa_graphs_that_outgrow_the_estimate_run_again(lib, gpu_ctx):
    """unrelated 100-base reads: the graph passes 3 x 100 nodes at the 4th or 5th read, the molecule overflows its first slot and is run
    again in a slot of its worst case; every molecule of the batch has reads of exactly 100 bases, so all share one slot size and the
    model says exactly which ones overflow"""
    rng = np.random.default_rng(104)
    mols = [[cm.random_seq(rng, 100) for _ in range(10)] for _ in range(6)]
    mols += [[cm.random_seq(rng, 100)] * 3, [cm.random_seq(rng, 100) for _ in range(3)]]      # these two stay inside the estimate
    want = sum(_outgrows_estimate(m) for m in mols)
    assert want == 6
    assert check_poa(lib, gpu_ctx, mols) == want


def test_poa_int32_rows_for_reads_over_6000_bases(lib, gpu_ctx):
    rng = np.random.default_rng(106)
    src = cm.random_seq(rng, 6100)
    mols = [[src, cm.noisy_copy(rng, src[1000:1300]), cm.noisy_copy(rng, src[5800:6100]), src[3000:3100]],
            [cm.random_seq(rng, 6001), cm.random_seq(rng, 40), cm.random_seq(rng, 40)], noisy_molecule(rng, 5, 200)]
    assert check_poa(lib, gpu_ctx, mols) == 0


def test_poa_molecule_larger_than_the_budget_fails_by_index(lib, gpu_ctx):
    rng = np.random.default_rng(105)
    mols = [noisy_molecule(rng, 3, 50), noisy_molecule(rng, 10, 2000)]
    with pytest.raises(lib.SmiError, match=r"molecule 1 \(10 reads"):
        lib.poa_batch(gpu_ctx, *batch(mols), scratch_bytes=8 << 20)


def _bam_file(tmp_path, records, block=0xFF00):
    bam = bammodel.bam_bytes(HEAD, REFS, records)
    p = tmp_path / "in.bam"
    p.write_bytes(bammodel.bgzf_compress(bam, block=block))
    return bam, p


def _molecule_records(rng, n_mol, reads_per, length, seed_names="m", first=0):
    recs = []
    for m in range(first, first + n_mol):
        src = cm.random_seq(rng, length)
        k = reads_per if isinstance(reads_per, int) else int(rng.integers(*reads_per))
        for r in range(k):
            seq = cm.noisy_copy(rng, src).decode()
            us = "TTTTTTTT" + seq + "AAAAAAAAAAGG"
            aux = tm.aux_z("BC", f"CELL{m % 7:02d}-1") + tm.aux_z("U8", f"UMI{m:05d}") + tm.aux_z("US", us) + tm.aux_int("TE", "C", 8)
            aux += tm.aux_int("PS", "S", 8 + len(seq)) + tm.aux_f("de", float(rng.integers(0, 5)) / 100)
            recs.append(bammodel.bam_record(f"{seed_names}{m}_{r}", 0, m % 2, 100 + m, 60, [("S", 8), ("M", len(seq)), ("S", 12)], "ACGT", aux=aux))
    return recs


def _filters_records(rng):
    recs = _molecule_records(rng, 30, (1, 8), 150)
    z = lambda t, v: tm.aux_z(t, v)  # noqa: E731
    recs += [
        bammodel.bam_record("f_nobc", 0, 0, 5, 60, [("M", 4)], "ACGT", aux=z("U8", "X") + z("US", "ACGTAC")),
        bammodel.bam_record("f_unmapped", 4, -1, -1, 0, [("M", 4)], "ACGT", aux=z("BC", "B") + z("U8", "X") + z("US", "ACGTAC")),
        bammodel.bam_record("f_chim", 0, 0, 5, 60, [("H", 200), ("M", 4)], "ACGT", aux=z("BC", "B") + z("U8", "X")),
        bammodel.bam_record("f_chim2", 0, 0, 5, 60, [("M", 4), ("S", 151)], "ACGT", aux=z("BC", "B") + z("U8", "X") + z("US", "ACGTAC")),
        bammodel.bam_record("f_noumi", 0, 0, 5, 60, [("M", 4)], "ACGT", aux=z("BC", "B") + z("US", "ACGTAC")),
        bammodel.bam_record("f_sec0", 256, 0, 5, 0, [("M", 4)], "ACGT", aux=z("BC", "B") + z("U8", "X") + z("US", "ACGTACGT")),
        bammodel.bam_record("f_cs", 0, 0, 5, 60, [("M", 4)], "ACGT", aux=z("BC", "B-1") + z("U8", "X") + z("CS", "GATTACA") + tm.aux_int("TE", "i", 2)),
        bammodel.bam_record("f_df", 2048, 1, 5, 3, [("M", 4)], "ACGT", aux=z("BC", "B") + z("U8", "X") + z("US", "CCCCGGGG") + tm.aux_f("df", 0.01)),
        bammodel.bam_record("f_cs", 256, 0, 5, 60, [("M", 4)], "ACGT", aux=z("BC", "B") + z("U8", "X") + z("CS", "GATTACAT") + tm.aux_f("de", 2.0)),
    ]
    us = "TTTTACGTACGTAAAAGG"
    edge = lambda name, aux, cigar=None, umi="EDGE": bammodel.bam_record(name, 0, 0, 5, 60, cigar or [("M", 4)], "ACGT",  # noqa: E731
                                                                       aux=z("BC", "AC-1GT-1-1") + z("U8", umi) + aux)
    recs += [
        edge("e_ps_end", z("US", us) + tm.aux_int("TE", "c", 4) + tm.aux_int("PS", "S", 17)),              # PS >= len-1: end = len-1
        edge("e_te_end", z("US", us) + tm.aux_int("TE", "C", 12) + tm.aux_int("PS", "i", 12)),            # TE >= end: the whole US
        edge("e_empty", z("US", "") + tm.aux_int("TE", "i", 0)),                                           # empty US: an empty cDNA
        edge("e_clip150", z("US", us), cigar=[("H", 150), ("M", 4), ("S", 150)]),                          # clips of exactly MAXCLIP
        edge("e_ps16", z("US", us) + tm.aux_int("PS", "I", 16), umi="EDGE2"),                              # PS = len-2, no TE
        edge("e_cs_te", z("CS", "GATTACA") + z("US", us) + tm.aux_int("TE", "s", 30), umi="EDGE2"),       # CS wins over US / TE
    ]
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


@pytest.mark.parametrize("mapqv0", [False, True])
def test_file_to_file_matches_the_model(cc, gpu_ctx, tmp_path, mapqv0):
    rng = np.random.default_rng(201)
    recs = _filters_records(rng)
    bam, path = _bam_file(tmp_path, recs, block=5000)
    info = cc.compute_consensus(gpu_ctx, str(path), str(tmp_path / "out.fq"), segment_bytes=20000, n_threads=3, mapqv0=mapqv0)
    want, cnt = cm.compute_consensus(bam, mapqv0=mapqv0)
    assert (tmp_path / "out.fq").read_bytes() == want
    assert {k: info[k] for k in cnt} == cnt
    assert info["poa_molecules"] > 5
    assert b"@ACGT-EDGE-4\n" in want and b"@ACGT-EDGE2-2\n" in want


@pytest.mark.parametrize("max_reads", [3, 20, 50])
def test_maxreads(cc, gpu_ctx, tmp_path, max_reads):
    rng = np.random.default_rng(300 + max_reads)
    recs = _molecule_records(rng, 6, (2, 60), 60)
    bam, path = _bam_file(tmp_path, recs)
    info = cc.compute_consensus(gpu_ctx, str(path), str(tmp_path / "out.fq"), max_reads=max_reads, min_ps=4, max_ps=25)
    want, cnt = cm.compute_consensus(bam, max_reads=max_reads, min_ps=4, max_ps=25)
    assert (tmp_path / "out.fq").read_bytes() == want
    assert info["molecules"] == cnt["molecules"] == 6


def test_scratch_budget_error_names_the_molecule(cc, lib, gpu_ctx, tmp_path):
    rng = np.random.default_rng(8)
    recs = _molecule_records(rng, 1, 4, 60) + _molecule_records(rng, 2, 3, 2000, seed_names="big", first=1)
    _bam, path = _bam_file(tmp_path, recs)
    with pytest.raises(lib.SmiError, match=r"ComputeConsensus: molecule CELL0([12])-UMI0000\1-3 \(3 reads, \d+ bases: needs \d+ MiB"):
        cc.compute_consensus(gpu_ctx, str(path), str(tmp_path / "out.fq"), scratch_bytes=8 << 20)


def test_missing_sequence_fails_with_the_read_name(cc, lib, gpu_ctx, tmp_path):
    recs = _molecule_records(np.random.default_rng(7), 2, 3, 50)
    recs.insert(2, bammodel.bam_record("no_seq_read", 0, 0, 5, 60, [("M", 4)], "ACGT", aux=tm.aux_z("BC", "B") + tm.aux_z("U8", "X")))
    _bam, path = _bam_file(tmp_path, recs)
    with pytest.raises(lib.SmiError, match="no_seq_read"):
        cc.compute_consensus(gpu_ctx, str(path), str(tmp_path / "out.fq"))


STEP4 = "$params.java -jar $params.javaXmx $params.nanopore tagbamwithread --inFastq $fastqgz --inBam $bam --outBam parsedbamseq.bam --readTag US --qvTag QS"
# sicelore-nf/main.nf:156, verbatim
STEP4B = ("$params.java -jar $params.javaXmx $params.sicelore ComputeConsensus -T $params.max_cpus -I $bam -O chr.fq -CELLTAG $params.CELLTAG "
          "-UMITAG $params.UMITAG -GENETAG $params.GENETAG -TSOENDTAG $params.TSOENDTAG -POLYASTARTTAG $params.POLYASTARTTAG -CDNATAG $params.CDNATAG "
          "-USTAG $params.USTAG -RNTAG $params.RNTAG -MAPQV0 $params.MAPQV0 -TMPDIR $params.tmpdir -VALIDATION_STRINGENCY SILENT -MAXREADS $params.MAXREADS "
          "-MINPS $params.MINPS -MAXPS $params.MAXPS -DEBUG $params.DEBUG")
PARAMS = {"$params.javaXmx": "-Xmx4G", "$params.nanopore": "Jar/NanoporeBC_UMI_finder-2.1.jar", "$params.sicelore": "Jar/Sicelore-2.1.jar",
          "$params.max_cpus": "16", "$params.CELLTAG": "BC", "$params.UMITAG": "U8", "$params.GENETAG": "GE", "$params.TSOENDTAG": "TE",
          "$params.POLYASTARTTAG": "PS", "$params.CDNATAG": "CS", "$params.USTAG": "US", "$params.RNTAG": "RN", "$params.MAPQV0": "false",
          "$params.tmpdir": "/tmp", "$params.MAXREADS": "20", "$params.MINPS": "3", "$params.MAXPS": "20", "$params.DEBUG": "false"}


def _nf(cmd):
    for k in sorted(PARAMS, key=len, reverse=True):
        cmd = cmd.replace(k, PARAMS[k])
    return cmd.replace("$params.java", "$java")


def test_main_nf_step4b_on_what_tagbamwithread_wrote(pkg, synth, gpu_ctx, tmp_path):
    """synth reads -> run_files.run -> the passed FASTQ -> BAM records with BC / U8 / TE / PS for those names -> main.nf:116 (tagbamwithread)
    -> main.nf:156 (ComputeConsensus) through bin/java, and the README's I= O= form: both FASTQs are the model's on the tagged BAM"""
    import torch

    run_files = importlib.import_module("sicelore_amd.run_files")
    dev = torch.device("cuda", 0)
    wl = synth.make_whitelist(30_000, seed=5501, device=dev)
    used = synth.pick_used(wl, 40, seed=5502)
    fastqdir, scandir = tmp_path / "fastq", tmp_path / "scan"
    run_files.write_synthetic_dir(synth, str(fastqdir), 2, 1200, used, dev, seed=5510, chimera_frac=0.05)
    run_files.run(gpu_ctx, str(fastqdir), str(scandir), max_ed=1, n_workers=4, reads_per_chunk=1000, whitelist_keys=np.sort(wl.cpu().numpy().astype(np.uint64)),
                  compress=True)
    fastqgz = tmp_path / "fastq_pass.fastq.gz"
    with open(fastqgz, "wb") as f:
        for p in sorted((scandir / "passed").iterdir()):
            f.write(p.read_bytes())
    text = gzip.open(fastqgz).read()
    lines = text.split(b"\n")
    names = [ln[1:].split(b" ")[0].decode() for ln in lines[0::4] if ln]
    lens = [len(s) for s in lines[1::4]][:len(names)]
    assert len(names) > 1000
    rng = np.random.default_rng(8)
    pick = sorted(rng.choice(len(names), 600, replace=False))
    recs = []
    for k, i in enumerate(pick):
        mol = int(rng.integers(0, 120))                         # ~5 reads per molecule
        n = lens[int(i)]
        aux = tm.aux_z("BC", f"BC{mol % 9}-1") + tm.aux_z("U8", f"U{mol:04d}") + tm.aux_int("TE", "s", int(rng.integers(0, 40)))
        aux += tm.aux_int("PS", "S", max(n - int(rng.integers(0, 60)), 0)) + tm.aux_f("de", float(rng.integers(0, 20)) / 200)
        recs.append(bammodel.bam_record(names[int(i)], 16 if k % 3 == 0 else 0, k % 2, 100 + k, 60, [("M", 4)], "ACGT", aux=aux))
    bam = bammodel.bam_bytes(HEAD, REFS, recs)
    (tmp_path / "passedParsed.bam").write_bytes(bammodel.bgzf_compress(bam, block=16384))
    os.environ["PYTHON"] = sys.executable
    java = "bash " + os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java")
    env = dict(os.environ, java=java, fastqgz=str(fastqgz), bam=str(tmp_path / "passedParsed.bam"))
    r = subprocess.run(["bash", "-c", _nf(STEP4)], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    tagged = bammodel.bgzf_decompress((tmp_path / "parsedbamseq.bam").read_bytes())
    want, cnt = cm.compute_consensus(tagged, gene_tag="GE")
    assert cnt["molecules"] > 50 and cnt["valid"] == 600
    env["bam"] = str(tmp_path / "parsedbamseq.bam")
    r = subprocess.run(["bash", "-c", _nf(STEP4B)], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "chr.fq").read_bytes() == want
    assert f"Total SAMrecords\t{cnt['records']}" in r.stderr and f"Total molecules\t\t{cnt['molecules']}" in r.stderr
    r = subprocess.run(["bash", "-c", "$java -jar -Xmx32g Sicelore-2.1.jar ComputeConsensus I=parsedbamseq.bam O=molecules.chr1.fastq T=20 TMPDIR=/tmp/"],
                       env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    want_ig, _ = cm.compute_consensus(tagged)
    assert (tmp_path / "molecules.chr1.fastq").read_bytes() == want_ig
