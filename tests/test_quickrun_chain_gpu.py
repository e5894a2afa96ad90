"""The four `java` lines of the reference's quickrun-2.1.sh in script order -- 35 scanfastq, 42 assignumis, 45 SelectValidCellBarcode,
46 IsoformMatrix -- each as it stands through sicelore-2.1_amd/bin/java, one process after the other.  Only the mapping step between
lines 35 and 42 (minimap2 / samtools in the script) is replaced: the BAM is made from the names of the reads line 35 passed.  The cell
list that line 46 reads is the one line 45 wrote from the BarcodesAssigned.tsv of line 35; nothing here writes it by hand."""
import gzip
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import bammodel
import isoformmodel as im

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# quickrun-2.1.sh:35, :42, :45 and :46, verbatim
STEP1 = "$java -jar -Xmx4G Jar/NanoporeBC_UMI_finder-2.1.jar scanfastq -d $fastqdir -o $readscandir --bcEditDistance 1 --compress "
STEP3 = "$java -jar  -Xmx4G Jar/NanoporeBC_UMI_finder-2.1.jar assignumis --inFileNanopore ${mappingdir}passed.bam -o ${umidir}passedParsed.bam --annotationFile Data/gencode.v38.chr12.refFlat"
STEP4_SELECT = "$java -jar -Xmx4g Jar/Sicelore-2.1.jar SelectValidCellBarcode -I ${readscandir}BarcodesAssigned.tsv -O ${siceloredir}barcodes.csv -MINUMI 1 -ED0ED1RATIO 1"
STEP4_MATRIX = "$java -jar -Xmx4g Jar/Sicelore-2.1.jar IsoformMatrix -I ${umidir}passedParsed.bam -REFFLAT Data/gencode.v38.chr12.refFlat -CSV ${siceloredir}barcodes.csv -OUTDIR $siceloredir -PREFIX reads -ISOBAM true -VALIDATION_STRINGENCY SILENT"


def _line(cmd, env, cwd):
    return subprocess.run(["bash", "-c", cmd], env=env, cwd=cwd, capture_output=True, text=True, timeout=300)


def _selection(tsv_text, min_umi=1, ratio=1):
    """SelectValidCellBarcode.java:L57-78 on a table scanfastq wrote (four columns of non-negative numbers) -> (rows, kept barcodes)"""
    rows, kept = [], []
    for ln in tsv_text.split("\n")[1:]:
        if not ln:
            continue
        f = ln.replace(",", "").split("\t")
        total, ed0, ed1 = int(f[1]), int(f[2]), int(f[3])
        rows.append((f[0], total))
        if total >= min_umi and ed0 // (ed1 or 1) >= ratio:
            kept.append(f[0])
    return rows, kept


@pytest.fixture(scope="module")
def chain(pkg, synth, tmp_path_factory):
    """runs the four lines once, stopping at the first that does not exit 0 -> what each returned and where the files are"""
    import torch

    run_files = importlib.import_module("sicelore_amd.run_files")
    dev = torch.device("cuda", 0)
    wl = synth.make_whitelist(30_000, seed=7401, device=dev)
    used = synth.pick_used(wl, 40, seed=7402)
    work = tmp_path_factory.mktemp("quickrun")
    (work / "Data").mkdir()
    dirs = {k: str(work / k) + "/" for k in ("fastq", "scan", "map", "umi", "sicelore")}
    for k in ("map", "umi", "sicelore"):
        os.makedirs(dirs[k])
    run_files.write_synthetic_dir(synth, dirs["fastq"], 2, 1500, used, dev, seed=7410, chimera_frac=0.05)
    # the application directory's barcode file (config.xml:37), found in the working directory
    with gzip.open(work / "3M-february-2018.txt.gz", "wt") as f:
        for k in np.sort(wl.cpu().numpy().astype(np.uint64)):
            f.write("".join("AGCT"[(int(k) >> (2 * (15 - i))) & 3] for i in range(16)) + "-1\n")
    ref = "".join(f"GENE{g}\tTX{g}\tchr12\t+\t{19_000 + 4_000 * g}\t{22_500 + 4_000 * g}\t{19_100 + 4_000 * g}\t{22_400 + 4_000 * g}\t2\t"
                  f"{19_000 + 4_000 * g},{20_999 + 4_000 * g},\t{20_100 + 4_000 * g},{22_500 + 4_000 * g},\n" for g in range(8))
    ref += "".join(f"GENE{g}\tTX{g}b\tchr12\t+\t{19_000 + 4_000 * g}\t{22_500 + 4_000 * g}\t0\t0\t1\t{19_000 + 4_000 * g},\t{22_500 + 4_000 * g},\n"
                   for g in range(0, 8, 3))
    (work / "Data" / "gencode.v38.chr12.refFlat").write_text(ref)
    java = "bash " + os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java")
    env = dict(os.environ, PYTHON=sys.executable, java=java, fastqdir=dirs["fastq"], readscandir=dirs["scan"], mappingdir=dirs["map"],
               umidir=dirs["umi"], siceloredir=dirs["sicelore"])
    done = []
    out = dict(work=work, dirs=dirs, env=env, ref=ref, done=done)
    for name, cmd in (("35", STEP1), ("42", STEP3), ("45", STEP4_SELECT), ("46", STEP4_MATRIX)):
        if name == "42":
            # "mapping": two-exon alignments of the passed reads at eight loci, junctions jittered around the refFlat's
            names = []
            for p in sorted(os.listdir(dirs["scan"] + "passed")):
                lines = gzip.open(dirs["scan"] + "passed/" + p).read().split(b"\n")
                names += [ln[1:].split(b" ")[0].decode() for ln in lines[0::4] if ln]
            out["n_passed"] = len(names)
            rng = np.random.default_rng(74)
            rows = []
            for i, nm in enumerate(names):
                g = i % 8
                a, b = 20_100 + 4_000 * g + int(rng.integers(-3, 4)), 21_000 + 4_000 * g + int(rng.integers(-3, 4))
                p1 = a - 80
                rows.append((p1 - 1, nm, 16 if g & 1 else 0, [("S", 10), ("M", a - p1 + 1), ("N", b - a - 1), ("M", 70), ("S", 5)]))
            rows.sort()
            recs = [bammodel.bam_record(nm, fl, 0, p0, 30, cig, "C" * (sum(n for o, n in cig if o in "MS"))) for p0, nm, fl, cig in rows]
            header = bammodel.bam_bytes("@HD\tVN:1.6\tSO:coordinate\n", [("chr12", 10 ** 8)], [])
            with open(dirs["map"] + "passed.bam", "wb") as f:
                f.write(bammodel.bgzf_compress(header + b"".join(recs), block=16384))
        r = _line(cmd, env, str(work))
        done.append((name, r.returncode, r.stderr))
        if r.returncode != 0:
            break
    return out


def _completed(chain):
    assert [(name, rc) for name, rc, _err in chain["done"]] == [("35", 0), ("42", 0), ("45", 0), ("46", 0)], chain["done"][-1][2][-2000:]


def test_quickrun_java_lines_in_script_order(chain):
    _completed(chain)
    d = chain["dirs"]
    assert chain["n_passed"] > 1000
    tsv = open(d["scan"] + "BarcodesAssigned.tsv").read()
    rows, want = _selection(tsv)
    csv = open(d["sicelore"] + "barcodes.csv").read()
    assert csv == "".join(b + "\n" for b in want) and len(rows) >= 30
    err45 = chain["done"][2][2]
    assert f"Total cell barcodes\t\t[{len(rows)}]\nValid cell barcodes\t\t[{len(want)}]\n" in err45
    parsed = bammodel.bgzf_decompress(open(d["umi"] + "passedParsed.bam", "rb").read())
    _t, _r, recs = bammodel.parse_bam(parsed)
    in_bam = {a["aux"][a["aux"].index(b"BCZ") + 3:].split(b"\0")[0].decode() for a in recs if b"BCZ" in a["aux"]}
    assert len(recs) > 500 and len(in_bam & set(want)) >= 5               # the list names cells of this BAM: nothing below passes vacuously
    model, cnt = im.isoform_matrix(parsed, chain["ref"], csv, isobam=True)
    for name, data in model.items():
        got = open(d["sicelore"] + f"reads_{name}", "rb").read()
        if name == "isobam.bam":
            got = bammodel.bgzf_decompress(got)
        assert got == data, name
    assert cnt["onematch"] + cnt["monoexon"] > 100 and cnt["cells"] == len(want)
    log = open(d["sicelore"] + "reads.log").read()
    assert log.startswith(f"IsoformMatrix INPUT,{d['umi']}passedParsed.bam\n") and f"Total molecules,{cnt['molecules']}\n" in log


def test_line_45_again_with_minumi_at_the_median(chain):
    _completed(chain)
    d, env, work = chain["dirs"], chain["env"], chain["work"]
    tsv = open(d["scan"] + "BarcodesAssigned.tsv").read()
    rows, first = _selection(tsv)
    median = int(np.median([t for _b, t in rows]))
    _rows, want = _selection(tsv, min_umi=median)
    assert 0 < len(want) < len(rows)
    os.makedirs(d["sicelore"] + "median")
    cmd = STEP4_SELECT.replace("-MINUMI 1", f"-MINUMI {median}").replace("barcodes.csv", "median/barcodes.csv")
    assert cmd != STEP4_SELECT
    r = _line(cmd, env, str(work))
    assert r.returncode == 0, r.stderr[-2000:]
    csv = open(d["sicelore"] + "median/barcodes.csv").read()
    got = csv.split("\n")[:-1]
    assert got == want and csv.endswith("\n")
    assert r.stderr.count(" barcode removed\t\t[") == len(rows) - len(got) > 0
    assert f"Total cell barcodes\t\t[{len(rows)}]\nValid cell barcodes\t\t[{len(got)}]\n" in r.stderr
    assert set(got) <= set(first) and got == [b for b in first if b in set(got)]          # a subset of line 45's list, in its order
    assert open(d["sicelore"] + "barcodes.csv").read() == "".join(b + "\n" for b in first)   # which is still there
    cmd = STEP4_MATRIX.replace("barcodes.csv", "median/barcodes.csv").replace("-OUTDIR $siceloredir", "-OUTDIR ${siceloredir}median")
    r = _line(cmd, env, str(work))
    assert r.returncode == 0, r.stderr[-2000:]
    header = open(d["sicelore"] + "median/reads_isomatrix.txt").readline().rstrip("\n").split("\t")
    assert header[:3] == ["geneId", "transcriptId", "nbExons"] and len(header) - 3 == len(got) == len(set(got))
    assert sorted(header[3:]) == sorted(got)
