"""SelectValidCellBarcode without a GPU: one table built from literals against outputs written out by hand from
SelectValidCellBarcode.java:L57-90, the rows the reference dies on, and the command line -- in process and, for quickrun-2.1.sh:45 and
sicelore-nf/main.nf:48, through bin/java in a subprocess."""
import importlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "Barcode\tn Reads with ED<=1 match\tED=0\tED=1"
# line 2 onwards; the comment is the quotient ed0 / ed1 of L75 (an ed1 of 0 is 1)
ROWS = [
    "AAAA\t140,612\t118,919\t21,693",         # grouped numbers: 118919 / 21693 = 5
    "AAAC\t40\t20\t20",                       # exactly 1
    "AAAG\t39\t19\t20",                       # ed0 one below ed1: 0
    "AAAT\t29\t19\t10",                       # 19 / 10 = 1, not 1.9
    "AACA\t12\t3\t0",                         # ed1 0 reads as 1: 3
    "AACC\t12\t0\t0",                         # 0 / 1 = 0
    "AACG\t10\t10\t0",                        # reads == MINUMI 10
    "AACT\t9\t9\t0",                          # reads one below MINUMI 10
    "AAGA\t15\t\t3",                          # an empty field 2 is 0: 0
    "AAGC\t15\t7\t\t8",                       # an empty field 3 (kept by the fifth field behind it) is 0, then 1: 7
    "AAGG\t50\t4\t2\t44",                     # five columns (--bcEditDistance 2): reads 50 though ED=0 + ED=1 = 6 < MINUMI; 2
    "AAGT\t+20\t+5\t+5",                      # a leading + is read: 1
    "AATA\t20\t-5\t2",                        # -5 / 2 = -2 (toward zero; a floor would give -3)
    "AATC\t2147483647\t2147483647\t1",        # Integer.MAX_VALUE
    "AATG\t20\t-2147483648\t-1",              # Integer.MIN_VALUE / -1 = Integer.MIN_VALUE
    "AA,TT\t2,0\t1,0\t5",                     # the commas go from the whole line: AATT, 20, 10 / 5 = 2
    "\t30\t9\t3",                             # an empty barcode: an empty line in the output; 3
    "ACAA\t30\t9\t3\tx\ty\tnot a number",     # columns past the fourth are not read: 3
]
TABLE = HEADER + "\n" + "".join(r + "\n" for r in ROWS)
# (MINUMI, ED0ED1RATIO) -> the output file, by hand
KEPT = {
    (10, 1.0): "AAAA\nAAAC\nAAAT\nAACA\nAACG\nAAGC\nAAGG\nAAGT\nAATC\nAATT\n\nACAA\n",
    (10, 0.0): "AAAA\nAAAC\nAAAG\nAAAT\nAACA\nAACC\nAACG\nAAGA\nAAGC\nAAGG\nAAGT\nAATC\nAATT\n\nACAA\n",
    (10, 1.5): "AAAA\nAACA\nAACG\nAAGC\nAAGG\nAATC\nAATT\n\nACAA\n",
    (10, -2.0): "AAAA\nAAAC\nAAAG\nAAAT\nAACA\nAACC\nAACG\nAAGA\nAAGC\nAAGG\nAAGT\nAATA\nAATC\nAATT\n\nACAA\n",
    (9, 1.0): "AAAA\nAAAC\nAAAT\nAACA\nAACG\nAACT\nAAGC\nAAGG\nAAGT\nAATC\nAATT\n\nACAA\n",
    (200000, 1.0): "AATC\n",
}
# the `barcode removed` messages of (10, 1.0) in order, by hand: the line is shown after its commas went
REMOVED_10_1 = [
    "AAAG barcode removed\t\t[AAAG\t39\t19\t20]",
    "AACC barcode removed\t\t[AACC\t12\t0\t0]",
    "AACT barcode removed\t\t[AACT\t9\t9\t0]",
    "AAGA barcode removed\t\t[AAGA\t15\t\t3]",
    "AATA barcode removed\t\t[AATA\t20\t-5\t2]",
    "AATG barcode removed\t\t[AATG\t20\t-2147483648\t-1]",
]


@pytest.fixture(scope="module")
def sv(pkg):
    return importlib.import_module("sicelore_amd.selectvalidcellbarcode")


@pytest.fixture(scope="module")
def cli(pkg):
    return importlib.import_module("sicelore_amd.cli")


@pytest.fixture(scope="module")
def libmod(pkg):
    return importlib.import_module("sicelore_amd.lib")


def _select(sv, tmp_path, text, min_umi, ratio):
    (tmp_path / "t.tsv").write_bytes(text.encode())
    log = io.StringIO()
    info = sv.select_valid_cell_barcodes(str(tmp_path / "t.tsv"), str(tmp_path / "o.csv"), min_umi=min_umi, ed0ed1_ratio=ratio, log=log)
    return (tmp_path / "o.csv").read_bytes().decode(), info, log.getvalue().split("\n")


@pytest.mark.parametrize("params", sorted(KEPT))
def test_hand_built_table(sv, tmp_path, params):
    out, info, log = _select(sv, tmp_path, TABLE, *params)
    assert out == KEPT[params]
    n_kept = KEPT[params].count("\n")
    assert info == dict(total=18, kept=n_kept)
    assert log[-3:] == ["Total cell barcodes\t\t[18]", f"Valid cell barcodes\t\t[{n_kept}]", ""]
    assert len(log) - 3 == 18 - n_kept and all(" barcode removed\t\t[" in ln and ln.endswith("]") for ln in log[:-3])
    if params == (10, 1.0):
        assert log[:-3] == REMOVED_10_1
    if params == (10, 1.5):
        assert "AAAT barcode removed\t\t[AAAT\t29\t19\t10]" in log and "AAGT barcode removed\t\t[AAGT\t+20\t+5\t+5]" in log
    if params == (200000, 1.0):
        assert log[0] == "AAAA barcode removed\t\t[AAAA\t140612\t118919\t21693]"
        assert "AATT barcode removed\t\t[AATT\t20\t10\t5]" in log and " barcode removed\t\t[\t30\t9\t3]" in log
        assert "AAGC barcode removed\t\t[AAGC\t15\t7\t\t8]" in log and "ACAA barcode removed\t\t[ACAA\t30\t9\t3\tx\ty\tnot a number]" in log


def test_defaults_are_minumi_1_and_ratio_1(sv, tmp_path):
    (tmp_path / "t.tsv").write_text(TABLE)
    assert sv.select_valid_cell_barcodes(str(tmp_path / "t.tsv"), str(tmp_path / "o.csv"), log=None) == dict(total=18, kept=13)
    assert (tmp_path / "o.csv").read_text() == KEPT[(9, 1.0)]          # every row has at least one read: the list of MINUMI 9


@pytest.mark.parametrize("ending", ["\r\n", "\r", "none", "mixed"])
def test_line_endings_of_readline(sv, tmp_path, ending):
    """BufferedReader.readLine: \\n, \\r\\n and a lone \\r end a line, and a last line without any counts"""
    if ending == "none":
        text = TABLE[:-1]
    elif ending == "mixed":
        lines = TABLE.split("\n")[:-1]
        text = "".join(ln + ("\n", "\r\n", "\r")[i % 3] for i, ln in enumerate(lines))[:-1]
    else:
        text = TABLE.replace("\n", ending)
    out, info, log = _select(sv, tmp_path, text, 10, 1.0)
    assert out == KEPT[(10, 1.0)] and info == dict(total=18, kept=12)
    assert log == REMOVED_10_1 + ["Total cell barcodes\t\t[18]", "Valid cell barcodes\t\t[12]", ""]


@pytest.mark.parametrize("text", ["", HEADER, HEADER + "\n", HEADER + "\r\n", HEADER + "\r", "\n"])
def test_empty_and_header_only(sv, tmp_path, text):
    out, info, log = _select(sv, tmp_path, text, 1, 1.0)
    assert out == "" and info == dict(total=0, kept=0)
    assert log == ["Total cell barcodes\t\t[0]", "Valid cell barcodes\t\t[0]", ""]


def test_bytes_pass_through_unchanged(libmod):
    """no charset is applied: a barcode field of any bytes comes out as it went in"""
    tsv = b"h\n\xff\xfe\xc3\x28\t5\t5\t1\n\xe2\x82\xac\t5\t1\t5\n"
    kept, removed, total, n_kept = libmod.select_valid_cells(tsv)
    assert (kept, total, n_kept) == (b"\xff\xfe\xc3\x28\n", 2, 1)
    assert removed == b"\xe2\x82\xac barcode removed\t\t[\xe2\x82\xac\t5\t1\t5]\n"


def test_the_sizing_idiom_of_the_c_entry_point(libmod):
    import ctypes

    lib = libmod.load_library()
    tsv = TABLE.encode()
    n_out, n_rem, line = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(7)
    counts = (ctypes.c_int64 * 2)()
    tail = (ctypes.byref(n_rem), counts, ctypes.byref(line))
    assert lib.smi_select_valid_cells(tsv, len(tsv), 10, 1.0, None, 0, ctypes.byref(n_out), None, 0, *tail) == 0        # sizes only
    assert (n_out.value, n_rem.value, counts[0], counts[1], line.value) == (len(KEPT[(10, 1.0)]), sum(len(m) + 1 for m in REMOVED_10_1), 18, 12, 0)
    buf = ctypes.create_string_buffer(n_out.value)
    assert lib.smi_select_valid_cells(tsv, len(tsv), 10, 1.0, buf, n_out.value, ctypes.byref(n_out), None, 0, *tail) == 0   # one buffer only
    assert buf.raw == KEPT[(10, 1.0)].encode()
    assert lib.smi_select_valid_cells(tsv, len(tsv), 10, 1.0, buf, n_out.value - 1, ctypes.byref(n_out), None, 0, *tail) < 0
    assert b"too small" in lib.smi_last_error()
    assert lib.smi_select_valid_cells(None, 5, 10, 1.0, None, 0, ctypes.byref(n_out), None, 0, *tail) < 0
    assert b"smi_select_valid_cells" in lib.smi_last_error()
    bad = b"h\nA\t1\t1\n"
    assert lib.smi_select_valid_cells(bad, len(bad), 1, 1.0, None, 0, ctypes.byref(n_out), None, 0, *tail) == 2
    assert line.value == 2 and b"line 2" in lib.smi_last_error()


GOOD = "AAAA\t9\t8\t1"
# name -> (the table, the 1-based line of the row the reference dies on, a piece of the reason)
BAD = {
    "three_columns": ("Barcode\tn Reads with ED<=0 match\tED=0\nAAAA\t9\t9\nAAAC\t8\t8\n", 2, "no ED=1 column"),
    "row_ends_in_tab": (f"{HEADER}\n{GOOD}\n{GOOD}\nAAAC\t5\t5\t\n{GOOD}\n", 4, "3 fields"),
    "blank_line": (f"{HEADER}\n{GOOD}\n{GOOD}\n\n{GOOD}\n", 4, "1 field"),
    "blank_line_crlf": (f"{HEADER}\r\n{GOOD}\r\n{GOOD}\r\n\r\n{GOOD}\r\n", 4, "1 field"),
    "only_tabs": (f"{HEADER}\n{GOOD}\n{GOOD}\n\t\t\t\n{GOOD}\n", 4, "0 fields"),
    "decimal_point": (f"{HEADER}\n{GOOD}\n{GOOD}\nAAAC\t1.5\t1\t1\n{GOOD}\n", 4, '"1.5" is not an int'),
    "above_int_range": (f"{HEADER}\n{GOOD}\n{GOOD}\nAAAC\t9\t2147483648\t1\n{GOOD}\n", 4, '"2147483648" is not an int'),
    "below_int_range": (f"{HEADER}\n{GOOD}\n{GOOD}\n{GOOD}\nAAAC\t9\t-2147483649\t1\n", 5, '"-2147483649" is not an int'),
    "leading_blank": (f"{HEADER}\n{GOOD}\n{GOOD}\nAAAC\t9\t5\t 5\n{GOOD}\n", 4, '" 5" is not an int'),
    "sign_alone": (f"{HEADER}\n{GOOD}\nAAAC\t9\t5\t-\n", 3, '"-" is not an int'),
    "empty_reads_field": (f"{HEADER}\n{GOOD}\n{GOOD}\nAAAC\t\t1\t1\n{GOOD}\n", 4, '"" is not an int'),
    "last_line_unterminated": (f"{HEADER}\n{GOOD}\nAAAC\t9\t5", 3, "3 fields"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_rows_the_reference_dies_on(cli, libmod, sv, tmp_path, capsys, case):
    """exit 1, the line and the reason named, no output file made and an existing one left byte for byte as it was"""
    text, line, why = BAD[case]
    (tmp_path / "t.tsv").write_bytes(text.encode())
    args = ["SelectValidCellBarcode", "-I", str(tmp_path / "t.tsv"), "-O", str(tmp_path / "o.csv"), "-MINUMI", "1", "-ED0ED1RATIO", "1"]
    assert cli.main(args) == 1
    err = capsys.readouterr().err
    assert f"line {line}:" in err and why in err and "ERROR: SelectValidCellBarcode" in err and str(tmp_path / "t.tsv") in err
    assert "Total cell barcodes" not in err
    assert not (tmp_path / "o.csv").exists()
    before = b"OLD\x00LIST\r\n"
    (tmp_path / "o.csv").write_bytes(before)
    st = os.stat(tmp_path / "o.csv")
    assert cli.main(args) == 1
    assert f"line {line}:" in capsys.readouterr().err
    assert (tmp_path / "o.csv").read_bytes() == before and os.stat(tmp_path / "o.csv").st_mtime_ns == st.st_mtime_ns
    with pytest.raises(libmod.CellTableError, match=f"line {line}:") as e:
        sv.select_valid_cell_barcodes(str(tmp_path / "t.tsv"), str(tmp_path / "o.csv"), log=None)
    assert e.value.line == line and (tmp_path / "o.csv").read_bytes() == before


def test_only_the_three_column_table_is_told_about_ed1(libmod):
    with pytest.raises(libmod.CellTableError) as e:
        libmod.select_valid_cells(BAD["row_ends_in_tab"][0].encode())
    assert "ED=1 column" not in str(e.value)


def test_cli_parses_both_syntaxes_and_defaults(cli):
    a = cli._picard_parse("-I a.tsv -O b.csv -MINUMI 1 -ED0ED1RATIO 1".split(), "SelectValidCellBarcode", cli.SV_OPTIONS, cli.SV_LONG)
    b = cli._picard_parse("INPUT=a.tsv OUTPUT=b.csv MINUMI=1 ED0ED1RATIO=1".split(), "SelectValidCellBarcode", cli.SV_OPTIONS, cli.SV_LONG)
    assert a == b == dict(I="a.tsv", O="b.csv", MINUMI=1, ED0ED1RATIO=1.0) and isinstance(a["ED0ED1RATIO"], float)
    assert {k: d for k, (_f, _k, d) in cli.SV_OPTIONS.items() if d is not None} == dict(MINUMI=1, ED0ED1RATIO=1.0, VALIDATION_STRINGENCY="STRICT")
    c = cli._picard_parse("I=a O=b ED0ED1RATIO=1.5 MINUMI=-3".split(), "SelectValidCellBarcode", cli.SV_OPTIONS, cli.SV_LONG)
    assert (c["ED0ED1RATIO"], c["MINUMI"]) == (1.5, -3)
    for text, want in (("2e-1", 0.2), (".5", 0.5), ("3.", 3.0), ("-0.25", -0.25), ("1d", 1.0), ("Infinity", float("inf"))):
        assert cli._picard_parse(["ED0ED1RATIO=" + text], "SelectValidCellBarcode", cli.SV_OPTIONS, cli.SV_LONG) == dict(ED0ED1RATIO=want)


def test_cli_runs_without_a_context(cli, tmp_path, capsys, monkeypatch):
    def no_context():
        raise AssertionError("SelectValidCellBarcode must not open a GPU context")

    monkeypatch.setattr(cli, "_context", no_context)
    (tmp_path / "t.tsv").write_text(TABLE)
    i, o = str(tmp_path / "t.tsv"), str(tmp_path / "o.csv")
    assert cli.main(["SelectValidCellBarcode", "-I", i, "-O", o, "-MINUMI", "10", "-ED0ED1RATIO", "1"]) == 0
    cap = capsys.readouterr()
    assert (tmp_path / "o.csv").read_text() == KEPT[(10, 1.0)] and cap.out == ""
    assert cap.err.split("\n")[:8] == REMOVED_10_1 + ["Total cell barcodes\t\t[18]", "Valid cell barcodes\t\t[12]"]
    assert cli.main(["SelectValidCellBarcode", f"I={i}", f"O={o}", "MINUMI=10", "ED0ED1RATIO=1.5", "VALIDATION_STRINGENCY=SILENT"]) == 0
    assert (tmp_path / "o.csv").read_text() == KEPT[(10, 1.5)]
    assert cli.main(["SelectValidCellBarcode", f"INPUT={i}", f"OUTPUT={o}"]) == 0                  # the defaults: MINUMI 1, ED0ED1RATIO 1
    assert (tmp_path / "o.csv").read_text() == KEPT[(9, 1.0)]
    assert cli.main(["SelectValidCellBarcode", "--INPUT", i, "--OUTPUT", o, "-ED0ED1RATIO=-2", "-MINUMI=10"]) == 0
    assert (tmp_path / "o.csv").read_text() == KEPT[(10, -2.0)]
    capsys.readouterr()


def test_cli_argument_errors(cli, tmp_path, capsys, monkeypatch):
    (tmp_path / "t.tsv").write_text(TABLE)
    base = [f"I={tmp_path / 't.tsv'}", f"O={tmp_path / 'o.csv'}"]
    for drop in range(2):
        assert cli.main(["SelectValidCellBarcode"] + base[:drop] + base[drop + 1:]) == 1
        assert "missing required option(s) " + base[drop][0] in capsys.readouterr().err
    for args, needle in (
            ([f"I={tmp_path / 'nope.tsv'}", base[1]], f"I={tmp_path / 'nope.tsv'}: no such file"),
            ([f"I={tmp_path}", base[1]], f"I={tmp_path}: no such file"),
            ([base[0], f"O={tmp_path / 'nodir' / 'o.csv'}"], f"O={tmp_path / 'nodir' / 'o.csv'}: no such directory"),
            (base + ["MINUMI=one"], "MINUMI 'one' is not a number"),
            (base + ["MINUMI=1.5"], "MINUMI '1.5' is not a number"),
            (base + ["MINUMI=2147483648"], "MINUMI 2147483648 is not a number"),
            (base + ["ED0ED1RATIO=high"], "ED0ED1RATIO 'high' is not a number"),
            (base + ["ED0ED1RATIO=1,5"], "ED0ED1RATIO '1,5' is not a number"),
            (base + ["ED0ED1RATIO=1_0"], "ED0ED1RATIO '1_0' is not a number"),
            (base + ["ED0ED1RATIO="], "ED0ED1RATIO '' is not a number"),
            (base + ["CELLTAG=BC"], "unknown option 'CELLTAG'"),
            (base + ["-MINUMI"], "option -MINUMI needs a value"),
            (base + ["VALIDATION_STRINGENCY=LOUD"], "VALIDATION_STRINGENCY 'LOUD'")):
        assert cli.main(["SelectValidCellBarcode"] + args) == 1, args
        assert needle in capsys.readouterr().err, args
    assert not (tmp_path / "o.csv").exists()
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert cli.main(["SelectValidCellBarcode"] + base) == 1
    assert "SelectValidCellBarcode runs in one process" in capsys.readouterr().err and not (tmp_path / "o.csv").exists()


def test_version_and_the_unknown_sub_command_text(cli, capsys):
    for flag in ("-version", "--version"):
        assert cli.main([flag]) == 0
        cap = capsys.readouterr()
        assert cap.out == "" and cap.err.count("\n") == 1 and "sicelore-2.1_amd" in cap.err
    for sub in ("ExportClippedReads", "AddBamReadTags", "AddBamReadSequenceTag", "mergestats", "parseillumina"):
        assert cli.main([sub, "I=a.bam"]) == 1
        err = capsys.readouterr().err
        assert f"sub-command {sub!r}" in err and "CollapseModel and FusionDetector" in err and "mergestats" in err and "SelectValidCellBarcode" in err


# quickrun-2.1.sh:45 (quickrun-2.1.step4b.sh:47 is the same line) and sicelore-nf/main.nf:48, verbatim
STEP4_SELECT = "$java -jar -Xmx4g Jar/Sicelore-2.1.jar SelectValidCellBarcode -I ${readscandir}BarcodesAssigned.tsv -O ${siceloredir}barcodes.csv -MINUMI 1 -ED0ED1RATIO 1"
NF_SELECT = "$params.java -jar $params.javaXmx $params.sicelore SelectValidCellBarcode -I $barcodeassigned -O BarcodesValidated.csv -MINUMI $params.MINUMI -ED0ED1RATIO $params.ED0ED1RATIO"


def _seeded_table(libmod):
    """a BarcodesAssigned.tsv from seeded per-barcode counters -> (text, the barcodes the counters say stay, in the table's order)"""
    rng = np.random.default_rng(4545)
    keys = np.unique(rng.integers(0, 1 << 32, size=400, dtype=np.uint64))
    counts = np.zeros((keys.size, 3), dtype=np.uint32)
    counts[:, 0] = rng.integers(0, 3000, size=keys.size)
    counts[:, 1] = rng.integers(0, 3000, size=keys.size)
    counts[::7, 1] = 0                  # no ED=1 read at all
    counts[::11, 0] = 0
    counts[::77] = 0                    # never assigned: no row
    counts[5] = (1, 1, 0)
    counts[6] = (0, 1, 0)
    text = libmod.assigned_tsv(keys, counts, max_ed=1)
    name = lambda k: "".join("AGCT"[(int(k) >> (2 * (15 - i))) & 3] for i in range(16))  # noqa: E731
    stay = {name(k) for k, (e0, e1, _e2) in zip(keys, counts.tolist()) if e0 + e1 >= 1 and e0 // max(e1, 1) >= 1}
    listed = [ln.split("\t")[0] for ln in text.split("\n")[1:] if ln]
    assert len(listed) == int((counts.sum(axis=1) > 0).sum()) and "," in text
    assert 50 < len(stay) < len(listed) - 50
    return text, [b for b in listed if b in stay]


def test_pipeline_lines_through_bin_java(libmod, tmp_path):
    text, want = _seeded_table(libmod)
    work = tmp_path / "run"
    for d in ("scan", "sicelore", "nf"):
        (work / d).mkdir(parents=True)
    (work / "scan" / "BarcodesAssigned.tsv").write_text(text)
    (work / "nf" / "BarcodesAssigned.tsv").write_text(text)
    java = "bash " + os.path.join(ROOT, "sicelore-2.1_amd", "bin", "java")
    # no device is offered to the child: the command has to run where there is no GPU
    env = dict(os.environ, PYTHON=sys.executable, java=java, readscandir=str(work / "scan") + "/", siceloredir=str(work / "sicelore") + "/",
               HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run(["bash", "-c", STEP4_SELECT], env=env, cwd=str(work), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (work / "sicelore" / "barcodes.csv").read_text() == "".join(b + "\n" for b in want)
    n_rows = text.count("\n") - 1
    assert f"Total cell barcodes\t\t[{n_rows}]\nValid cell barcodes\t\t[{len(want)}]\n" in r.stderr
    assert r.stderr.count(" barcode removed\t\t[") == n_rows - len(want)
    # main.nf:48 with the values of sicelore-nf/nextflow.config (java, javaXmx -Xmx12g, MINUMI 1, ED0ED1RATIO 1), filled in as Nextflow does
    line = NF_SELECT
    for k, v in (("$params.javaXmx", "-Xmx12g"), ("$params.java", java), ("$params.sicelore", "Jar/Sicelore-2.1.jar"), ("$params.MINUMI", "1"),
                 ("$params.ED0ED1RATIO", "1"), ("$barcodeassigned", "BarcodesAssigned.tsv")):
        line = line.replace(k, v)
    r = subprocess.run(["bash", "-c", line], env=env, cwd=str(work / "nf"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (work / "nf" / "BarcodesValidated.csv").read_text() == "".join(b + "\n" for b in want)
    r = subprocess.run(["bash", "-c", "$java -version"], env=env, cwd=str(work), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "sicelore-2.1_amd" in r.stderr
