"""The host plumbing the handles share (csrc/smi_handle.h) on a CPU: tools/asan/handle_host.cpp, built here with g++, runs the CellList
reader, the refFlat line reader, the size protocol of the text getters and the error_read body; the cell lists and the refFlat lines must
be those of the Python models (isoformmodel, collapsemodel), the error texts those the two parse_model functions have always given."""
import os
import subprocess

import pytest

import collapsemodel
import isoformmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = tmp_path_factory.mktemp("handle") / "handle_host"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{ROOT}/include", f"-I{ROOT}/sicelore-2.1_amd/csrc",
                    f"{ROOT}/tools/asan/handle_host.cpp", "-o", str(exe)], check=True)
    return str(exe)


def _run(tool, tmp_path, mode, text, *args):
    p = tmp_path / "in.txt"
    p.write_bytes(text.encode("latin-1"))
    out = subprocess.run([tool, mode, *args, str(p)], check=True, capture_output=True).stdout.decode("latin-1")
    return [line.split("\t") for line in out.split("\n")[:-1]]


CELL_LISTS = dict(
    empty="", one_no_newline="AAA", no_final_newline="AAA\nCCC", crlf="AAA\r\nCCC\r\n", lone_cr="AAA\rCCC\rGGG\n", cr_at_the_end="AAA\nCCC\r",
    empty_line_in_the_middle="AAA\n\nCCC\n", minus1_at_the_end="AAA-1\nCCC-1\n", minus1_in_the_middle="AA-1A\nCCC\n", minus1_twice="A-1A-1\n-1-1C\n",
    only_minus1="AAA\n-1\nCCC\n", nested_minus1="A--11\n", duplicates="CCC\nAAA\nCCC-1\nAAA\n", crlf_then_empty="AAA\r\n\r\nCCC", final_crlf_cr="AAA\r\n\r")


@pytest.mark.parametrize("name", sorted(CELL_LISTS))
def test_cell_list(tool, tmp_path, name):
    text = CELL_LISTS[name]
    got = _run(tool, tmp_path, "cells", text)
    assert all(g[0] == "cell" and len(g) == 2 for g in got)
    cells = [g[1] for g in got]
    assert sorted(set(cells)) == isoformmodel.cell_list(text)          # what Isoform, Snp and Fusion keep
    assert all("-1" not in c or name == "nested_minus1" for c in cells)
    # file order, one entry per line: what Collapse inserts
    lines = text.replace("\r\n", "\n").replace("\r", "\n").split("\n")
    assert cells == [ln.replace("-1", "") for ln in (lines[:-1] if lines[-1] == "" else lines)]


def test_cell_list_cases_hold_what_they_are_named_for():
    assert isoformmodel.cell_list("") == [] and isoformmodel.cell_list(CELL_LISTS["only_minus1"]) == ["", "AAA", "CCC"]
    assert isoformmodel.cell_list(CELL_LISTS["duplicates"]) == ["AAA", "CCC"] and isoformmodel.cell_list(CELL_LISTS["nested_minus1"]) == ["A-1"]
    assert isoformmodel.cell_list(CELL_LISTS["empty_line_in_the_middle"]) == ["", "AAA", "CCC"]


def _line(gene="G", tx="T", chrom="chr1", strand="+", nums=(100, 900, 150, 850, 2), xs="100,500,", xe="200,900,", extra=()):
    return "\t".join([gene, tx, chrom, strand, *[str(v) for v in nums], xs, xe, *extra])


def _both(text, line, why):
    return text, (line, why), (line, why)


GOOD = _line("G0", "T0")
# name -> (text, error of IsoformMatrix or None, error of CollapseModel or None); an error is (line, text behind "REFFLAT line <n>: ")
REFFLAT = dict(
    plain=(GOOD + "\n" + _line("G1", "T1", strand="-", xs="10,20,30", xe="15,25,35") + "\n", None, None),
    no_final_newline=(GOOD, None, None),
    ten_fields=_both(GOOD + "\n" + "\t".join(_line().split("\t")[:10]) + "\n", 2, "has 10 fields, at least 11 are needed"),
    twelve_fields=(_line(extra=("x",)) + "\n", None, None),
    trailing_commas=(_line(xs="100,500,,,", xe="200,900,,") + "\n", None, None),
    no_trailing_comma=(_line(xs="100,500", xe="200,900") + "\n", None, None),
    empty_exon_lists=_both(GOOD + "\n" + _line(xs=",", xe=",") + "\n", 2, "field 10 is not a list of integers"),
    more_starts_than_ends=_both(_line(xs="100,500,950", xe="200,900") + "\n", 1, "fewer exon ends than exon starts"),
    more_ends_than_starts=(_line(xs="100,500", xe="200,900,1000,1100") + "\n", None, None),
    zero_bases=(GOOD + "\n" + _line("GZ", "TZ", xs="100,500", xe="100,500") + "\n" + _line("G2", "T2") + "\n", None, None),
    zero_bases_cancel=(_line(xs="100,500", xe="200,400") + "\n" + GOOD + "\n", None, None),
    bad_strand=(GOOD + "\n" + _line(strand="x") + "\n", None, (2, "field 4 is no strand (+, - or .)")),
    dot_strand=(_line(strand=".") + "\n", None, None),
    bad_strand_behind_too_few_fields=_both("\t".join(_line(strand="x").split("\t")[:9]) + "\n", 1, "has 9 fields, at least 11 are needed"),
    trailing_cr=(GOOD + "\r\n" + _line("G1", "T1") + "\r\n", None, None),
    cr_alone_in_the_last_field=(_line(xe="200,900,\r") + "\n", None, None),
    negative_numbers=(_line(nums=(-5, 900, -1, 850, 2), xs="-100,500", xe="200,900") + "\n", None, None),
    bad_exon_end=_both(_line(xe="200,9x0") + "\n", 1, "field 11 is not a list of integers"),
    empty_line=_both(GOOD + "\n\n", 2, "has 1 fields, at least 11 are needed"),
)
for _k in range(5):
    _nums = [100, 900, 150, 850, 2]
    _nums[_k] = ("x", "1.5", "", "1e3", "0x10")[_k]
    REFFLAT[f"non_integer_field_{_k + 5}"] = _both(GOOD + "\n" + _line(nums=_nums) + "\n", 2, f"field {_k + 5} is not an integer")


def _kept(rows):
    return [dict(line=int(r[1]), gene=r[2], tx=r[3], strand=r[4], nums=[int(v) for v in r[5:10]],
                 xs=[int(v) for v in r[10].split(",")[:-1]], xe=[int(v) for v in r[11].split(",")[:-1]]) for r in rows if r[0] == "kept"]


@pytest.mark.parametrize("name", sorted(REFFLAT))
def test_refflat_lines(tool, tmp_path, name):
    text, iso_err, col_err = REFFLAT[name]
    for who, strand, err, model in (("IsoformMatrix", "0", iso_err, isoformmodel.parse_refflat), ("CollapseModel", "1", col_err, collapsemodel.parse_refflat)):
        rows = _run(tool, tmp_path, "refflat", text, who, strand)
        if err is not None:
            assert rows[-1] == ["bad", f"{who}: REFFLAT line {err[0]}: {err[1]}"] and all(r[0] != "bad" for r in rows[:-1])
            with pytest.raises(isoformmodel.IsoformError, match=f"REFFLAT line {err[0]}: "):
                model(text)
            continue
        assert all(r[0] in ("kept", "dropped") for r in rows)
        kept = _kept(rows)
        assert all(len(k["xe"]) >= len(k["xs"]) for k in kept)
        if who == "IsoformMatrix":
            genes, by_gene, n = model(text)
            assert n == len(kept) and genes == list(dict.fromkeys(k["gene"] for k in kept))
            for g in genes:
                mine = [k for k in kept if k["gene"] == g]
                assert [(k["tx"], [(k["xe"][i - 1], k["xs"][i] + 1) for i in range(1, len(k["xs"]))], len(k["xs"])) for k in mine] == by_gene[g]
        else:
            by_gene, n = model(text)
            assert n == len(kept) and list(by_gene) == list(dict.fromkeys(k["gene"] for k in kept))
            for g, txs in by_gene.items():
                mine = [k for k in kept if k["gene"] == g]
                assert [(k["tx"], k["nums"][:4], [[k["xs"][i] + 1, k["xe"][i]] for i in range(len(k["xs"]))]) for k in mine] == \
                    [(t.tx, [t.tx_start, t.tx_end, t.cds_start, t.cds_end], t.exons) for t in txs]     # (the extra ends are dropped)


def test_refflat_cases_hold_what_they_are_named_for(tool, tmp_path):
    def rows(name, who="CollapseModel", strand="1"):
        return _run(tool, tmp_path, "refflat", REFFLAT[name][0], who, strand)
    assert [r[:2] for r in rows("zero_bases")] == [["kept", "1"], ["dropped", "2"], ["kept", "3"]]
    assert [r[:2] for r in rows("zero_bases_cancel")] == [["dropped", "1"], ["kept", "2"]]
    assert _kept(rows("more_ends_than_starts"))[0]["xe"] == [200, 900, 1000, 1100]
    assert _kept(rows("trailing_commas"))[0]["xs"] == [100, 500] and _kept(rows("cr_alone_in_the_last_field"))[0]["xe"] == [200, 900]
    assert [k["strand"] for k in _kept(rows("bad_strand", "IsoformMatrix", "0"))] == ["+", "x"]
    assert [k["gene"] for k in _kept(rows("trailing_cr"))] == ["G0", "G1"] and _kept(rows("plain"))[1]["nums"] == [100, 900, 150, 850, 2]


def test_exon_bases_of_two_to_the_32_are_zero_in_int_arithmetic(tool, tmp_path):
    """getExonBases() is an int: 2^32 bases come to 0 and the line is dropped, by both programs (the Python models count in big integers and
    would keep it, so this case states its expectation itself); 2^31 bases are not 0 and the line stays"""
    two32 = _line("GW", "TW", xs="-2147483648,-2147483648", xe="0,0")
    two31 = _line("GH", "TH", xs="-2147483648", xe="0")
    text = GOOD + "\n" + two32 + "\n" + two31 + "\n"
    for who, strand in (("IsoformMatrix", "0"), ("CollapseModel", "1")):
        rows = _run(tool, tmp_path, "refflat", text, who, strand)
        assert [r[:2] for r in rows] == [["kept", "1"], ["dropped", "2"], ["kept", "3"]]
    assert isoformmodel.parse_refflat(two32 + "\n")[2] == 1
    rows = _run(tool, tmp_path, "refflat", _line(nums=(2147483648, 900, 150, 850, 2)) + "\n", "IsoformMatrix", "0")   # Integer.valueOf of 2^31
    assert rows == [["bad", "IsoformMatrix: REFFLAT line 1: field 5 is not an integer"]]


GETTER_TEXTS = dict(empty="", one_byte="x", text="gene\tcell1\tcell2\nG0\t1\t0\n", binary="\x00\xff\x00line\r\n" * 40)


@pytest.mark.parametrize("name", sorted(GETTER_TEXTS))
def test_getter_size_protocol(tool, tmp_path, name):
    text = GETTER_TEXTS[name]
    n = str(len(text))
    rows = _run(tool, tmp_path, "getter", text)
    assert rows[0] == ["size", "0", n]                                  # out == NULL: the size, SMI_OK
    if text:
        assert rows[1] == ["short", "1", n, "1"]                        # cap one short: 1, *n_out set, out untouched
    assert rows[-1] == ["exact", "0", n, "1", "1"] and len(rows) == (3 if text else 2)


def test_error_read_cuts_the_name_to_cap(tool):
    out = subprocess.run([tool, "error_read", "read_12345", "41"], check=True, capture_output=True).stdout.decode()
    rows = [line.split("\t") for line in out.split("\n")[:-1]]
    assert rows == [["0", "0", "41", "-", "1"],            # cap 0: nothing written, the record index set
                    ["1", "0", "41", "", "1"],             # cap 1: the NUL alone
                    ["4", "0", "41", "rea", "1"],          # cap 4 of a 10-byte name: 3 bytes and the NUL
                    ["64", "0", "41", "read_12345", "1"]]
    out = subprocess.run([tool, "error_read", "", "-1"], check=True, capture_output=True).stdout.decode()
    assert [line.split("\t") for line in out.split("\n")[:-1]][2] == ["4", "0", "-1", "", "1"]


def test_grow_only_buffer_under_the_sanitizers(tmp_path):
    """csrc/smi_growbuf.h against a counting allocator (tools/asan/growbuf_host.cpp): a stand-alone host program, built with
    AddressSanitizer and UBSan and run directly"""
    exe = tmp_path / "growbuf_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{ROOT}/sicelore-2.1_amd/csrc",
                    f"{ROOT}/tools/asan/growbuf_host.cpp", "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True)
    assert out.returncode == 0 and out.stdout.decode().strip() == "growbuf_host: ok", out.stderr.decode()
