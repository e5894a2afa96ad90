"""The record reader of csrc/smi_longread.h on a CPU: tools/asan/longread_host.cpp, built here with g++, runs the filters of
IsoformMatrix, ComputeConsensus, CollapseModel and FusionDetector through lr::read_segment over the BAMs of tests/longreadcases.py; the
counters, the kept records and the read an error names must be those of the Python models, for every case and every program.  Its --aux
mode walks the attribute lists of tests/auxcases.py with lr::aux_size alone, the rule the kernels call too."""
import os
import subprocess

import pytest

import auxcases as ac
import longreadcases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the tool's outcome names under the counters' names of the handles
NAMES = dict(isoform=dict(kept="valid", mapq0="mapqv0", chimeric="chimeria"), consensus=dict(kept="valid", mapq0="mapqv0", chimeric="chimeria"),
             fusion=dict(kept="valid", mapq0="mapqv0", chimeric="chimeria"), collapse={})


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = tmp_path_factory.mktemp("longread") / "longread_host"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{ROOT}/include", f"-I{ROOT}/sicelore-2.1_amd/csrc",
                    f"{ROOT}/tools/asan/longread_host.cpp", "-o", str(exe), "-lpthread"], check=True)
    return str(exe)


def _settings(outside=None):
    s = "cell BC\numi U8\ngene GE\nrn RN\niso IT\nte TE\nps PS\ncs CS\nus US\n"
    s += f"max_clip {lc.MAX_CLIP}\nmapqv0 0\nrn_min {lc.RN_MIN}\nthreads 4\n"
    s += "".join(f"listed {c}\n" for c in lc.CSV.split("\n")[:-1])
    return s + (f"outside {outside}\n" if outside is not None else "")


def _run(tool, tmp_path, name):
    data, kw = lc.CASES[name]
    (tmp_path / "in.bam").write_bytes(data)
    (tmp_path / "s.txt").write_text(_settings(kw.get("outside")))
    text = subprocess.run([tool, str(tmp_path / "in.bam"), str(tmp_path / "s.txt")], check=True, capture_output=True).stdout.decode("latin-1")
    got = {}
    for line in text.split("\n")[:-1]:
        f = line.split("\t")
        if f[1] == "refused":
            got[f[0]] = ("refused", f[2])
        elif f[1] == "error":
            got[f[0]] = ("error", int(f[2]), f[3], f[4])
        elif f[1] == "counts":
            c = {k: int(v) for k, v in (kv.split("=") for kv in f[2].split(" "))}
            c["unvalid"] = c["records"] - c["kept"]
            got[f[0]] = ("counts", {NAMES[f[0]].get(k, k): v for k, v in c.items()}, [])
        else:
            got[f[0]][2].append(tuple(f[2:]))
    return got


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_every_program_reads_the_case_as_its_model_does(tool, tmp_path, name):
    got, want = _run(tool, tmp_path, name), lc.expected(name)
    assert sorted(got) == sorted(lc.PROGRAMS)
    for p in lc.PROGRAMS:
        g, w = got[p], want[p]
        assert g[0] == w[0], (p, g[:2], w[:2])
        if w[0] == "refused":
            assert g[1] == f"smi_{p}_add_segment: record {w[1]} lies outside the segment"
        elif w[0] == "error":
            assert g[2] == w[1], (p, g, w)
            if p == "consensus" or w[2] in (lc.MALFORMED, "no CIGAR", "the CIGAR walk runs past the alignment blocks"):
                assert g[3] == w[2], (p, g, w)                       # (the other models word a failed cast in their own way)
        else:
            assert {k: g[1][k] for k in lc.COUNTS[p]} == w[1], p
            kept = [(r, bc, None if wr[2] is None else cdna, None if wr[3] is None else junc) for (r, bc, _umi, cdna, junc), wr in zip(g[2], w[2])]
            if p == "collapse":                                        # (the model holds its evidence gene by gene)
                assert sorted(r[0] for r in g[2]) == sorted(r[0] for r in w[2])
                by_read = {r[0]: r for r in w[2]}
                assert all(len(by_read) == len(w[2]) and (r, bc, None, junc) == by_read[r] for r, bc, _umi, _cdna, junc in g[2])
            else:
                assert len(g[2]) == len(w[2]) and kept == w[2], p


def test_the_cases_hold_what_they_are_named_for():
    """each rule is in its input: the outcomes the models give are the ones the case was built to provoke"""
    def kind(name):
        return {p: v[0] if v[0] != "counts" else v[1] for p, v in lc.expected(name).items()}
    assert kind("rn_z_no_cell") == dict(isoform=dict(records=3, valid=2, unvalid=1, mapqv0=0, no_gene=0, no_umi=0, chimeria=0, null=1),
                                        consensus=dict(records=3, valid=2, unvalid=1, mapqv0=0, no_gene=0, no_umi=0, chimeria=0, null=1),
                                        collapse="error", fusion=dict(records=3, valid=2, unvalid=1, mapqv0=0, no_gene=0, no_umi=0, chimeria=0, null=1))
    for name in ("rn_I_2_31", "bc_i_unmapped", "de_i_df_f", "df_z", "bc_z_then_i", "no_cigar"):
        assert set(kind(name).values()) == {"error"}, name
    for name in ("rn_I_max", "rn_types", "de_f_df_z", "bc_i_then_z", "d_20_21", "eq_x_blocks"):
        assert all(isinstance(v, dict) and v.get("valid", v.get("kept")) == v["records"] for v in kind(name).values()), name
    assert all(v["null"] == 1 for v in kind("no_cigar_unmapped").values())
    k = kind("no_sequence")
    assert k["collapse"]["null"] == 1 and all(k[p]["null"] == 0 and k[p]["valid"] == 3 for p in ("isoform", "consensus", "fusion"))
    for name in ("clip_no_block", "clip_no_block_151"):
        k = kind(name)
        assert k["consensus"]["chimeria"] == 1 and [k[p] for p in ("isoform", "collapse", "fusion")] == ["error"] * 3, name
    k = kind("clip_good")
    assert (k["isoform"]["chimeria"], k["consensus"]["chimeria"], k["collapse"]["chimeric"], k["fusion"]["chimeria"]) == (3, 3, 3, 1)
    k = kind("no_cdna")
    assert k["consensus"] == "error" and all(isinstance(k[p], dict) for p in ("isoform", "collapse", "fusion"))
    assert kind("no_cdna_chimeric")["consensus"]["chimeria"] == 1
    assert kind("te_negative")["consensus"] == "error" and kind("te_z")["consensus"] == "error"
    cdna = {r[0]: r[2] for r in lc.expected("ps_cuts")["consensus"][2]}
    assert cdna == dict(ps0="GTACGTACG", ps_last="GTACGTACG", ps_in="GTACGTAC", ps_far="GTACGTACG", te_behind="ACGTACGTACGT", bare="ACGTACGTACG")
    assert [r[1] for r in lc.expected("minus1")["isoform"][2]] == ["A", "", "1", "-1", "CELL1", "CELL2"]
    reasons = dict(isoform=("valid", "mapqv0", "no_gene", "no_umi", "chimeria"), consensus=("valid", "mapqv0", "no_umi", "chimeria"),
                   collapse=("kept", "mapq0", "chimeric", "low_rn", "not_listed", "no_gene"), fusion=("valid", "mapqv0", "no_gene", "chimeria"))
    for name in ("precedence", "threaded"):
        k = kind(name)
        assert all(k[p][c] > 0 for p in lc.PROGRAMS for c in reasons[p]), name
    assert all(v["null"] > 0 and v["records"] == 8200 for v in kind("threaded").values())
    e = lc.expected("threaded_errors")
    assert all(e[p][:2] == ("error", "t4100") for p in lc.PROGRAMS)


def test_the_attribute_size_rule_walks_every_list_as_the_model_does(tool, tmp_path):
    names = sorted(ac.CASES)
    (tmp_path / "blobs.txt").write_text("".join(ac.CASES[n].hex() + "\n" for n in names))
    text = subprocess.run([tool, "--aux", str(tmp_path / "blobs.txt")], check=True, capture_output=True).stdout.decode()
    lines = text.split("\n")[:-1]
    assert len(lines) == len(names)
    for name, line in zip(names, lines):
        got = [tuple(int(x) for x in step.split(":")) for step in line.split()]
        assert got == ac.walk(ac.CASES[name]), name


def test_the_attribute_lists_hold_what_they_are_named_for():
    w = {n: ac.walk(b) for n, b in ac.CASES.items()}
    assert w["empty"] == [] and w["one_byte"] == w["two_bytes"] == w["tag_and_type"] == [(0, ac.TRUNCATED)]
    assert w["good_then_one"] == w["good_then_two"] == [(4, ac.FINE), (0, ac.TRUNCATED)]
    for t, width in ac.WIDTH.items():
        assert w[f"scalar_{t}"] == [(4, ac.FINE), (3 + width, ac.FINE)] and w[f"scalar_{t}_short"] == [(4, ac.FINE), (0, ac.TRUNCATED)], t
    assert w["z"] == [(4, ac.FINE), (7, ac.FINE)] and w["z_empty"] == [(4, ac.FINE)] and w["z_then_good"] == [(6, ac.FINE), (4, ac.FINE)]
    assert w["z_no_nul"] == w["h_no_nul"] == [(4, ac.FINE), (0, ac.TRUNCATED)] and w["z_no_value"] == [(0, ac.TRUNCATED)]
    assert w["h"] == [(4, ac.FINE), (8, ac.FINE)] and w["h_odd"] == [(7, ac.FINE), (4, ac.FINE)] and w["h_not_hex"] == [(6, ac.FINE)]
    for e, width in ac.ELEMENT.items():
        assert w[f"b_{e}_0"] == [(4, ac.FINE), (8, ac.FINE), (4, ac.FINE)] and w[f"b_{e}_1"] == [(8 + width, ac.FINE), (4, ac.FINE)], e
    assert w["b_seven_left"] == [(4, ac.FINE), (0, ac.SHORT_ARRAY)] and w["b_header_only_type"] == [(0, ac.SHORT_ARRAY)]
    assert w["b_bad_element"] == [(4, ac.FINE), (0, ac.BAD_ELEMENT)] and w["b_bad_element_short"] == [(0, ac.SHORT_ARRAY)]
    assert w["b_one_past"] == w["b_huge"] == [(4, ac.FINE), (0, ac.TRUNCATED)] and w["b_one_past_i"] == w["b_huge_f"] == [(0, ac.TRUNCATED)]
    assert w["bad_type"] == w["bad_type_last"] == [(4, ac.FINE), (0, ac.BAD_TYPE)] and w["bad_type_nul"] == [(0, ac.BAD_TYPE)]
