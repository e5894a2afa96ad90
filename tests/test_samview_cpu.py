"""SamView without a GPU: the model (tests/sammodel.py) against a stream written out by hand and against the independent encoder
(tests/bammodel.py), the header rule, every stop by its text, the reader of the text in segments, the command line with the device call
replaced, and the edges tests/test_samview_gpu.py claims for the inputs of tests/samcases.py."""
import importlib
import io
import struct

import numpy as np
import pytest

import __graft_entry__ as graft
import bammodel
import samcases as sc
import sammodel as sm


def _mod(name):
    return importlib.import_module(f"{graft.PKG_NAME}.{name}")


def _records(raw):
    """the model's records of a case, parsed back by the independent parser"""
    header, recs = sm.convert(raw)
    return recs, bammodel.parse_bam(header + b"".join(recs))[2]


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def test_model_equals_the_stream_written_out_by_hand():
    text = b"@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000\n@SQ\tSN:c2\tLN:70000\n" \
           b"r1\t16\tc2\t16385\t60\t2S3M1D2M\t=\t101\t-7\tacGTnAC\t!\"#$%&'\tNM:i:300\tXA:A:q\tXF:f:-1.5\tXZ:Z:hi\tXB:B:S,1,65535\n" \
           b"u\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*"
    header = b"BAM\1" + struct.pack("<I", 48) + text[:48] + struct.pack("<I", 2) + struct.pack("<I", 3) + b"c1\0" + struct.pack("<I", 1000) + \
        struct.pack("<I", 3) + b"c2\0" + struct.pack("<I", 70000)
    assert text[:48].endswith(b"LN:70000\n")
    # pos 16384 .. 16390 on the reference: inside one 16 kb window, bin 4681 + 1
    r1 = struct.pack("<iiBBHHHiiii", 1, 16384, 3, 60, 4682, 4, 16, 7, 1, 100, -7) + b"r1\0" + struct.pack("<4I", 2 << 4 | 4, 3 << 4, 1 << 4 | 2, 2 << 4) + \
        bytes([0x12, 0x48, 0xF1, 0x20]) + bytes(range(7)) + b"NMs" + struct.pack("<h", 300) + b"XAAq" + b"XFf" + struct.pack("<f", -1.5) + b"XZZhi\0" + \
        b"XBBS" + struct.pack("<IHH", 2, 1, 65535)
    u = struct.pack("<iiBBHHHiiii", -1, -1, 2, 0, 4680, 0, 4, 0, -1, -1, 0) + b"u\0"
    want = header + struct.pack("<I", len(r1)) + r1 + struct.pack("<I", len(u)) + u
    assert sm.stream(text) == want


def test_model_against_the_independent_encoder():
    """records through bammodel.bam_record / bam_bytes, rendered to SAM text, converted back: equal on every field parse_bam returns, and
    byte for byte once bin, next_ref_id, next_pos and tlen are set aside (bam_record fixes them to 4680, -1, -1, 0)"""
    rng = np.random.default_rng(2)
    refs = [("c1", 100_000), ("c2", 5_000)]
    records = []
    for k in range(60):
        n = int(rng.integers(0, 40))
        seq = "".join(rng.choice(list(sc.ALPHABET), n))
        aux = b"NMC" + bytes([128 + k]) + b"XSs" + struct.pack("<h", -300 - k) + b"XIi" + struct.pack("<i", 70000 + k) + b"XUI" + struct.pack("<I", 2 ** 31 + k) + \
            b"XcC\xc8" + b"XZZvalue %d\0" % k + b"XHH1AFF\0" + b"XAA*" + b"XFf" + struct.pack("<f", k / 4 - 3) + b"XBBs" + struct.pack("<Ihh", 2, -5, k) + \
            b"XEBf" + struct.pack("<I", 0)
        cigar = [("S", 2), ("M", n), ("N", 100 + k), ("=", 1), ("X", 2), ("I", 3), ("D", 4), ("H", 5), ("P", 6)][:k % 10] if n else []
        records.append(bammodel.bam_record(f"read{k}", int(rng.integers(0, 65536)), int(rng.integers(-1, 2)), int(rng.integers(-1, 90_000)), int(rng.integers(0, 256)),
                                           cigar, seq, bytes(rng.integers(0, 94, n, dtype=np.uint8)) if k % 3 else None, aux if k % 4 else b""))
    header_text = "@HD\tVN:1.6\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in refs)
    original = bammodel.bam_bytes(header_text, refs, records)
    _text, _refs, parsed = bammodel.parse_bam(original)
    header, back = sm.convert(sm.sam_text(header_text, refs, parsed))
    again = bammodel.parse_bam(header + b"".join(back))
    assert again == (_text, _refs, parsed)
    assert header == original[:len(header)]
    for mine, theirs in zip(back, records):
        assert mine[:14] == theirs[:14] and mine[16:24] == theirs[16:24] and mine[36:] == theirs[36:]
        assert theirs[14:16] == struct.pack("<H", 4680) and theirs[24:36] == struct.pack("<iii", -1, -1, 0)


def test_header_rule():
    header, refs = sm.bam_header(sc.HEADER.encode())
    text, parsed, recs = bammodel.parse_bam(header)
    assert text == sc.HEADER and parsed == sc.REFS and recs == [] and "@PG\tID:samview" not in text
    assert refs == {b"chr1": 0, b"chr2": 1, b"chrM": 2}
    assert sm.bam_header(b"") == (b"BAM\1" + struct.pack("<II", 0, 0), {})
    # text order, fields in any order, a second line of a name keeps its entry and the first one its number
    header, refs = sm.bam_header(b"@SQ\tLN:5\tSN:b\n@CO\tSN:x\tLN:1\n@SQ\tSN:a\tLN:7\tUR:x\n@SQ\tSN:b\tLN:9")
    assert bammodel.parse_bam(header)[1] == [("b", 5), ("a", 7), ("b", 9)] and refs == {b"b": 0, b"a": 1}
    assert sm.split_header(b"@HD\n@CO\tx\nr\t0\n@late\n") == (b"@HD\n@CO\tx\n", b"r\t0\n@late\n", 2)
    assert sm.split_header(b"@HD\n@SQ") == (b"@HD\n@SQ", b"", 2)


@pytest.mark.parametrize("name", sorted(sc.stops()))
def test_every_stop_by_its_text(name):
    raw, line, reason = sc.stops()[name]
    with pytest.raises(sm.Stop) as e:
        sm.convert(raw)
    assert (e.value.line, e.value.reason) == (line, reason) and str(e.value) == f"line {line}: {reason}"


def test_first_of_two_bad_lines_and_the_late_stop():
    raw, line, reason = sc.two_bad_lines()
    with pytest.raises(sm.Stop) as e:
        sm.convert(raw)
    assert (e.value.line, e.value.reason) == (line, reason)
    raw, seg, line, reason = sc.late_stop()
    with pytest.raises(sm.Stop) as e:
        sm.convert(raw)
    assert (e.value.line, e.value.reason) == (line, reason)
    assert raw.find(b"\n", 0) and len(b"\n".join(raw.split(b"\n")[:line - 1])) > 4 * seg      # the stop lies in the fifth segment or behind it


def test_float_class_is_a_single_rounding():
    """inside the class, an exact integer below 2^53 times or by an exact power of ten is what float() gives"""
    for t in sc.FLOATS[:-3]:
        m = sm.FLOAT.match(t.encode())
        digits = (m.group(1) + (m.group(2) or b""))
        p = int(m.group(3) or 0) - len(m.group(2) or b"")
        v = float(int(digits)) * 10.0 ** p if p >= 0 else float(int(digits)) / 10.0 ** -p
        assert int(digits) < 2 ** 53 and abs(p) <= 22 and float(10 ** abs(p)) == 10.0 ** abs(p) and int(10.0 ** abs(p)) == 10 ** abs(p)
        assert struct.pack("<f", -v if t[0] == "-" else v) == sm.float_bits(t.encode()), t
    assert [sm.float_bits(t.encode()) for t in ("inf", "-inf", "nan")] == [b"\0\0\x80\x7f", b"\0\0\x80\xff", b"\0\0\xc0\x7f"]
    assert all(sm.float_bits(t.encode()) is None for t in sc.BAD_FLOATS)


# ---- the inputs hold the edges the GPU test claims ---------------------------------------------------------------------------------------------
def test_sequence_case():
    raw, _seg = sc.seq_lengths()
    recs, parsed = _records(raw)
    lens = [(len(r["seq"]), r["qual"] != b"\xff" * len(r["qual"])) for r in parsed[:2 * len(sc.SEQ_LENGTHS)]]
    assert lens == [(n, q and n > 0) for n in sc.SEQ_LENGTHS for q in (False, True)]
    # the layout that puts records at every offset mod 4: names of 1, 2, 3, 4 bytes in turn, so the sizes run through every residue
    offs, at = [], 0
    for r in recs:
        offs.append(at % 4)
        at += len(r)
    assert set(offs) == {0, 1, 2, 3}
    seq_at = {(r["off"] + 36 + len(r["name"]) + 1 + 4 * len(r["cigar"])) % 4 for r in parsed if len(r["seq"]) >= 17}
    assert seq_at == {0, 1, 2, 3}                                    # SEQ and QUAL begin at every alignment too
    assert parsed[-2]["seq"] == "ACGT=ACGT" and parsed[-1]["seq"] == "ANCNGNTNNNN" and set("".join(r["seq"] for r in parsed)) == set(sc.ALPHABET)


def test_cigar_case():
    raw, _seg = sc.cigars()
    _recs, parsed = _records(raw)
    assert [len(r["cigar"]) for r in parsed[:len(sc.CIGAR_COUNTS)]] == sc.CIGAR_COUNTS
    by = {r["name"]: r for r in parsed}
    assert [op for op, _n in by["letters"]["cigar"]] == list("MIDNSHP=X")
    assert by["longest"]["cigar"] == [("M", 2 ** 28 - 1), ("D", 2 ** 28 - 1), ("M", 1)] and by["zeros"]["cigar"] == [("M", 7), ("I", 0)]
    bins = {r["name"]: struct.unpack_from("<H", sm.convert(raw)[1][k], 14)[0] for k, r in enumerate(parsed)}
    assert bins["clip"] == bins["insert"] == 4681                    # reference length 0 on a window's last base: end = pos + 1 stays inside it
    with pytest.raises(sm.Stop):
        sm.convert(sc.stops()["cigar_65536"][0])


def test_attribute_case():
    raw, _seg = sc.attributes()
    recs, parsed = _records(raw)
    by = {r["name"]: r for r in parsed}

    def types(aux):
        out, p = [], 0
        while p < len(aux):
            ty = chr(aux[p + 2])
            out.append(ty)
            if ty in "ZH":
                p = aux.index(b"\0", p + 3) + 1
            elif ty == "B":
                p += 8 + struct.unpack_from("<I", aux, p + 4)[0] * (1 if aux[p + 3:p + 4] in b"cC" else 2 if aux[p + 3:p + 4] in b"sS" else 4)
            else:
                p += 3 + {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2}.get(ty, 4)
        return out

    assert [len(types(by[f"a{n}"]["aux"])) for n in sc.ATTR_COUNTS] == sc.ATTR_COUNTS
    assert types(by["types"]["aux"]) == list("AAccfZHHB")
    assert "".join(types(by["ints"]["aux"])) == "iissccCCssSSiiII"
    assert len(types(by["floats"]["aux"])) == len(sc.FLOATS)
    for st in "cCsSiIf":
        aux = by[f"B{st}"]["aux"]
        assert types(aux) == ["B"] * 4 and [struct.unpack_from("<I", aux, p)[0] for p in _b_counts_at(aux)] == sc.B_COUNTS
    z = by["z"]["aux"]
    assert z.startswith(b"Z0Z\0Z1Zx\0Z2Z") and len(z) == 4 + 5 + 4 + 5000 + 4


def _b_counts_at(aux):
    out, p = [], 0
    while p < len(aux):
        out.append(p + 4)
        p += 8 + struct.unpack_from("<I", aux, p + 4)[0] * (1 if aux[p + 3:p + 4] in b"cC" else 2 if aux[p + 3:p + 4] in b"sS" else 4)
    return out


def test_names_and_positions_case():
    raw, _seg = sc.names_and_positions()
    recs, parsed = _records(raw)
    by = {r["name"]: (r, recs[k]) for k, r in enumerate(parsed)}

    def core(name):
        return struct.unpack_from("<iiBBHHHiiii", by[name][1], 4)

    assert len(by["b" * 254][0]["name"]) == 254 and "a" in by
    assert core("a")[0] == 0 and core("a")[8:] == (0, 8, 7) and core("b" * 254)[0] == sc.N_MANY - 1 and core("b" * 254)[8:] == (0, 2 ** 31 - 2, -2 ** 31)
    assert core("unplaced")[:2] == (-1, -1) and core("unplaced")[4] == 4680 and core("on_ref_pos0")[:2] == (7, -1) and core("on_ref_pos0")[8] == sc.N_MANY - 1
    assert core("last_pos")[1] == 2 ** 31 - 2
    assert [core(n)[4] for n in ("in16k", "over16k", "next16k")] == [4681, 585, 4682]
    assert [core(n)[4] for n in ("in128k", "over128k", "next128k")] == [4681 + 7, 73, 4681 + 8]
    assert [core(n)[4] for n in ("in512m", "over512m", "next512m")] == [(4681 + 32767) & 0xFFFF, 0, (4681 + 32768) & 0xFFFF]
    assert core("whole")[4] == 0


def test_file_edges():
    assert sm.convert(sc.header_only()[0]) == (sm.bam_header(sc.HEADER.encode())[0], [])
    assert sm.convert(sc.header_only_open()[0])[1] == [] and sm.convert(sc.empty()[0]) == (b"BAM\1" + bytes(8), [])
    header, recs = sm.convert(sc.no_header()[0])
    assert header == b"BAM\1" + bytes(8) and len(recs) == 2
    assert sm.convert(sc.last_line_open()[0]) == sm.convert(sc.hand()[0]) and not sc.last_line_open()[0].endswith(b"\n")


# ---- the reader of the text -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_text_reader_cuts_on_line_ends(pkg, name):
    sv = _mod("samview")
    raw, seg = sc.CASES[name]()
    want_header, want_body, _n = sm.split_header(raw)
    for size in (seg, 1 << 20):
        pieces = list(sv.text_segments(io.BytesIO(raw), size))
        assert pieces[0] == want_header and b"".join(p.tobytes() for p in pieces[1:]) == want_body
        assert all(p.size and (p[-1] == 10 or p is pieces[-1]) for p in pieces[1:])
    if name in ("hand", "seq_lengths", "attributes"):
        assert len(list(sv.text_segments(io.BytesIO(raw), seg))) > 3


def test_small_segments_cut_inside_the_header_on_an_lf_and_inside_every_field():
    raw, seg = sc.hand()
    reads = set(range(seg, len(raw), seg))                            # where one read of the stream ends and the next begins
    header, _body, _n = sm.split_header(raw)
    assert any(0 < r < len(header) and raw[r - 1] != 10 for r in reads)
    assert any(raw[r] == 10 for r in reads if r >= len(header))
    inside = set()
    at = len(header)
    for ln in raw[at:].split(b"\n"):
        b = at
        for k, f in enumerate(ln.split(b"\t")):
            if any(b < r < b + len(f) for r in reads):
                inside.add(min(k, 11))
            b += len(f) + 1
        at += len(ln) + 1
    assert inside == set(range(12))                                    # the eleven fields and the attributes


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def stubbed(pkg, monkeypatch):
    """samview.main with the device call replaced: the arguments it would run with"""
    sv, cli = _mod("samview"), _mod("cli")
    calls = []

    def fake(ctx, in_sam, out_bam, index=False, n_threads=4, **kw):
        calls.append((in_sam, out_bam, index, n_threads))
        return dict(records=5, segments=1, bytes_written=400)
    monkeypatch.setattr(sv, "sam_to_bam", fake)
    monkeypatch.setattr(cli, "_context", lambda: None)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("SMI_ACTIVE_PROCESSORS", raising=False)
    return sv, calls


def test_command_line_argument_forms(stubbed, tmp_path, capsys):
    sv, calls = stubbed
    sam, out = tmp_path / "x.sam", str(tmp_path / "y.bam")
    sam.write_bytes(sc.hand()[0])
    for argv in (["-b", "-o", out, str(sam)], ["-bS", "-o", out, str(sam)], ["-Sb", str(sam), "-o", out], ["-S", "-b", "-h", "-@", "3", "-o", out, str(sam)],
                 ["-bhS", "-@8", "-o", out, "-"], ["-O", "bam", "-o", out, str(sam)], ["-b", "-O", "BAM", "--threads", "64", "-o", out, str(sam)]):
        assert sv.main(argv) == 0, argv
    assert [c[:3] for c in calls] == [(str(sam), out, False)] * 4 + [("-", out, False)] + [(str(sam), out, False)] * 2
    assert [calls[k][3] for k in (3, 4, 6)] == [3, 8, 16]
    assert "5 records in 1 segments, 400 bytes written" in capsys.readouterr().err
    assert sv.main([]) == 0
    text = capsys.readouterr().out
    assert "samtools view -bS" in text and "have no effect" in text


def test_command_line_refusals(stubbed, tmp_path, capsys, monkeypatch):
    sv, calls = stubbed
    sam, bam, out = tmp_path / "x.sam", tmp_path / "x.bam", str(tmp_path / "y.bam")
    sam.write_bytes(sc.hand()[0])
    bam.write_bytes(bammodel.bgzf_compress(b"BAM\1" + bytes(8)))
    cases = [(["-S", "-o", out, str(sam)], "this build writes BAM alone"), (["-b", str(sam)], "writes a file, not the standard output"),
             (["-b", "-o", out, str(sam), "chr1:1-100"], "a region behind the input is not built"), (["-b", "-o", out, str(bam)], "this build reads SAM text"),
             (["-b", "-O", "sam", "-o", out, str(sam)], "writes BAM alone"), (["-O", "cram", "-o", out, str(sam)], "writes BAM alone"),
             (["-b", "-o", out, str(tmp_path / "missing.sam")], "no such file"), (["-b", "-o", str(tmp_path / "nodir" / "y.bam"), str(sam)], "no such directory"),
             (["-b", "-o", str(tmp_path), str(sam)], "a directory"), (["-b", "-@", "x", "-o", out, str(sam)], "not a number"),
             (["-b", "-x", "-o", out, str(sam)], "unknown option"), (["-b", "--fast", "-o", out, str(sam)], "unknown option"), (["-b", "-o", out], "usage"),
             (["-b", "-o"], "needs a value")]
    cases += [([f"-b{c}", "-o", out, str(sam)], f"-{c}: ") for c in "fFqLrRsc1u"] + [(["-b", "-F", "4", "-o", out, str(sam)], "a filter on flag bits is not built")]
    for argv, text in cases:
        assert sv.main(argv) == 1, argv
        assert text in capsys.readouterr().err, argv
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert sv.main(["-b", "-o", out, str(sam)]) == 1
    assert "start it without torchrun" in capsys.readouterr().err
    assert calls == []


def test_a_stop_is_exit_code_1_and_names_the_line(stubbed, tmp_path, capsys, monkeypatch):
    sv, _calls = stubbed
    lib = _mod("lib")

    def stop(*a, **k):
        raise lib.SamViewError("line 12: QUAL and SEQ differ in length", 12, "QUAL and SEQ differ in length")
    monkeypatch.setattr(sv, "sam_to_bam", stop)
    sam, out = tmp_path / "x.sam", str(tmp_path / "y.bam")
    sam.write_bytes(sc.hand()[0])
    assert sv.main(["-bS", "-o", out, str(sam)]) == 1
    err = capsys.readouterr().err
    assert "line 12: QUAL and SEQ differ in length" in err and f"{out} was not written" in err


def test_cli_main_still_does_not_know_view(pkg, capsys):
    cli = _mod("cli")
    assert cli.main(["view", "-bS", "x.sam"]) == 1
    assert "this build has" in capsys.readouterr().err
    assert _mod("bamsort").main(["-o", "y.bam", "-"]) == 1
    assert "not the standard input" in capsys.readouterr().err


def test_library_mirror_lists_the_new_entry_points(pkg):
    lib = _mod("lib")
    names = [n for n in lib.EXPORTS if n.startswith("smi_samview_")]
    assert sorted(names) == sorted(f"smi_samview_{w}" for w in ("create", "header", "add_segment", "convert", "counts", "stage_ms", "error_line", "free", "host_loop"))
    assert lib.SAMVIEW_STAGES == ("index", "size", "scan", "write", "deflate") and issubclass(lib.SamViewError, lib.SmiError)
