"""The validator of CollapseModel in plain Python (test infrastructure only): BEDParser over BEDCodec(StartOffset.ZERO).decode,
getDistanceCage / getDistancePolyA, UCSCRefFlatParser.validator, statistics and exportFiles over TranscriptRecord's printers, literally, on top
of tests/collapsemodel.py, with DESIGN.md section 8h's rules: SHORT is read once in file order (no index), a record with flag 0x4 supports
nothing, and a BED line the reference's constructor would stop at is an error (ValidatorError) naming the file and the line."""
import re

import bammodel
import collapsemodel as cm
import isoformmodel as im

MAX_VALUE = 2 ** 31 - 1
VCOUNT_KEYS = ("valid_isoforms", "valid_evidences", "gencode_valid", "gencode_valid_ev", "ckj_valid", "ckj_valid_ev", "cks_valid",
               "cks_valid_ev", "nss_valid", "nss_valid_ev", "short_records", "short_boundaries", "junction_keys", "junction_hits", "table_slots",
               "cage_references", "cage_entries", "polya_references", "polya_entries")
KEY = {"gencode": "gencode", "combination_of_known_junctions": "ckj", "combination_of_known_splicesites": "cks",
       "at_least_one_novel_splicesite": "nss"}
# Float.parseFloat, the decimal forms (a hexadecimal floating literal counts as malformed, as in the library)
_FLOAT = re.compile(r"[+-]?(NaN|Infinity|(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?[fFdD]?)\Z")
_INT = re.compile(r"[+-]?\d+\Z")


class ValidatorError(RuntimeError):
    pass


def _jtrim(s):
    """String.trim: characters up to U+0020 off both ends"""
    a, b = 0, len(s)
    while a < b and s[a] <= " ":
        a += 1
    while b > a and s[b - 1] <= " ":
        b -= 1
    return s[a:b]


def _parse_int(s):
    """Integer.parseInt -> int, or None for a NumberFormatException"""
    if s is None or not _INT.match(s) or not -2 ** 31 <= int(s) <= MAX_VALUE:
        return None
    return int(s)


def _psplit(s, n):
    """ParsingUtils.split(s, new String[n], ','): the first n comma-separated parts, None where there is none"""
    parts = im.jsplit(s, ",")
    return [parts[k] if k < len(parts) else None for k in range(n)]


def decode_bed_line(line):
    """BEDCodec.decode(String) L82-92 and decode(String[]) L128-198 -> (chr, start, end, strand) or None; strand '+', '-' or None (NONE).
    Raises ValueError where the reference throws out of decode (BEDParser's constructor then stops reading, L57)."""
    if _jtrim(line) == "":
        return None
    if line.startswith("#") or line.startswith("track") or line.startswith("browser"):
        return None
    tokens = re.split(r"\t|( +)", line)[::2]                # Pattern "\t|( +)", split(line, -1); the group's captures dropped
    if len(tokens) < 2:
        return None
    start = _parse_int(tokens[1])
    if start is None:
        raise ValueError("the start is not an integer")
    end = start
    if len(tokens) > 2:
        end = _parse_int(tokens[2])
        if end is None:
            raise ValueError("the end is not an integer")
    if abs(start) > 2 ** 30 or abs(end) > 2 ** 30:
        raise ValueError("a start or end beyond 2^30")        # this build's rule: the reference's 32-bit differences would wrap
    strand = None
    if len(tokens) > 4 and not _FLOAT.match(_jtrim(tokens[4])):
        return tokens[0], start, end, None                    # L163-168: the feature as it is, strand NONE
    if len(tokens) > 5:
        st = _jtrim(tokens[5])
        c = st[0] if st else " "
        strand = c if c in "+-" else None
    if len(tokens) > 8 and "," in tokens[8]:                  # ParsingUtils.parseColor L369-374
        rgb = im.jsplit(tokens[8], ",")
        vals = []
        for k in range(3):
            if k >= len(rgb):
                raise ValueError("a colour of fewer than three parts")      # ArrayIndexOutOfBoundsException
            v = _parse_int(rgb[k])
            if v is None:
                break                                                        # NumberFormatException: caught, black
            vals.append(v)
        if len(vals) == 3 and not all(0 <= v <= 255 for v in vals):
            raise ValueError("a colour part outside 0 .. 255")               # IllegalArgumentException of Color
    if len(tokens) > 11:                                      # createExons L209-231
        if _parse_int(tokens[6]) is None or _parse_int(tokens[7]) is None:
            raise ValueError("thickStart or thickEnd is not an integer")
        count = _parse_int(tokens[9])
        if count is None or count < 0:
            raise ValueError("the block count is not a count")
        sizes, starts = _psplit(tokens[10], count), _psplit(tokens[11], count)
        for i in range(count):
            if _parse_int(starts[i]) is None or _parse_int(sizes[i]) is None:
                raise ValueError("fewer block sizes or starts than blocks, or one that is no integer")
    return tokens[0], start, end, strand


def parse_bed(text, what):
    """BEDParser(File) L27-60 -> ({chromosome: [(start, end, strand)] in file order}, entries)"""
    lines = re.split("\r\n|\n|\r", text)                      # AsciiLineReader
    if lines and lines[-1] == "":
        lines.pop()
    chr_to_bf, entries = {}, 0
    for no, line in enumerate(lines, 1):
        try:
            bf = decode_bed_line(line)
        except ValueError as e:
            raise ValidatorError(f"{what} line {no}: {e}")
        if bf is not None:
            entries += 1
            chr_to_bf.setdefault(bf[0], []).append(bf[1:])
    return chr_to_bf, entries


def distance(chr_to_bf, chromosome, strand, pos):
    """getDistanceCage L68-91 = getDistancePolyA L97-119"""
    mn, minabs = MAX_VALUE, MAX_VALUE
    for start, end, fstrand in chr_to_bf.get(chromosome, []):
        if strand == fstrand:
            pp = start if strand == "+" else end
            if abs(pos - pp) < minabs:
                mn, minabs = pos - pp, abs(pos - pp)
    return -mn if strand == "+" else mn


def block_junctions(pos1, cigar):
    """validator L325-333 over SAMUtils.getAlignmentBlocks L726-762: (e_prev - 1, s) between consecutive blocks"""
    blocks, ref = [], pos1
    for op, n in cigar:
        if op in "M=X":
            blocks.append((ref, n))
            ref += n
        elif op in "DN":
            ref += n
    return [(blocks[b - 1][0] + blocks[b - 1][1] - 1, blocks[b][0]) for b in range(1, len(blocks))]


def short_index(short_bam):
    """-> (reference names of SHORT, [(ref_id, junction list)] of the records the queries can return, records seen)"""
    _text, refs, recs = bammodel.parse_bam(short_bam)
    out = []
    for r in recs:
        if r["flag"] & 4 or not 0 <= r["ref_id"] < len(refs):  # a record with flag 0x4 supports nothing
            continue
        out.append((r["ref_id"], block_junctions(r["pos0"] + 1, r["cigar"])))
    return [nm for nm, _ln in refs], out, len(recs)


def print_txt(t):
    b = lambda x: "true" if x else "false"  # noqa: E731
    return (f"{t.gene}\t{t.tx}\t{t.chrom}\t{t.strand}\t{t.tx_start}\t{t.tx_end}\t{len(t.exons)}\t{t.nb_umis}\t{t.nb_cells}\t{t.categorie}\t"
            f"{t.subcategorie}\t{t.novel_text()}\t{t.junction_reads}\t{b(t.is_valid_junction)}\t{t.dist_cage}\t{b(t.is_valid_cage)}\t"
            f"{t.dist_polya}\t{b(t.is_valid_polya)}\t{b(t.is_valid)}\n")


def print_gff(t):
    ids = f'gene_id "{t.gene}"; transcript_id "{t.tx}";'
    s = (f'{t.chrom}\tsicelore\ttranscript\t{t.tx_start}\t{t.tx_end}\t.\t{t.strand}\t.\t{ids} category "{t.categorie}"; '
         f'subcategory "{t.subcategorie}"; UMIs "{t.nb_umis}"; Cells "{t.nb_cells}"; novelJunctions "{t.novel_text()}"; '
         f'supportingReads "{t.junction_reads}"; CAGEdist "{t.dist_cage}"; POLYAdist "{t.dist_polya}"; '
         f'color "{cm.COLORS.get(t.subcategorie, "#000000")}";\n')
    for a, b in t.exons:
        s += f"{t.chrom}\tsicelore\texon\t{a}\t{b}\t.\t{t.strand}\t.\t{ids}\n"
    return s


def transcripts(bam, refflat, csv, **kw):
    """CollapseModel.process L153-164 with tests/collapsemodel.py's functions: loader, collapser, initialize, filter, classifier
    -> (genes in output order, {gene: [Tx]}, counts)"""
    cfg = dict(cm.DEFAULTS, **kw)
    delta = cfg["delta"]
    cnt = dict.fromkeys(cm.COUNT_KEYS, 0)
    model, n_lines = cm.parse_refflat(refflat)
    cells = set(im.cell_list(csv)) if csv else set()
    cnt["cells"], cnt["model_genes"], cnt["model_transcripts"] = len(cells), len(model), n_lines
    genes = cm.load(bam, model, cells, cfg, cnt)
    order = sorted(genes, key=lambda g: g.encode("latin-1"))
    cnt["genes"] = len(genes)
    index = [1]
    for g in order:
        lst = genes[g]
        undef = next((t for t in lst if t.tx == "undef"), None)
        if undef is not None:
            cnt["undef_records"] += len(undef.evidence)
            cnt["monoexon"] += sum(1 for r in undef.evidence if not r["junctions"])
            cnt["max_undef"] = max(cnt["max_undef"], len(undef.evidence))
            novel = cm.collapse(undef.evidence, g, delta, index)
            cnt["founders"] += len(novel)
            cnt["max_founders"] = max(cnt["max_founders"], len(novel))
            lst.remove(undef)
            for t in novel:
                if len(t.evidence) >= cfg["min_evidence"]:
                    lst.append(t)
                    cnt["novel_evidenced"] += 1
    for g in order:
        for t in genes[g]:
            t.initialize()
    for g in order:
        keep = []
        for t in sorted(genes[g], key=lambda t: -len(t.exons)):
            if t.is_known:
                keep.append(t)
            else:
                j = t.junctions()
                if any(cm.is_all_include(j, k.junctions(), delta) for k in keep) or \
                        any(cm.is_all_include(j, m.junctions(), delta) for m in model.get(g, [])):
                    cnt["novel_filtered"] += 1
                else:
                    keep.append(t)
        genes[g] = keep
    for g in order:
        for t in genes[g]:
            if t.is_novel:
                cm.novelty_detector(t, model.get(g, []), delta)
            # TranscriptRecord L46-52
            t.is_valid = t.is_valid_cage = t.is_valid_polya = t.is_valid_junction = False
            t.dist_cage = t.dist_polya = t.junction_reads = 0
    return order, genes, cnt


def validator(order, genes, cage, polya, short_bam, cage_co, polya_co, junc_co, vc):
    """UCSCRefFlatParser.validator L279-366"""
    names, records, vc["short_records"] = short_index(short_bam)
    # the query of L321 and the loop of L322-342 for any key at once: isIn is a boolean, so a record counts once per junction it has
    having = {}
    for rid, junc in records:
        for j in set(junc):
            having[(rid,) + j] = having.get((rid,) + j, 0) + 1
    is_done = {}
    for g in order:
        for t in genes[g]:
            t.dist_cage = distance(cage, t.chrom, t.strand, t.tx_start if t.strand == "+" else t.tx_end)
            t.dist_polya = distance(polya, t.chrom, t.strand, t.tx_end if t.strand == "+" else t.tx_start)
            t.is_valid_cage = abs(t.dist_cage) <= cage_co
            t.is_valid_polya = abs(t.dist_polya) <= polya_co
            ok, total = True, 0
            for donor, acceptor in t.novel_junctions:
                jkey = (t.chrom, donor, acceptor)
                if jkey not in is_done:
                    ref = names.index(t.chrom) if t.chrom in names else -1     # reference index -1: an empty iterator
                    is_done[jkey] = having.get((ref, donor, acceptor), 0)
                total += is_done[jkey]
                if is_done[jkey] < junc_co:
                    ok = False
            t.is_valid_junction, t.junction_reads = ok, total
            if t.is_valid_cage and t.is_valid_polya and t.is_valid_junction:
                t.is_valid = True
    # what the library reports about its one pass
    keyed = set(names.index(c) for c, _d, _a in is_done if c in names)
    vc["junction_keys"] = sum(1 for c, _d, _a in is_done if c in names)
    vc["junction_hits"] = sum(is_done.values())
    for rid, junc in records:
        if rid in keyed:
            vc["short_boundaries"] += sum(1 for i, j in enumerate(junc) if i == 0 or junc[i - 1] != j)
    return is_done


def table_slots(n_keys, table_log2=0):
    if table_log2:
        return 1 << table_log2
    size = 16
    while size < 2 * n_keys:
        size <<= 1
    return size


def collapse_model(bam, refflat, csv, cage_text=None, polya_text=None, short_bam=None, cage_co=50, polya_co=50, junc_co=1, table_log2=0, **kw):
    """-> ({suffix: bytes}, counts, validator counts or None, supports {(chrom, donor, acceptor): reads}, {gene: [Tx]})"""
    order, genes, cnt = transcripts(bam, refflat, csv, **kw)
    vc, supports = None, {}
    if cage_text is not None and polya_text is not None and short_bam is not None:
        vc = dict.fromkeys(VCOUNT_KEYS, 0)
        cage, vc["cage_entries"] = parse_bed(cage_text, "CAGE")
        polya, vc["polya_entries"] = parse_bed(polya_text, "POLYA")
        vc["cage_references"], vc["polya_references"] = len(cage), len(polya)
        supports = validator(order, genes, cage, polya, short_bam, cage_co, polya_co, junc_co, vc)
        vc["table_slots"] = table_slots(vc["junction_keys"], table_log2)
    out = dict.fromkeys(cm.SUFFIXES, "")
    out[".txt"] = cm.LEGEND
    for g in order:                                            # statistics L553-578, exportFiles L611-628
        for t in genes[g]:
            k = KEY[t.subcategorie]
            cnt["isoforms"] += 1
            cnt["evidences"] += len(t.evidence)
            cnt[k] += 1
            cnt[k + "_ev"] += len(t.evidence)
            out[".refflat.txt"] += t.print_refflat()
            out[".txt"] += print_txt(t)
            out[".gff"] += print_gff(t)
            if t.is_known or (t.is_novel and t.is_valid):
                out[".final.gff"] += print_gff(t)
                out[".final.refflat.txt"] += t.print_refflat()
                if vc is not None:
                    vc["valid_isoforms"] += 1
                    vc["valid_evidences"] += len(t.evidence)
                    vc[k + "_valid"] += 1
                    vc[k + "_valid_ev"] += len(t.evidence)
    return {k: v.encode("latin-1") for k, v in out.items()}, cnt, vc, supports, genes


def message_lines(c, v, cage_path, polya_path):
    """the messages of a validated run in order (CollapseModel.java:L154, L167; BEDParser.java:L59; UCSCRefFlatParser.java:L142, L207, L213,
    L286, L293, statistics L542, L580-591), without the logger's prefix"""
    return [
        f"\tCells detected\t\t[{c['cells']}]",
        "Loader Bam Start...",
        f"Loader Bam End...{c['genes']}",
        f"Collapser Start...[{c['genes']} total genes]",
        "\tPerform validation using provided CAGE bed, POLYA bed and SHORT read bam files",
        f"BEDParser\t{cage_path}\t[references={v['cage_references']},entries={v['cage_entries']}]",
        f"BEDParser\t{polya_path}\t[references={v['polya_references']},entries={v['polya_entries']}]",
        f"Validator Start...[{c['genes']} total genes]",
    ] + [f"{nb} genes processed" for nb in range(1, c["genes"] + 1) if nb % 2500 == 0] + [
        "Printing statistics...",
        "-----------------------------------------------------------------------",
        "\t\t\t\t\tall_set (UMI)\tvalid_set (UMI)",
        f"total_genes\t\t\t\t{c['genes']}",
        f"total_isoforms\t\t\t\t{c['isoforms']} ({c['evidences']})\t{v['valid_isoforms']} ({v['valid_evidences']})",
        "full_splice_match",
        f" o gencode\t\t\t\t{c['gencode']} ({c['gencode_ev']})\t{v['gencode_valid']} ({v['gencode_valid_ev']})",
        "novel_in_catalog",
        f" o combination_of_known_junctions\t{c['ckj']} ({c['ckj_ev']})\t{v['ckj_valid']} ({v['ckj_valid_ev']})",
        f" o combination_of_known_splicesites\t{c['cks']} ({c['cks_ev']})\t{v['cks_valid']} ({v['cks_valid_ev']})",
        "novel_not_in_catalog",
        f" o at_least_one_novel_splicesite\t{c['nss']} ({c['nss_ev']})\t{v['nss_valid']} ({v['nss_valid_ev']})",
        "------------------------------------------------------------------------",
    ]
