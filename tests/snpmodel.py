"""SNPMatrix in plain Python (test infrastructure only): SNPMatrix.doWork, htsjdk's getReadPositionAtReferencePosition, the filter of
LongreadRecord.fromSAMRecord and Matrix.addMolecule / writeIsoformMatrix with a null model, under DESIGN.md section 8e's rules in place of
the reference's hash orders: cells and rows in byte order, molinfos in SNP-file line order, then BAM record order; every line against
every record (no index, any record order); what the reference swallows in mid-run raises SnpError naming the line or the read."""
import re

import numpy as np

import bammodel
import consensusmodel as cm
import isoformmodel as im

COUNT_KEYS = ("records", "lines", "cells", "hits", "lowRN", "lowQV", "pairs", "kept", "rows", "total_count")
COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C"}


class SnpError(RuntimeError):
    pass


def parse_snp(text, ref_names):
    """-> the kept lines in file order: dict(line, ref, chrom, neg, gene, pos (as written), arr (ascending))"""
    lines = re.split("\r\n|\r|\n", text)
    if lines and lines[-1] == "":
        lines.pop()
    kept = []
    for no, line in enumerate(lines, 1):
        if line == "":                                   # L102: the first empty line ends the file
            break
        tok = [] if set(line) == {","} else im.jsplit(line, ",")
        if not tok:
            raise SnpError(f"SNP line {no} ({line}): no fields")
        if tok[0] not in ref_names:                      # L107
            continue
        if len(tok) < 4:
            raise SnpError(f"SNP line {no} ({line}): has {len(tok)} fields, 4 are needed")
        pos = [tok[1]]
        if "|" in tok[1]:
            pos = [] if set(tok[1]) == {"|"} else im.jsplit(tok[1], "|")
        if not pos:
            raise SnpError(f"SNP line {no} ({line}): no position")
        arr = []
        for p in pos:
            if not re.fullmatch("[+-]?[0-9]+", p) or not -2 ** 31 <= int(p) < 2 ** 31:
                raise SnpError(f"SNP line {no} ({line}): position '{p}' is not an integer")
            arr.append(int(p))
        kept.append(dict(line=line, ref=ref_names.index(tok[0]), chrom=tok[0], neg=tok[2] == "-", gene=tok[3], pos=pos, arr=sorted(arr)))
    return kept


def read_position(pos1, cigar, p):
    """SAMRecord.getReadPositionAtReferencePosition(p): the 1-based read offset of reference position p inside an M / = / X block (read
    offsets count S and I, not H), 0 in a deletion, an intron or outside the alignment"""
    ref, read = pos1, 1
    for op, n in cigar:
        if op in "M=X":
            if ref <= p < ref + n:
                return p - ref + read
            ref += n
            read += n
        elif op in "DN":
            ref += n
        elif op in "IS":
            read += n
    return 0


def reference_length(cigar):
    return sum(n for op, n in cigar if op in "M=XDN")


def from_sam_record(r, cfg):
    """LongreadRecord.fromSAMRecord(r, false) as far as SNPMatrix reads it -> None, or dict(bc, umi, rn); raises where the reference throws"""
    name = r["name"]
    aux = cm._split_aux(r["aux"])

    def get(tag, want):
        try:
            return cm._value(aux.get(tag), want, name, tag)
        except cm.ConsensusError:
            raise SnpError(f"read {name}: attribute {tag} is not of the type SNPMatrix reads")
    get(cfg["gene_tag"], "Z")
    bc = get(cfg["cell_tag"], "Z")
    umi = get(cfg["umi_tag"], "Z")
    if bc is None or r["flag"] & 4:
        return None
    if get("de", "f") is None:
        get("df", "f")
    rn = get(cfg["rn_tag"], "i")
    if not r["cigar"]:
        raise SnpError(f"read {name}: no CIGAR")
    try:
        im.junctions(r["pos0"] + 1, r["cigar"])
    except im.IsoformError as e:
        raise SnpError(f"read {name}: {e}")
    return dict(bc=bc.replace(b"-1", b"").decode(), umi=None if umi is None else umi.decode(), rn=1 if rn is None else rn)


def snp_matrix(bam, snp, csv, min_rn=0, min_qv=0, cell_tag="BC", umi_tag="U8", gene_tag="GE", rn_tag="RN"):
    """-> ({file name suffix: bytes} -- empty when no row exists --, counts, [dict(line, hits, lowRN, lowQV)] per kept line)"""
    cfg = dict(cell_tag=cell_tag, umi_tag=umi_tag, gene_tag=gene_tag, rn_tag=rn_tag)
    _text, refs, recs = bammodel.parse_bam(bam)
    lines = parse_snp(snp, [nm for nm, _ln in refs])
    cells = im.cell_list(csv)
    in_list = set(cells)
    cnt = dict.fromkeys(COUNT_KEYS, 0)
    cnt.update(records=len(recs), lines=len(lines), cells=len(cells))
    matrix, mol, per_line = {}, [], []
    r_ref = np.array([r["ref_id"] for r in recs], dtype=np.int64)
    r_start = np.array([r["pos0"] + 1 for r in recs], dtype=np.int64)
    r_end = r_start + np.array([reference_length(r["cigar"]) for r in recs], dtype=np.int64) - 1
    r_neg = np.array([bool(r["flag"] & 16) for r in recs], dtype=bool)
    for L in lines:
        c = dict(line=L["line"], hits=0, lowRN=0, lowQV=0)
        # query(.., contained = false) L121 and the strand test L126, in file order
        for i in np.nonzero((r_ref == L["ref"]) & (r_start <= L["arr"][-1]) & (r_end >= L["arr"][0]) & (r_neg == L["neg"]))[0]:
            r = recs[i]
            start = int(r_start[i])
            lrr = from_sam_record(r, cfg)
            if lrr is None:
                continue
            rp = [read_position(start, r["cigar"], p) for p in L["arr"]]
            if not (min(rp) > 0 and len(r["seq"]) > max(rp)):
                continue
            if r["qual"][:1] == b"\xff":
                raise SnpError(f"read {r['name']}: no base qualities (*)")
            nuc = [r["seq"][x - 1] for x in rp]
            qv = [r["qual"][x - 1] for x in rp]
            if L["neg"]:
                nuc = [COMPLEMENT.get(b, "") for b in nuc]
            cnt["pairs"] += 1
            if lrr["rn"] < min_rn:
                c["lowRN"] += 1
            elif min(qv + [100]) < min_qv:
                c["lowQV"] += 1
            else:
                c["hits"] += 1
                if lrr["bc"] in in_list:                                                             # Matrix.addMolecule L69
                    if lrr["umi"] is None:
                        raise SnpError(f"read {r['name']}: a hit of cell {lrr['bc']} without the UMI attribute")
                    tx = f"{L['chrom']}:{'|'.join(L['pos'])}..{''.join(nuc)}"
                    matrix.setdefault(L["gene"] + "\t" + tx, {}).setdefault(lrr["bc"], set()).add(lrr["umi"])
                    mol.append(f"{lrr['bc']}\t{lrr['umi']}\t{lrr['rn'] if lrr['rn'] > 1 else 1}\t0\tnull\t{','.join(map(str, qv))}\t{L['gene']}\t{tx}\n")
        per_line.append(c)
        for k in ("hits", "lowRN", "lowQV"):
            cnt[k] += c[k]
    cnt["kept"], cnt["rows"] = len(mol), len(matrix)
    out = {}
    if matrix:
        rows = sorted(matrix, key=lambda k: k.encode("latin-1"))
        mat = ["geneId\ttranscriptId\tnbExons" + "".join("\t" + c for c in cells) + "\n"]
        met = ["geneId\ttranscriptId\tnbExons\tnbUmis\n"]
        for k in rows:
            vals = [len(matrix[k].get(c, ())) for c in cells]
            mat.append(k + "\tna" + "".join(f"\t{v}" for v in vals) + "\n")
            met.append(f"{k}\tna\t{sum(vals)}\n")
            cnt["total_count"] += sum(vals)
        out = {"snpmatrix.txt": "".join(mat).encode("latin-1"), "snpmetrics.txt": "".join(met).encode("latin-1"),
               "snpmolinfos.txt": ("cellBC\tUMI\tnbReads\tnbSupportingReads\tmappingPctId\tsnpPhredScore\tgeneId\ttranscriptId\n"
                                   + "".join(mol)).encode("latin-1")}
    return out, cnt, per_line


# ---- the hand-built case of tests/test_snp_cpu.py and tests/test_snp_gpu.py ------------------------------------------------------------
HEAD = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:1000000\n"
REFS = [("chr1", 1000000), ("chr2", 1000000)]
CSV = "CELL1\nCELL2-1\nCELL3\nCELL4\n"
SNP = ("chromosome,position,strand,name\n"
       "chr1,1010,+,before\n" "chr1,1050,+,indel\n" "chr1,1060,+,after\n" "chr1,1101,+,lastbase\n"
       "chr1,2000,+,clipS\n" "chr1,3000,+,clipH\n" "chr1,4010,+,ins\n" "chr1,5100,+,inN\n" "chr1,5520,+,afterN\n"
       "chrZ,100,+,nochrom\n"
       "chr1,6010|6011,-,revN\n" "chr1,6010,+,fwdN\n" "chr1,7302|7101,+,swapped\n" "chr2,1010,+,chr2site\n"
       "\n"
       "chr1,1010,+,ignored\n")


def seq_of(n):
    return ("ACGT" * (n // 4 + 1))[:n]


def qual_of(n):
    return bytes(i % 40 + 2 for i in range(n))


def rec(name, cigar, pos1, bc, umi, rn=None, flag=0, ref=0, seq=None, qual=None, extra=b""):
    import tagbammodel as tm

    n = sum(ln for op, ln in cigar if op in "MIS=X")
    aux = (tm.aux_z("BC", bc) if bc is not None else b"") + (tm.aux_z("U8", umi) if umi is not None else b"")
    if rn is not None:
        aux += tm.aux_int("RN", "C", rn)
    seq = seq_of(n) if seq is None else seq
    return bammodel.bam_record(name, flag, ref, pos1 - 1, 60, cigar, seq, qual_of(len(seq)) if qual is None else qual, aux=aux + extra)


def hand_records():
    M, D, N, I, S, H = "M", "D", "N", "I", "S", "H"
    n_seq = seq_of(100)[:10] + "N" + seq_of(100)[11:]
    return [
        rec("two", [(M, 400)], 7000, "CELL1", "UMI7"),
        rec("outside", [(S, 5), (M, 95)], 2000, "CELLX", "UMI8"),
        rec("fwd_del", [(M, 50), (D, 2), (M, 50)], 1000, "CELL1-1", "UMI1"),
        rec("clip", [(S, 5), (M, 95)], 2000, "CELL2", "UMI2", rn=1),
        rec("hclip", [(H, 5), (M, 100)], 3000, "CELL2", "UMI3", rn=5),
        rec("ins", [(M, 10), (I, 3), (M, 87)], 4000, "CELL1", "UMI1"),
        rec("gap", [(M, 20), (N, 500), (M, 80)], 5000, "CELL1", "UMI4"),
        rec("rev_n", [(M, 100)], 6000, "CELL3", "UMI5", flag=16, seq=n_seq),
        rec("fwd_n", [(M, 100)], 6000, "CELL3", "UMI6", seq=n_seq),
        rec("two", [(M, 400)], 7000, "CELL1", "UMI7", flag=256),
        rec("on_chr2", [(M, 100)], 1000, "CELL2", "UMI9", ref=1),
        rec("nobc", [(M, 100)], 1000, None, "UMI1"),
        rec("unmapped_flag", [(M, 100)], 1000, "CELL1", "UMI1", flag=4),
    ]


def hand_bam():
    return bammodel.bam_bytes(HEAD, REFS, hand_records())
