"""FusionDetector in plain Python (test infrastructure only): LongreadRecord.fromSAMRecord L71-184 and LongreadParser L42-115 with the
fixed parameters of FusionDetector.java L63-67, Longread.addRecord L40-54, MoleculeDataset(LongreadParser) L60-98 with
Molecule.addLongread L127-135, the selection and the key of FusionDetector.java L76-92 and Matrix.writeIsoformMatrix L158-223 with
model == null, literally, with DESIGN.md section 8i's rules in place of the reference's hash orders: cells and rows in byte order,
molinfos in (cell, UMI) byte order, two names of one HashSet bucket in byte order, the reads of a molecule in order of their first kept
record, a UMI whose text is `null` apart from a missing UMI, and an error (FusionError, naming the read) where the reference's parse loop
dies on an exception."""
import struct

import numpy as np

import bammodel
import consensusmodel as cm
import isoformmodel as im

MAXCLIP = 10000                                             # FusionDetector.java L64
COUNT_KEYS = ("records", "valid", "unvalid", "mapqv0", "no_gene", "no_umi", "chimeria", "null", "reads", "reads_multi", "molecules",
              "molecule_reads", "multi_ig", "cells", "gene_fields", "genes", "counted", "rows")
SUFFIXES = ("_fusmatrix.txt", "_fusmetrics.txt", "_fusmolinfos.txt")
MOLINFOS_HEAD = "cellBC\tUMI\tnbReads\tnbSupportingReads\tmappingPctId\tsnpPhredScore\tgeneId\ttranscriptId\n"


class FusionError(RuntimeError):
    def __init__(self, read, why):
        super().__init__(f"read {read}: {why}")
        self.read = read


def java_split(s):
    """String.split(","): trailing empty strings removed, the others kept ("".split(",") is [""], but an empty GE never gets here)"""
    return im.jsplit(s, ",")


def java_hash(name):
    """String.hashCode over the bytes of a name, as a 32-bit unsigned value"""
    h = 0
    for c in name.encode("latin-1"):
        h = (31 * h + c) & 0xFFFFFFFF
    return h


def bucket(name):
    """the bucket of a name in a java.util.HashSet of 16: (h ^ (h >>> 16)) & 15"""
    h = java_hash(name)
    return (h ^ (h >> 16)) & 15


def set_order(names):
    """iteration order of a two-element HashSet: by bucket; a shared bucket: byte order (deviation 2)"""
    return sorted(names, key=lambda g: (bucket(g), g.encode("latin-1")))


def fusion_key(names):
    """set.toString() through the three replace calls of FusionDetector.java L82-85"""
    key = "[" + ", ".join(set_order(names)) + "]"
    return key.replace(", ", "|").replace("[", "").replace("]", "")


def parse_records(bam, cnt):
    """-> the kept records in file order"""
    _text, _refs, recs = bammodel.parse_bam(bam)
    kept = []
    for r in recs:
        cnt["records"] += 1
        name = r["name"]
        aux = cm._split_aux(r["aux"])

        def get(tag, want):
            try:
                return cm._value(aux.get(tag), want, name, tag)
            except cm.ConsensusError:
                raise FusionError(name, f"attribute {tag} is not of the type FusionDetector reads")
        gene, bc, umi = get("GE", "Z"), get("BC", "Z"), get("U8", "Z")          # L75-77: the casts come first
        if bc is None or r["flag"] & 4:                                            # L80
            cnt["unvalid"] += 1
            cnt["null"] += 1
            continue
        de = get("de", "f")
        if de is None:
            de = get("df", "f")
        if de is None:
            de = 1.0
        rn = get("RN", "i")
        rn = 1 if rn is None else rn
        cig = r["cigar"]
        if not cig:
            raise FusionError(name, "no CIGAR")
        try:
            im.junctions(r["pos0"] + 1, cig)                                       # the exon walk runs for every record that is not null
        except im.IsoformError as e:
            raise FusionError(name, str(e))
        clip = lambda c: c[0] in "SH" and c[1] > MAXCLIP  # noqa: E731
        if clip(cig[0]) or clip(cig[-1]):                                          # LongreadParser L101
            cnt["unvalid"] += 1
            cnt["chimeria"] += 1
        elif gene is None or gene in (b"", b"undef"):                              # L102
            cnt["unvalid"] += 1
            cnt["no_gene"] += 1
        elif r["mapq"] == 0 and r["flag"] & 0x900:                                 # L105-111: a primary record of mapq 0 is kept
            cnt["unvalid"] += 1
            cnt["mapqv0"] += 1
        else:
            cnt["valid"] += 1
            kept.append(dict(name=name, bc=bc.replace(b"-1", b"").decode("latin-1"), umi=None if umi is None else umi.decode("latin-1"),
                             genes=java_split(gene.decode("latin-1")), rn=rn, de=struct.unpack("<f", struct.pack("<f", de))[0]))
    return kept


def molecules(kept, cnt):
    """Longread.addRecord and MoleculeDataset(LongreadParser): -> the molecules in order of their first read"""
    reads = {}
    for k in kept:
        rd = reads.setdefault(k["name"], dict(records=[], genes=set(), bc=None, umi=None, rn=1))
        rd["genes"].update(k["genes"])
        rd["bc"] = k["bc"]
        if k["umi"] is not None:
            rd["umi"] = k["umi"]
        rd["rn"] = k["rn"]
        rd["records"].append(k)
    cnt["reads"] = len(reads)
    cnt["reads_multi"] = sum(len(rd["records"]) > 1 for rd in reads.values())
    cnt["gene_fields"] = sum(len(k["genes"]) for k in kept)
    cnt["genes"] = len(set(g for k in kept for g in k["genes"]))
    mols = {}
    for rd in reads.values():                                # (reads in order of their first kept record: deviation 3)
        key = (rd["bc"] + ":" + (rd["umi"] or ""), rd["umi"] is not None)   # "null" is a text of its own: deviation 4
        if key not in mols:
            mols[key] = dict(bc=rd["bc"], umi=rd["umi"], rn=rd["rn"], reads=[], genes=set(), pct=None)
        m = mols[key]
        m["reads"].append(rd)
        m["pct"] = np.float32(1.0) - np.float32(rd["records"][0]["de"])
        m["genes"].update(rd["genes"])
    cnt["molecules"] = len(mols)
    cnt["molecule_reads"] = sum(len(m["reads"]) for m in mols.values())
    cnt["multi_ig"] = sum(len(m["genes"]) > 1 for m in mols.values())
    return list(mols.values())


def fusion_detector(bam, csv):
    """-> ({file name suffix: bytes}, counts, [(key, molecules)] in row order, the molecules)"""
    cnt = dict.fromkeys(COUNT_KEYS, 0)
    cells = im.cell_list(csv) if csv else []
    cnt["cells"] = len(cells)
    mols = molecules(parse_records(bam, cnt), cnt)
    counted = [m for m in mols if m["bc"] in set(cells) and m["umi"] is not None and len(m["genes"]) == 2]
    matrix = {}
    for m in counted:
        m["key"] = fusion_key(m["genes"])
        matrix.setdefault(m["key"], {}).setdefault(m["bc"], set()).add(m["umi"])
    rows = sorted(matrix, key=lambda k: k.encode("latin-1"))
    cnt["counted"], cnt["rows"] = len(counted), len(rows)
    mat = "geneId\ttranscriptId\tnbExons" + "".join("\t" + c for c in cells) + "\n"
    met = "geneId\ttranscriptId\tnbExons\tnbUmis\n"
    fusions = []
    for k in rows:
        vals = [len(matrix[k].get(c, ())) for c in cells]
        mat += f"{k}\t{k}\tna" + "".join(f"\t{v}" for v in vals) + "\n"
        met += f"{k}\t{k}\tna\t{sum(vals)}\n"
        fusions.append((k, sum(vals)))
    mi = MOLINFOS_HEAD
    for m in sorted(counted, key=lambda m: (m["bc"].encode("latin-1"), m["umi"].encode("latin-1"))):
        nreads = m["rn"] if m["rn"] > 1 else len(m["reads"])
        mi += f"{m['bc']}\t{m['umi']}\t{nreads}\t0\t{im.java_float(m['pct'])}\t\t{m['key']}\t{m['key']}\n"
    out = dict(zip(SUFFIXES, (mat, met, mi)))
    return {k: v.encode("latin-1") for k, v in out.items()}, cnt, fusions, mols


def statistics_lines(c, fusions):
    """FusionDetector.java L60, L70, L103; LongreadParser.java L51, L84-93; MoleculeDataset.java L63, L85, L96-97"""
    lines = [f"\tCells detected\t[{c['cells']}]", "\tstart...", "\tend...", f"\tTotal SAMrecords\t{c['records']}",
             f"\tSAMrecords valid\t{c['valid']}", f"\tSAMrecords unvalid\t{c['unvalid']}", f"\tSAMrecords mapqv=0\t{c['mapqv0']}",
             f"\tSAMrecords no gene\t{c['no_gene']}", f"\tSAMrecords no UMI\t{c['no_umi']}", f"\tSAMrecords chimeria\t{c['chimeria']}",
             f"\tTotal reads\t\t{c['reads']}", f"\tTotal reads multiSAM\t{c['reads_multi']}", "\tMoleculeDataset init start...",
             f"\tTotal molecules\t\t{c['molecules']}", f"\tTotal molecule reads\t{c['molecule_reads']}",
             f"\tTotal molecule multiIG\t{c['multi_ig']}", "\tSetFusions\t\tstart..."]
    for key, n in sorted(fusions, key=lambda kv: (-kv[1], kv[0].encode("latin-1"))):
        if n >= 10:
            lines.append(f"\t{n} distincts molecules support fusion [{key}]")
    return lines
