"""IsoformMatrix in plain Python (test infrastructure only): LongreadRecord's CIGAR walk and filter, UCSCRefFlatParser, CellList,
MoleculeDataset.setIsoformStrictNew and the Matrix writers, with DESIGN.md section 8d's rules in place of the reference's hash orders and
random pick: rows and cells in byte order, molinfos in (cell, UMI) order, an ambiguous tie goes to the smallest `txId|geneId`, a nomatch
tie to the gene whose first refFlat line comes first, reads of a molecule in order of their first kept record."""
import re
import struct

import bammodel
import consensusmodel as cm

COUNT_KEYS = ("records", "valid", "unvalid", "mapqv0", "no_gene", "no_umi", "chimeria", "null", "reads", "reads_multi", "molecules",
              "molecule_reads", "multi_ig", "genes", "transcripts", "monoexon", "nomatch", "onematch", "ambiguous", "cells", "matrix_genes",
              "matrix_junctions", "matrix_isoforms", "total_count", "isoforms_def", "isoforms_undef")


class IsoformError(RuntimeError):
    pass


def jsplit(s, sep):
    """String.split for a literal one-character separator: trailing empty strings removed ("".split -> [""])"""
    if s == "":
        return [""]
    out = s.split(sep)
    while out and out[-1] == "":
        out.pop()
    return out


def java_float(x):
    """Float.toString for a float32 value (the shortest decimal that reads back as the float)"""
    import numpy as np

    f = np.float32(x)
    if f != f:
        return "NaN"
    if np.isinf(f):
        return "Infinity" if f > 0 else "-Infinity"
    if f == 0:
        return "-0.0" if str(f).startswith("-") else "0.0"
    sci = np.format_float_scientific(f, unique=True, trim="-")
    sign = ""
    if sci[0] == "-":
        sign, sci = "-", sci[1:]
    mant, e = sci.split("e")
    exp = int(e)
    dig = mant.replace(".", "")
    if 1e-3 <= abs(float(f)) < 1e7:
        if exp >= 0:
            ip = dig[:exp + 1].ljust(exp + 1, "0")
            fp = dig[exp + 1:] or "0"
            return sign + ip + "." + fp
        return sign + "0." + "0" * (-exp - 1) + dig
    return sign + dig[0] + "." + (dig[1:] or "0") + "E" + str(exp)


# ---- LongreadRecord.fromSAMRecord L120-150 ----------------------------------------------------------------------------------------------
def alignment_blocks(pos1, cigar):
    """htsjdk getAlignmentBlocks: (reference start, length) per M / = / X"""
    blocks, ref = [], pos1
    for op, n in cigar:
        if op in "M=X":
            blocks.append((ref, n))
            ref += n
        elif op in "DN":
            ref += n
    return blocks


def junctions(pos1, cigar):
    """the reference's walk, literally (on the CIGAR text).  Raises IsoformError where the reference throws."""
    blocks = alignment_blocks(pos1, cigar)
    text = "".join(f"{n}{op}" for op, n in cigar)
    text = re.sub("[0-9]+[IS]", "", text)
    ctype = re.split("[0-9]+", text)
    csize = jsplit_re(text, "[A-Z]")
    while ctype and ctype[-1] == "" and len(ctype) > 1:
        ctype.pop()
    try:
        if not blocks:
            raise IndexError
        s = e = blocks[0][0]
        starts, ends = [], []
        bi = 0
        for i in range(len(csize)):
            if bi >= len(blocks) or i >= len(ctype):
                raise IndexError
            cs, cl = blocks[bi]
            t = ctype[i]
            if t == "M":
                bi += 1
            if t == "N":
                starts.append(s)
                ends.append(e)
                s = cs
            elif t == "D" and int(csize[i - 1]) > 20:
                starts.append(s)
                ends.append(e)
                s = cs
            if t != "D":
                e = cs + cl - 1
        starts.append(s)
        ends.append(e)
    except (IndexError, ValueError):
        raise IsoformError("the CIGAR walk runs past the alignment blocks")
    return [(ends[i - 1], starts[i]) for i in range(1, len(starts))]


def jsplit_re(s, pat):
    if s == "":
        return [""]
    out = re.split(pat, s)
    while out and out[-1] == "":
        out.pop()
    return out


# ---- UCSCRefFlatParser / TranscriptRecord ----------------------------------------------------------------------------------------------
def parse_refflat(text):
    """-> (genes in order of their first line, {gene: [(tx, junctions, n_exons), ...] in file order}, lines kept)"""
    genes, by_gene, n = [], {}, 0
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for no, line in enumerate(lines, 1):
        line = line.rstrip("\r")
        f = jsplit(line, "\t")
        if len(f) < 11:
            raise IsoformError(f"REFFLAT line {no}: has {len(f)} fields, at least 11 are needed")
        try:
            for k in range(4, 9):
                int(f[k])
            xs = [int(v) for v in jsplit(f[9].rstrip(","), ",")]
            xe = [int(v) for v in jsplit(f[10].rstrip(","), ",")]
        except ValueError:
            raise IsoformError(f"REFFLAT line {no}: not an integer")
        if len(xe) < len(xs):
            raise IsoformError(f"REFFLAT line {no}: fewer exon ends than exon starts")
        if sum(xe[i] - xs[i] for i in range(len(xs))) == 0:
            continue
        n += 1
        exons = [(xs[i] + 1, xe[i]) for i in range(len(xs))]
        junc = [(exons[i - 1][1], exons[i][0]) for i in range(1, len(exons))]
        if f[0] not in by_gene:
            genes.append(f[0])
            by_gene[f[0]] = []
        by_gene[f[0]].append((f[1], junc, len(exons)))
    return genes, by_gene, n


def select(by_gene, gene, tx):
    """select(gene, tx): the last line of that transcript -> its exon count, 0 if none"""
    nex = 0
    for t, _j, ne in by_gene.get(gene, []):
        if t == tx:
            nex = ne
    return nex


def cell_list(text):
    """CellList: every line with "-1" removed, as a sorted list of distinct cells (an empty text has no line)"""
    if text == "":
        return []
    return sorted(set(line.replace("-1", "") for line in re.split("\r\n|\r|\n", text)[:-1 if re.search("(\r\n|\r|\n)$", text) else None]))


# ---- records, reads, molecules --------------------------------------------------------------------------------------------------------
def parse_records(bam, cfg):
    _text, _refs, recs = bammodel.parse_bam(bam)
    cnt = dict.fromkeys(COUNT_KEYS, 0)
    kept = []
    for r in recs:
        cnt["records"] += 1
        name = r["name"]
        aux = cm._split_aux(r["aux"])

        def get(tag, want):
            try:
                return cm._value(aux.get(tag), want, name, tag)
            except cm.ConsensusError as e:
                raise IsoformError(str(e))
        gene = get(cfg["gene_tag"], "Z")
        bc = get(cfg["cell_tag"], "Z")
        umi = get(cfg["umi_tag"], "Z")
        if bc is None or r["flag"] & 4:
            cnt["unvalid"] += 1
            cnt["null"] += 1
            continue
        de = get("de", "f")
        if de is None:
            de = get("df", "f")
        if de is None:
            de = 1.0
        rn = get(cfg["rn_tag"], "i")
        rn = 1 if rn is None else rn
        cig = r["cigar"]
        if not cig:
            raise IsoformError(f"read {name}: no CIGAR")
        clip = lambda c: c[0] in "SH" and c[1] > cfg["max_clip"]  # noqa: E731
        chim = clip(cig[0]) or clip(cig[-1])
        try:
            junc = junctions(r["pos0"] + 1, cig)
        except IsoformError as e:
            raise IsoformError(f"read {name}: {e}")
        if chim:
            cnt["unvalid"] += 1
            cnt["chimeria"] += 1
            continue
        if gene is None or gene in (b"", b"undef"):
            cnt["unvalid"] += 1
            cnt["no_gene"] += 1
            continue
        if umi is None:
            cnt["unvalid"] += 1
            cnt["no_umi"] += 1
            continue
        if not cfg["mapqv0"] and r["mapq"] == 0 and r["flag"] & 0x900:
            cnt["unvalid"] += 1
            cnt["mapqv0"] += 1
            continue
        cnt["valid"] += 1
        kept.append(dict(name=name, bc=bc.replace(b"-1", b"").decode(), umi=umi.decode(), gene=gene.decode(), rn=rn,
                         de=struct.unpack("<f", struct.pack("<f", de))[0], junc=junc))
    return kept, cnt


def molecules(kept, cnt):
    reads = {}
    for k in kept:
        reads.setdefault(k["name"], []).append(k)
    cnt["reads"] = len(reads)
    cnt["reads_multi"] = sum(len(v) > 1 for v in reads.values())
    mols = {}
    for recs in reads.values():
        last = recs[-1]
        key = last["bc"] + ":" + last["umi"]
        if key not in mols:
            mols[key] = dict(bc=last["bc"], umi=last["umi"], rn=last["rn"], reads=[], genes=set())
        m = mols[key]
        m["reads"].append(recs)
        for rr in recs:
            m["genes"].update(jsplit(rr["gene"], ","))
    cnt["molecules"] = len(mols)
    cnt["molecule_reads"] = len(reads)
    cnt["multi_ig"] = sum(len(m["genes"]) > 1 for m in mols.values())
    return mols


def is_in(j, lst, d):
    return any(abs(x[0] - j[0]) <= d and abs(x[1] - j[1]) <= d for x in lst)


def assign(m, genes, by_gene, delta, cnt):
    """setIsoformStrictNew -> sets gene, tx, support, junctions"""
    mg = sorted((g for g in m["genes"] if g in by_gene), key=genes.index)
    T = [(g, t) for g in mg for t in by_gene[g]]
    m.update(gene="undef", tx="undef", support=0, jset=set())
    if len(T) == 1 and not T[0][1][1]:
        cnt["monoexon"] += 1
        m.update(gene=T[0][0], tx=T[0][1][0], support=1)
        return
    cand = {}
    for recs in m["reads"]:
        for rr in recs:
            rj = rr["junc"]
            for g, (tx, tj, _ne) in T:
                ok = bool(tj) and len(tj) == len(rj) and all(is_in(j, rj, delta) for j in tj)
                for j in tj:
                    if is_in(j, rj, delta):
                        m["jset"].add(j)
                if ok:
                    k = tx + "|" + g
                    cand[k] = cand.get(k, 0) + 1
    if cand:
        best = max(cand.values())
        tied = sorted(k for k, v in cand.items() if v == best)
        cnt["onematch" if len(tied) == 1 else "ambiguous"] += 1
        tx, g = tied[0].split("|")
        m.update(gene=g, tx=tx, support=best)
    elif T:
        cnt["nomatch"] += 1
        lines = {}
        for g, _t in T:
            lines[g] = lines.get(g, 0) + 1
        top = max(lines.values())
        m.update(gene=next(g for g in mg if lines[g] == top))


def isoform_matrix(bam, refflat, csv, delta=2, mapqv0=False, to_bulk=False, cell_tag="BC", umi_tag="U8", gene_tag="GE", rn_tag="RN",
                   max_clip=150, isobam=False):
    """-> ({file name suffix: bytes}, counts); with isobam also "isobam.bam": the inflated ISOBAM"""
    cfg = dict(cell_tag=cell_tag, umi_tag=umi_tag, gene_tag=gene_tag, rn_tag=rn_tag, max_clip=max_clip, mapqv0=mapqv0)
    genes, by_gene, n_lines = parse_refflat(refflat)
    cells = cell_list(csv)
    kept, cnt = parse_records(bam, cfg)
    by_key = molecules(kept, cnt)
    mols = list(by_key.values())
    cnt["genes"], cnt["transcripts"], cnt["cells"] = len(genes), n_lines, len(cells)
    for m in mols:
        assign(m, genes, by_gene, delta, cnt)
    counted = [m for m in mols if m["bc"] in set(cells) and m["gene"] in by_gene]
    iso, gen, jun = {}, {}, {}
    for m in counted:
        iso.setdefault(m["gene"] + "\t" + m["tx"], {}).setdefault(m["bc"], set()).add(m["umi"])
        gen.setdefault(m["gene"], {}).setdefault(m["bc"], set()).add(m["umi"])
        for s, e in m["jset"]:
            jun.setdefault(f"{m['gene']}:{s}-{e}", {}).setdefault(m["bc"], set()).add(m["umi"])
    head = "".join("\t" + c for c in cells) + "\n"
    out = {}

    def dense(mat, label):
        rows, tot = [], {}
        for k in sorted(mat):
            vals = [len(mat[k].get(c, ())) for c in cells]
            tot[k] = sum(vals)
            rows.append(label(k) + "".join(f"\t{v}" for v in vals) + "\n")
        return "".join(rows), tot

    nex = {k: select(by_gene, *k.split("\t")) for k in iso}
    body, iso_tot = dense(iso, lambda k: f"{k}\t{nex[k]}")
    out["isomatrix.txt"] = "geneId\ttranscriptId\tnbExons" + head + body
    out["isometrics.txt"] = "geneId\ttranscriptId\tnbExons\tnbUmis\n" + "".join(f"{k}\t{nex[k]}\t{iso_tot[k]}\n" for k in sorted(iso))
    cnt["total_count"] = sum(iso_tot.values())
    body, gene_tot = dense(gen, lambda k: k)
    out["genematrix.txt"] = "geneId" + head + body
    body, junc_tot = dense(jun, lambda k: k)
    out["juncmatrix.txt"] = "junctionId" + head + body
    out["juncmetrics.txt"] = "junctionId\tnbUmis\n" + "".join(f"{k}\t{junc_tot[k]}\n" for k in sorted(jun))
    gk, gu = {}, {}
    cm_ = {c: dict(reads=0, genes=set(), umis=0, known=0, undef=0) for c in cells}
    for m in counted:
        und = m["tx"] == "undef"
        (gu if und else gk)[m["gene"]] = (gu if und else gk).get(m["gene"], 0) + 1
        x = cm_[m["bc"]]
        x["reads"] += len(m["reads"])
        x["genes"].add(m["gene"])
        x["umis"] += 1
        x["undef" if und else "known"] += 1
        cnt["isoforms_undef" if und else "isoforms_def"] += 1
    out["genemetrics.txt"] = "geneId\tnbUmis\tnbIsoformSet\tnbIsoformNotSet\n" + "".join(
        f"{g}\t{gk.get(g, 0) + gu.get(g, 0)}\t{gk.get(g, 0)}\t{gu.get(g, 0)}\n" for g in sorted(gen))
    out["cellmetrics.txt"] = "cellBC\tnbReads\tnbGenes\tnbUmis\tnbIsoformSet\tnbIsoformNotSet\n" + "".join(
        f"{c}\t{x['reads']}\t{len(x['genes'])}\t{x['umis']}\t{x['known']}\t{x['undef']}\n" for c, x in cm_.items())
    mi = ["cellBC\tUMI\tnbReads\tnbSupportingReads\tmappingPctId\tsnpPhredScore\tgeneId\ttranscriptId\n"]
    for m in sorted(counted, key=lambda m: (m["bc"].encode(), m["umi"].encode())):
        nreads = m["rn"] if m["rn"] > 1 else len(m["reads"])
        import numpy as np
        pct = np.float32(1.0) - np.float32(m["reads"][-1][0]["de"])
        mi.append(f"{m['bc']}\t{m['umi']}\t{nreads}\t{m['support']}\t{java_float(pct)}\t\t{m['gene']}\t{m['tx']}\n")
    out["molinfos.txt"] = "".join(mi)
    if to_bulk:
        bg = "geneId\tcount\n" + "".join(f"{g}\t{gene_tot[g]}\n" for g in sorted(gen)) + "".join(f"{k}\t{nex[k]}" for k in sorted(iso))
        bi = "transcriptId\texons\tcount\n" + "".join(f"{k}\t{nex[k]}\t{iso_tot[k]}\n" for k in sorted(iso))
        out["bulkgene.txt"], out["bulkiso.txt"] = bg, bi
    cnt["matrix_genes"], cnt["matrix_junctions"], cnt["matrix_isoforms"] = len(gen), len(jun), len(iso)
    res = {k: v.encode() for k, v in out.items()}
    if isobam:
        res["isobam.bam"] = isobam_bytes(bam, by_key, cell_tag, umi_tag)
    return res, cnt


def unsorted_header(text):
    """the header text of PREFIX_isobam.bam: SO:unsorted in the @HD line (an SO value replaced where it stands, else
    appended to the line); no @HD line: `@HD\tVN:1.6\tSO:unsorted` in front"""
    if text.startswith("@HD"):
        first, nl, rest = text.partition("\n")
        f = first.split("\t")
        so = [i for i in range(1, len(f)) if f[i].startswith("SO:")]
        if so:
            f[so[0]] = "SO:unsorted"
        else:
            f.append("SO:unsorted")
        return "\t".join(f) + nl + rest
    return "@HD\tVN:1.6\tSO:unsorted\n" + text


def isobam_bytes(bam, by_key, cell_tag, umi_tag):
    """IsoformMatrix.java L135-159 on an inflated BAM -> the inflated isobam: every record, IG / IT of the molecule keyed by the RAW cell
    and UMI strings ("null" when missing), "undef" otherwise; attributes by htsjdk's rules (assignumis.apply_tag_sets)"""
    import importlib

    import __graft_entry__ as graft
    graft.load_package()
    au = importlib.import_module(graft.PKG_NAME + ".assignumis")
    l_text = struct.unpack_from("<I", bam, 4)[0]
    text = unsorted_header(bam[8:8 + l_text].decode("latin-1")).encode("latin-1")
    p = 8 + l_text
    n_ref = struct.unpack_from("<I", bam, p)[0]
    q = p + 4
    for _ in range(n_ref):
        q += 8 + struct.unpack_from("<I", bam, q)[0]
    out = [b"BAM\1", struct.pack("<I", len(text)), text, bam[p:q]]
    while q < len(bam):
        bs = struct.unpack_from("<I", bam, q)[0]
        body = bam[q + 4:q + 4 + bs]
        q += 4 + bs
        l_nm, n_cig, l_seq = body[8], struct.unpack_from("<H", body, 12)[0], struct.unpack_from("<i", body, 16)[0]
        a = 32 + l_nm + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        fields = au.split_aux(body[a:])
        raw = {t: v for t, v in fields}
        get = lambda t: raw[t][3:-1].decode() if t in raw else "null"  # noqa: E731
        m = by_key.get(get(cell_tag) + ":" + get(umi_tag))
        ig, it = (m["gene"], m["tx"]) if m is not None else ("undef", "undef")
        new = body[:a] + b"".join(v for _, v in au.apply_tag_sets(fields, [("IG", ig), ("IT", it)]))
        out.append(struct.pack("<I", len(new)) + new)
    return b"".join(out)
