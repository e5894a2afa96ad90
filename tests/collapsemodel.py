"""CollapseModel in plain Python (test infrastructure only): UCSCRefFlatParser's loader, collapser / collapse, initialize, filter /
isPartOfLonger, classifier / noveltyDetector, statistics and exportFiles over TranscriptRecord's printers, literally, with DESIGN.md
section 8h's rules in place of the reference's hash order and index queries: genes in byte order of their name, evidence in
reference-dictionary order then file order, and an error (CollapseError, naming the read) where the reference throws inside the loader."""
import bammodel
import consensusmodel as cm
import isoformmodel as im

COUNT_KEYS = ("records", "kept", "null", "mapq0", "chimeric", "low_rn", "not_listed", "no_gene", "cells", "model_genes", "model_transcripts",
              "genes", "undef_records", "monoexon", "founders", "novel_evidenced", "novel_filtered", "isoforms", "evidences", "gencode",
              "gencode_ev", "ckj", "ckj_ev", "cks", "cks_ev", "nss", "nss_ev", "max_undef", "max_founders")
SUFFIXES = (".txt", ".refflat.txt", ".final.refflat.txt", ".gff", ".final.gff")
DEFAULTS = dict(cell_tag="BC", umi_tag="U8", gene_tag="IG", iso_tag="IT", rn_tag="RN", max_clip=150, delta=2, min_evidence=2, rn_min=1)
LEGEND = ("geneId\ttranscriptId\tchrom\tstrand\ttxStart\ttxEnd\texons\tUMIs\tCells\tcategorie\tsubcategorie\tnovelJunctions"
          "\tnovelJunctions_reads\tis_valid_allNovelJunctions\tdist_cage\tis_valid_cage\tdist_polya\tis_valid_polya\tis_valid\n")
COLORS = {"gencode": "#014e8e", "combination_of_known_junctions": "#9dd122", "combination_of_known_splicesites": "#c594e1",
          "at_least_one_novel_splicesite": "#e65802"}


class CollapseError(RuntimeError):
    def __init__(self, read, why):
        super().__init__(f"read {read}: {why}")
        self.read = read


class Tx:
    """TranscriptRecord"""

    def __init__(self, gene, tx):
        self.gene, self.tx = gene, tx
        self.evidence = []
        self.is_novel, self.is_known = False, True
        self.categorie, self.subcategorie = "undef", "undef2"
        self.novel_junctions = []
        self.exons = None
        self.chrom = self.strand = None
        self.tx_start = self.tx_end = self.cds_start = self.cds_end = 0
        self.nb_umis = self.nb_cells = 0

    def junctions(self):                                   # junctionsFromExons
        return [(self.exons[i - 1][1], self.exons[i][0]) for i in range(1, len(self.exons))]

    def initialize(self):
        lo, hi = 2 ** 31 - 1, -2 ** 31
        for r in self.evidence:
            self.strand, self.chrom = r["strand"], r["chrom"]
            lo, hi = min(lo, r["tx_start"]), max(hi, r["tx_end"])
        if self.is_novel:
            self.categorie, self.subcategorie = "undef", "undef2"
            self.exons[0][0] = lo
            self.exons[-1][1] = hi
            self.tx_start = self.cds_start = lo
            self.tx_end = self.cds_end = hi
        if self.is_known:
            self.categorie, self.subcategorie = "full_splice_match", "gencode"
        self.nb_umis = len(self.evidence)
        self.nb_cells = len(set(r["barcode"] for r in self.evidence))

    def novel_text(self):
        return ",".join(f"{a}-{b}" for a, b in self.novel_junctions) or "-"

    def print_txt(self):
        return (f"{self.gene}\t{self.tx}\t{self.chrom}\t{self.strand}\t{self.tx_start}\t{self.tx_end}\t{len(self.exons)}\t{self.nb_umis}\t"
                f"{self.nb_cells}\t{self.categorie}\t{self.subcategorie}\t{self.novel_text()}\t0\tfalse\t0\tfalse\t0\tfalse\tfalse\n")

    def print_refflat(self):
        return (f"{self.gene}\t{self.tx}\t{self.chrom}\t{self.strand}\t{self.tx_start}\t{self.tx_end}\t{self.cds_start}\t{self.cds_end}\t"
                f"{len(self.exons)}\t" + "".join(f"{e[0] - 1}," for e in self.exons) + "\t" + "".join(f"{e[1]}," for e in self.exons) + "\n")

    def print_gff(self):
        ids = f'gene_id "{self.gene}"; transcript_id "{self.tx}";'
        s = (f'{self.chrom}\tsicelore\ttranscript\t{self.tx_start}\t{self.tx_end}\t.\t{self.strand}\t.\t{ids} category "{self.categorie}"; '
             f'subcategory "{self.subcategorie}"; UMIs "{self.nb_umis}"; Cells "{self.nb_cells}"; novelJunctions "{self.novel_text()}"; '
             f'supportingReads "0"; CAGEdist "0"; POLYAdist "0"; color "{COLORS.get(self.subcategorie, "#000000")}";\n')
        for a, b in self.exons:
            s += f"{self.chrom}\tsicelore\texon\t{a}\t{b}\t.\t{self.strand}\t.\t{ids}\n"
        return s


def parse_refflat(text):
    """UCSCRefFlatParser(File): {gene: [Tx of every kept line, in file order]} -- known transcripts with the refFlat's numbers"""
    model, n = {}, 0
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    for no, line in enumerate(lines, 1):
        f = im.jsplit(line.rstrip("\r"), "\t")
        if len(f) < 11:
            raise im.IsoformError(f"REFFLAT line {no}: has {len(f)} fields, at least 11 are needed")
        if f[3] not in ("+", "-", "."):
            raise im.IsoformError(f"REFFLAT line {no}: field 4 is no strand")
        try:
            nums = [int(f[k]) for k in range(4, 9)]
            xs = [int(v) for v in im.jsplit(f[9].rstrip(","), ",")]
            xe = [int(v) for v in im.jsplit(f[10].rstrip(","), ",")]
        except ValueError:
            raise im.IsoformError(f"REFFLAT line {no}: not an integer")
        if len(xe) < len(xs):
            raise im.IsoformError(f"REFFLAT line {no}: fewer exon ends than exon starts")
        if sum(xe[i] - xs[i] for i in range(len(xs))) == 0:
            continue
        n += 1
        t = Tx(f[0], f[1])
        t.tx_start, t.tx_end, t.cds_start, t.cds_end = nums[:4]
        t.exons = [[xs[i] + 1, xe[i]] for i in range(len(xs))]
        model.setdefault(f[0], []).append(t)
    return model, n


def select(model, gene, tx):
    """select(geneId, transcriptId): the last line of that gene with that transcript id, or None"""
    found = None
    for t in model.get(gene, []):
        if t.tx == tx:
            found = t
    return found


def load(bam, model, cells, cfg, cnt):
    """loader: {gene: [Tx]} in the order the transcripts are first seen; the evidence in reference-dictionary order, then file order"""
    _text, refs, recs = bammodel.parse_bam(bam)
    kept = []
    for r in recs:
        cnt["records"] += 1
        name = r["name"]
        aux = cm._split_aux(r["aux"])

        def get(tag, want):
            try:
                return cm._value(aux.get(tag), want, name, tag)
            except cm.ConsensusError:
                raise CollapseError(name, f"attribute {tag} is not of the type CollapseModel reads")
        bc, _umi, ig, it = (get(cfg[k], "Z") for k in ("cell_tag", "umi_tag", "gene_tag", "iso_tag"))
        rn = get(cfg["rn_tag"], "i")
        rn = 1 if rn is None else rn
        if bc is None or r["flag"] & 4 or r["ref_id"] < 0:
            cnt["null"] += 1
            continue
        if get("de", "f") is None:
            get("df", "f")
        cig = r["cigar"]
        if not cig:
            raise CollapseError(name, "no CIGAR")
        try:
            junc = im.junctions(r["pos0"] + 1, cig)
        except im.IsoformError as e:
            raise CollapseError(name, str(e))
        clip = lambda c: c[0] in "SH" and c[1] > cfg["max_clip"]  # noqa: E731
        bc, ig = bc.decode("latin-1"), None if ig is None else ig.decode("latin-1")
        if r["mapq"] == 0:
            cnt["mapq0"] += 1
        elif clip(cig[0]) or clip(cig[-1]):
            cnt["chimeric"] += 1
        elif rn < cfg["rn_min"]:
            cnt["low_rn"] += 1
        elif bc not in cells:
            cnt["not_listed"] += 1
        elif ig is None or ig in ("", "undef"):
            cnt["no_gene"] += 1
        else:
            it = None if it is None else it.decode("latin-1")
            if it != "undef" and select(model, ig, it) is None:
                raise CollapseError(name, "no ISOFORMTAG attribute" if it is None else f"transcript {it} is no transcript of gene {ig}")
            cnt["kept"] += 1
            end = r["pos0"] + sum(n for op, n in cig if op in "MDN=X")
            kept.append(dict(name=name, gene=ig, it=it, ref_id=r["ref_id"], chrom=refs[r["ref_id"]][0], strand="-" if r["flag"] & 16 else "+",
                             tx_start=r["pos0"] + 1, tx_end=end, barcode=bc.replace("-1", ""), junctions=junc))
    kept.sort(key=lambda r: r["ref_id"])                   # stable: file order within a sequence
    genes = {}
    for r in kept:
        lst = genes.setdefault(r["gene"], [])
        t = next((t for t in lst if t.tx == r["it"]), None)
        if t is None:
            t = Tx(r["gene"], "undef") if r["it"] == "undef" else select(model, r["gene"], r["it"])
            lst.append(t)
        t.evidence.append(r)
    return genes


def is_in(j, lst, delta):
    return any(abs(a[0] - j[0]) <= delta and abs(a[1] - j[1]) <= delta for a in lst)


def is_exact_same_structure(junc_lrr, junc_tr, delta):
    if len(junc_tr) > 0 and len(junc_tr) == len(junc_lrr):
        return all(is_in(junc_tr[i], junc_lrr, delta) for i in range(len(junc_lrr)))
    return False


def is_all_include(j1, j2, delta):
    return all(is_in(a, j2, delta) for a in j1)


def collapse(records, gene, delta, index):
    """collapse(): -> the founders in creation order; index[0] is NOVELINDEX"""
    novel = []
    for r in records:
        seen = False
        for t in novel:
            if is_exact_same_structure(r["junctions"], t.junctions(), delta):
                if not seen:
                    t.evidence.append(r)
                seen = True
        if not seen and r["junctions"]:
            t = Tx(gene, f"Novel.{index[0]}")
            index[0] += 1
            t.is_novel, t.is_known = True, False
            j = r["junctions"]
            # the record's exons: first start and last end are replaced in initialize(); the junctions are all that is read before
            t.exons = [[r["tx_start"] if i == 0 else j[i - 1][1], j[i][0] if i < len(j) else r["tx_end"]] for i in range(len(j) + 1)]
            t.evidence.append(r)
            novel.append(t)
    return novel


def novelty_detector(t, model_list, delta):
    mj = [j for m in model_list for j in m.junctions()]
    splice = set(x for j in mj for x in j)
    for j in t.junctions():
        if not is_in(j, mj, delta):
            if j[0] in splice and j[1] in splice:
                if t.categorie == "undef":
                    t.categorie, t.subcategorie = "novel_in_catalog", "combination_of_known_splicesites"
                t.novel_junctions.append(j)
            else:
                t.categorie, t.subcategorie = "novel_not_in_catalog", "at_least_one_novel_splicesite"
                t.novel_junctions.append(j)
    if t.categorie == "undef":
        t.categorie, t.subcategorie = "novel_in_catalog", "combination_of_known_junctions"


def collapse_model(bam, refflat, csv, **kw):
    """-> ({suffix: bytes}, counts, per gene detail for the edge assertions)"""
    cfg = dict(DEFAULTS, **kw)
    delta = cfg["delta"]
    cnt = dict.fromkeys(COUNT_KEYS, 0)
    model, n_lines = parse_refflat(refflat)
    cells = set(im.cell_list(csv)) if csv else set()
    cnt["cells"], cnt["model_genes"], cnt["model_transcripts"] = len(cells), len(model), n_lines
    genes = load(bam, model, cells, cfg, cnt)
    order = sorted(genes, key=lambda g: g.encode("latin-1"))
    cnt["genes"] = len(genes)
    index = [1]
    detail = {}
    for g in order:                                        # collapser
        lst = genes[g]
        d = detail[g] = dict(undef=0, founders=[], dropped=[], kept=[])
        undef = next((t for t in lst if t.tx == "undef"), None)
        if undef is not None:
            cnt["undef_records"] += len(undef.evidence)
            cnt["monoexon"] += sum(1 for r in undef.evidence if not r["junctions"])
            cnt["max_undef"] = max(cnt["max_undef"], len(undef.evidence))
            d["undef"] = len(undef.evidence)
            novel = collapse(undef.evidence, g, delta, index)
            d["founders"] = [(t.tx, len(t.evidence)) for t in novel]
            cnt["founders"] += len(novel)
            cnt["max_founders"] = max(cnt["max_founders"], len(novel))
            lst.remove(undef)
            for t in novel:
                if len(t.evidence) >= cfg["min_evidence"]:
                    lst.append(t)
                    cnt["novel_evidenced"] += 1
    for g in order:                                        # initialize
        for t in genes[g]:
            t.initialize()
    for g in order:                                        # filter
        lst = sorted(genes[g], key=lambda t: -len(t.exons))
        keep = []
        for t in lst:
            if t.is_known:
                keep.append(t)
            else:
                j = t.junctions()
                part = any(is_all_include(j, k.junctions(), delta) for k in keep) or \
                    any(is_all_include(j, m.junctions(), delta) for m in model.get(g, []))
                if part:
                    cnt["novel_filtered"] += 1
                    detail[g]["dropped"].append(t.tx)
                else:
                    keep.append(t)
        genes[g] = keep
    key = {"gencode": "gencode", "combination_of_known_junctions": "ckj", "combination_of_known_splicesites": "cks",
           "at_least_one_novel_splicesite": "nss"}
    out = dict.fromkeys(SUFFIXES, "")
    out[".txt"] = LEGEND
    for g in order:                                        # classifier, statistics, exportFiles
        for t in genes[g]:
            if t.is_novel:
                novelty_detector(t, model.get(g, []), delta)
            cnt["isoforms"] += 1
            cnt["evidences"] += len(t.evidence)
            cnt[key[t.subcategorie]] += 1
            cnt[key[t.subcategorie] + "_ev"] += len(t.evidence)
            detail[g]["kept"].append((t.tx, t.subcategorie, len(t.exons)))
            out[".refflat.txt"] += t.print_refflat()
            out[".txt"] += t.print_txt()
            out[".gff"] += t.print_gff()
            if t.is_known:
                out[".final.gff"] += t.print_gff()
                out[".final.refflat.txt"] += t.print_refflat()
    return {k: v.encode("latin-1") for k, v in out.items()}, cnt, detail
