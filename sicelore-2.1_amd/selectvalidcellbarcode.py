"""`SelectValidCellBarcode` (org/ipmc/sicelore/programs/SelectValidCellBarcode.java:L39-92; quickrun-2.1.sh:45, sicelore-nf/main.nf:48):
the cell list that `IsoformMatrix`, `SNPMatrix`, `CollapseModel` and `FusionDetector` take as `CSV=`, from the `BarcodesAssigned.tsv` of
`scanfastq`.

    java -jar Sicelore-2.1.jar SelectValidCellBarcode -I BarcodesAssigned.tsv -O barcodes.csv -MINUMI 1 -ED0ED1RATIO 1

A barcode stays when its reads are at least MINUMI and its ED=0 reads divided by its ED=1 reads (int division) are at least ED0ED1RATIO.
The table has a few thousand rows: the program is host code of the library (smi_select_valid_cells), takes no Context and runs without a
GPU.  A row the reference dies on stops the run with its line number before the output file is touched."""
import sys

from . import lib as _lib


def statistics_lines(total, kept):
    """the two closing messages (SelectValidCellBarcode.java:L89-90), without the logger's prefix"""
    return [f"Total cell barcodes\t\t[{total}]", f"Valid cell barcodes\t\t[{kept}]"]


def select_valid_cell_barcodes(in_tsv, out_csv, min_umi=1, ed0ed1_ratio=1.0, log=sys.stderr):
    """in_tsv -> out_csv, one kept barcode per line in the table's order; the `barcode removed` messages and the two totals go to `log`
    (None: nowhere).  The output is written only after the whole table has been accepted: lib.CellTableError (with .line) leaves an
    existing out_csv as it was.  -> dict(total=data rows, kept=rows written)"""
    with open(in_tsv, "rb") as f:
        tsv = f.read()
    try:
        kept_text, removed_text, total, kept = _lib.select_valid_cells(tsv, min_umi, ed0ed1_ratio)
    except _lib.CellTableError as e:
        raise _lib.CellTableError(f"{in_tsv}: {e}", e.line) from None
    with open(out_csv, "wb") as f:
        f.write(kept_text)
    if log is not None:
        if removed_text:
            log.write(removed_text.decode(errors="replace"))
        for line in statistics_lines(total, kept):
            log.write(line + "\n")
    return dict(total=total, kept=kept)
