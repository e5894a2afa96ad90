"""DeduplicateMolecule in plain Python (DeduplicateMolecule.java:L41-302, Molecule.java:L40-60): the reference's reader,
its name rules, Java's split and Integer, the three folds, the output and the counters, with this build's written-down deviations -- output in
the input order of the winning records, exit instead of a swallowed exception (with the 1-based line), lines end at LF with one CR in front
of it dropped, bytes are bytes.  The yardstick of tests/test_dedup_gpu.py; tests/test_dedup_cpu.py checks it against outputs written by hand."""

FNV_OFFSET, FNV_PRIME = 14695981039346656037, 1099511628211


class DedupError(Exception):
    def __init__(self, line, why):
        super().__init__(f"line {line}: {why}")
        self.line = line


def split_lines(data):
    """-> [(start offset, line bytes)]: lines end at LF; bytes behind the last LF are a line of their own; one CR at the end of a line goes"""
    out, pos = [], 0
    n = len(data)
    while pos < n:
        e = data.find(b"\n", pos)
        if e < 0:
            e = n
        line = data[pos:e]
        if line.endswith(b"\r"):
            line = line[:-1]
        out.append((pos, line))
        pos = e + 1
    return out


def java_split(s, sep=b"-"):
    """String.split(sep) for a one-byte literal separator: trailing empty strings go, a leading one stays; a string without the
    separator comes back whole, the empty one too"""
    if sep not in s:
        return [s]
    parts = s.split(sep)
    while parts and parts[-1] == b"":
        parts.pop()
    return parts


def java_int(b):
    """new Integer(String): an optional sign, decimal digits, a value that fits 32 bits, nothing else -> int or None.  ('-' cannot reach
    it here: the name is split on it.)"""
    digits = b[1:] if b[:1] in (b"+", b"-") else b
    if not digits or any(c not in b"0123456789" for c in digits):
        return None
    v = int(digits)
    if b[:1] == b"-":
        v = -v
    return v if -(1 << 31) <= v < (1 << 31) else None


def normalise(header, marker):
    """L202-203: every marker byte removed, then every literal backslash + '|' -> '-'"""
    return header.replace(marker, b"").replace(b"\\|", b"-")


def fnv1a(key):
    h = FNV_OFFSET
    for c in key:
        h = ((h ^ c) * FNV_PRIME) & ((1 << 64) - 1)
    return h


def read_records(data, fasta=False):
    """the reader (L186-190, L114-116) and the name rules -> (records, counters).  A record: dict(line = 1-based line of its header,
    start / end = its byte span, ids0, ids1, key, rn, seq, qual)."""
    marker = b">" if fasta else b"@"
    need = 2 if fasta else 4
    lines = split_lines(data)
    recs, n_null, skipped = [], 0, 0
    i = 0
    while i < len(lines):
        start, line = lines[i]
        if not line.startswith(marker):
            skipped += 1
            i += 1
            continue
        body = [ln for _p, ln in lines[i + 1:i + need]]
        if len(body) >= 1 and body[0] == b"null":                 # L192 / L118, before anything else of the record is looked at
            n_null += 1
            i += need
            continue
        if len(body) < need - 1:
            raise DedupError(i + 1, "the record is cut short by the end of the input")
        ids = java_split(normalise(line, marker))
        if len(ids) < 3:
            raise DedupError(i + 1, f"{len(ids)} fields in the name, 3 are needed")
        rn = java_int(ids[2])
        if rn is None:
            raise DedupError(i + 1, f"{ids[2]!r} is no integer")
        end = lines[i + need][0] if i + need < len(lines) else len(data)
        recs.append(dict(line=i + 1, start=start, end=end, ids0=ids[0], ids1=ids[1], key=ids[0] + ids[1], rn=rn, seq=body[0],
                         qual=None if fasta else body[2]))
        i += need
    return recs, dict(lines=len(lines), records=len(recs), null_records=n_null, skipped_lines=skipped)


def fold(recs, fasta=False, select=True):
    """-> {key: index of the record that the reference's map holds at the end} (L208-217, L128-136, L285)"""
    held, length = {}, {}
    for i, r in enumerate(recs):
        k = r["key"]
        if k not in held:
            take = True
        elif fasta or select:
            cur = recs[held[k]]
            take = cur["rn"] < r["rn"] or (cur["rn"] == r["rn"] and length[k] < len(r["seq"]))
        else:
            take = False
        if take:
            held[k] = i
            length[k] = 0 if fasta else len(r["seq"])     # the four-argument constructor never sets consensusLength
    return held


def render(r, fasta=False):
    name = r["ids0"] + b"-" + r["ids1"] + b"-" + str(r["rn"]).encode()
    if fasta:
        return b">" + name + b"\n" + r["seq"] + b"\n"
    return b"@" + name + b"\n" + r["seq"] + b"\n+\n" + r["qual"] + b"\n"


def dedup(data, fasta=False, select=True):
    """-> (output bytes, counters)"""
    recs, cnt = read_records(data, fasta)
    held = fold(recs, fasta, select)
    out = b"".join(render(recs[i], fasta) for i in sorted(held.values()))
    return out, dict(cnt, molecules=len(held), bytes_written=len(out))


def group_sizes(data, fasta=False):
    """records per key"""
    sizes = {}
    for r in read_records(data, fasta)[0]:
        sizes[r["key"]] = sizes.get(r["key"], 0) + 1
    return sizes


# ---- the hand-built inputs; what they must give is written out by hand in tests/test_dedup_cpu.py --------------------------------------------
HAND_FASTQ = (
    b"junk in front of the first record\n"
    b"@A-U1-1\nACGT\n+\n@III\n"                      # a quality line that starts with '@'
    b"@A-U1-2\nACGTA\n+some text\nIIIII\n"           # the same molecule with a larger rn; text on the '+' line
    b"stray\n+\n"                                    # junk between records: each line costs itself
    b"@B-U2-3\r\nAC\r\n+\r\nII\r\n"                  # CRLF
    b"@N-U9-5\nnull\n+\nIIII\n"                      # dropped, not counted
    b"@@C@-U3-4\nACG\n+\nII\n"                       # '@' inside the name; quality shorter than the sequence
    b"@D\\|U4\\|5\nA\n+\nI\n"                        # backslash + '|' -> '-'
    b"@E|x-U5-6\nAC\n+\nII\n"                        # a bare '|' stays
    b"@F\\@|U6\\@|7\nACGT\n+\nIIII\n"                # the '@' goes first, then backslash + '|' -> '-'
    b"@-U7-8\nAC\n+\nII\n"                           # a leading empty field
    b"@G-U8-9--\nACG\n+\nIII\n"                      # trailing empty fields
    b"@H-U9-10-extra-more\nACGT\n+\nIIII\n"          # more than three fields
    b"@AB-C-1\nAAA\n+\nIII\n@A-BC-1\nAAAA\n+\nIIII\n"   # one molecule: the key has nothing between its halves
    b"@Z-R0-0\nA\n+\nI\n@Z-R1-007\nA\n+\nI\n@Z-R2-+7\nA\n+\nI\n@Z-R3-2147483647\nA\n+\nI\n"
    b"@T-1-5\nCCC\n+\nIII\n@T-1-5\nGGGGG\n+\nIIIII\n@T-1-5\nTTTTT\n+\nJJJJJ\n@T-1-4\nAAAAAAAAA\n+\nIIIIIIIII\n"
    b"@W-1-2\nAC\n+\nII"                             # no LF at the end of the file
)
HAND_FASTA = (
    b"junk\n"
    b">M-1-3\nAAA\n>M-1-3\nCCC\n>M-1-3\n\n>M-1-2\nGGGG\n"     # equal rn: the last non-empty one
    b">P-1-1\n\n>P-1-1\n\n"                                   # none non-empty behind the first: the first
    b">Q-1-1\nT\n>Q-1-2\n\n>Q-1-1\nTT\n"                      # a larger rn wins with an empty sequence
    b">N-1-1\nnull\n"
    b">>R\\|1\\|4\r\nACGT"                                     # '>' removed everywhere, CRLF, no LF at the end
)
# (input, is FASTA, the 1-based line the run stops on)
ERROR_CASES = {
    "two_fields": (b"@A-U-1\nA\n+\nI\n@A-U\nA\n+\nI\n", False, 5),
    "two_fields_trailing_empty": (b"@A-U--\nA\n+\nI\n", False, 1),
    "rn_empty": (b"junk\n@A-U--x\nA\n+\nI\n", False, 2),
    "rn_blank": (b"@A-U- 7\nA\n+\nI\n", False, 1),
    "rn_too_large": (b"@A-U-1\nA\n+\nI\n\n\n@A-U-2147483648\nA\n+\nI\n", False, 7),
    "rn_sign_only": (b"@A-U-+\nA\n+\nI\n", False, 1),
    "header_on_last_line": (b"@A-U-1\nA\n+\nI\n@B-U-1", False, 5),
    "header_on_last_line_lf": (b"@A-U-1\nA\n+\nI\n@B-U-1\n", False, 5),
    "cut_after_sequence": (b"@A-U-1\nA\n+\nI\n@B-U-1\nAC\n", False, 5),
    "cut_after_plus": (b"@A-U-1\nA\n+\nI\n@B-U-1\nAC\n+", False, 5),
    "smallest_line_wins": (b"@A-U-x\nA\n+\nI\n@A-U\nA\n+\nI\n", False, 1),
    "fasta_two_fields": (b">A-U-1\nA\n>A-U\nA\n", True, 3),
    "fasta_header_on_last_line": (b">A-U-1\nA\nx\n>B-U-1\n", True, 4),
}
