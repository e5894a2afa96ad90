"""BamSort's runs in plain Python ("Runs and the merge"): from the record lengths, the reader's segments and
resident_bytes the run every record falls into, and with sortmodel's order and windows the slice every output window draws from every
run file.  Test infrastructure only; it shares nothing with the product."""
import random

import bammodel
import sortcases as sc
import sortmodel as sm

PER_RECORD = 48          # SMI_BAMSORT_PER_RECORD


class SegmentTooLarge(Exception):
    """a segment that does not fit the empty arena: .segment"""

    def __init__(self, segment):
        super().__init__(f"segment {segment}")
        self.segment = segment


def segment_bytes(lengths, seg_counts):
    out, at = [], 0
    for c in seg_counts:
        out.append(sum(lengths[at:at + c]))
        at += c
    assert at == len(lengths)
    return out


def run_of(lengths, seg_counts, resident_bytes):
    """the spill rule: a segment of `bytes` with n records, `taken` records before it (spilled ones included), is taken into the arena
    unless arena_used + bytes + PER_RECORD * (taken + n) > resident_bytes; then what the arena holds becomes a run and the segment goes
    into the empty arena, where the same test refuses it (SegmentTooLarge).  If any run was cut, the last arena-full is a run too.
    -> (the run of every record in input order, the number of runs: 0 where everything fits)"""
    out, run, arena, taken = [], 0, 0, 0
    for k, (c, b) in enumerate(zip(seg_counts, segment_bytes(lengths, seg_counts))):
        if arena + b + PER_RECORD * (taken + c) > resident_bytes:
            if arena == 0 or b + PER_RECORD * (taken + c) > resident_bytes:
                raise SegmentTooLarge(k)
            run, arena = run + 1, 0
        out += [run] * c
        arena, taken = arena + b, taken + c
    return (out, run + 1) if run else ([0] * len(out), 0)


def least_budget(lengths, seg_counts):
    """the least resident_bytes that refuses no segment: every segment fits the empty arena beside the arrays of the records so far"""
    taken, most = 0, 0
    for c, b in zip(seg_counts, segment_bytes(lengths, seg_counts)):
        taken += c
        most = max(most, b + PER_RECORD * taken)
    return most


def merge_plan(keys, lengths, runs, n_runs, window_bytes):
    """keys, lengths, runs: of every record in input order (keys as sortmodel.key gives them).  A run file holds its records in sorted
    order (stable), one behind the other.  -> (windows, slices): sortmodel's windows over the whole file in sorted order, and per window
    one entry per run: (first byte in the run file, bytes, first ordinal, records), where the ordinals number the records run after run
    in each run's sorted order.  The records a window draws from a run are contiguous in the run file (asserted)."""
    n = len(keys)
    order = sorted(range(n), key=lambda i: keys[i])                     # stable: ties in input order, which is run order, then input order
    windows = sm.windows([lengths[i] for i in order], window_bytes)
    at_byte, ordinal, first_ordinal, next_ord = {}, {}, [], 0
    for j in range(n_runs):
        first_ordinal.append(next_ord)
        off = 0
        for i in sorted((i for i in range(n) if runs[i] == j), key=lambda i: keys[i]):
            at_byte[i], ordinal[i] = off, next_ord
            off, next_ord = off + lengths[i], next_ord + 1
    run_size = [sum(lengths[i] for i in range(n) if runs[i] == j) for j in range(n_runs)]
    cursor = [(0, first_ordinal[j]) for j in range(n_runs)]             # where the window before left each run
    slices = []
    for b, e, size in windows:
        per = [[cursor[j][0], 0, cursor[j][1], 0] for j in range(n_runs)]
        for i in (order[r] for r in range(b, e)):
            s = per[runs[i]]
            assert at_byte[i] == s[0] + s[1] and ordinal[i] == s[2] + s[3], "a window's records of one run are contiguous in its file"
            s[1] += lengths[i]
            s[3] += 1
        assert sum(s[1] for s in per) == size
        cursor = [(s[0] + s[1], s[2] + s[3]) for s in per]
        slices.append([tuple(s) for s in per])
    assert [c[0] for c in cursor] == run_size
    return windows, slices


def plan(raw, seg_counts, resident_bytes, window_bytes):
    """a BAM file's bytes -> (runs of the records, n_runs, windows, slices); slices is None where nothing spills"""
    _text, _dict, refs, recs = sm.split(bammodel.bgzf_decompress(raw))
    lengths = [r["length"] for r in recs]
    runs, n_runs = run_of(lengths, seg_counts, resident_bytes)
    if not n_runs:
        return runs, 0, sm.windows([lengths[i] for i in sorted(range(len(recs)), key=lambda i: sm.key(recs[i], len(refs)))], window_bytes), None
    windows, slices = merge_plan([sm.key(r, len(refs)) for r in recs], lengths, runs, n_runs, window_bytes)
    return runs, n_runs, windows, slices


def stage_residues(slices):
    """the residues mod 16 at which the non-empty slices begin in the staging buffer (the slices of a window stand one behind the other)"""
    out = set()
    for per in slices:
        at = 0
        for _first, size, _ord, _n in per:
            if size:
                out.add(at % 16)
            at += size
    return out


def exact_hits(lengths, seg_counts, resident_bytes):
    """the segments taken with the budget exactly full: arena_used + bytes + PER_RECORD * (taken + n) == resident_bytes"""
    hits, arena, taken = [], 0, 0
    for k, (c, b) in enumerate(zip(seg_counts, segment_bytes(lengths, seg_counts))):
        if arena + b + PER_RECORD * (taken + c) > resident_bytes:
            arena = 0
        if arena + b + PER_RECORD * (taken + c) == resident_bytes:
            hits.append(k)
        arena, taken = arena + b, taken + c
    return hits


# ---- inputs of the run tests beside tests/sortcases.py: (the BAM file's bytes, segment_bytes, window_bytes) --------------------------------------
# Every record is longer than a BGZF block and segment_bytes is smaller than a third of one (the seeded characters deflate to about three
# quarters), so the reader hands out one record per segment.
def _long(k, length, pos, rng):
    """a record of exactly `length` bytes on chr1: 36 fixed bytes, the name b<k> with its NUL, one Z attribute of seeded characters"""
    name = f"b{k}"
    pad = length - 36 - len(name) - 1 - 4
    aux = b"XZZ" + bytes(48 + (x & 63) for x in rng.randbytes(pad)) + b"\0"
    r = bammodel.bam_record(name, 16 * rng.randrange(2), 0, pos, 30, [], "", aux=aux)
    assert len(r) == length
    return r


def _one_per_segment(lengths, block, seed):
    rng = random.Random(seed)
    assert min(lengths) > block
    return sc.file_of([("chr1", 1 << 20)], [_long(k, n, rng.randrange(1 << 20), rng) for k, n in enumerate(lengths)], block=block)


def runs_65():
    """150 records of 3,000 bytes and a little more at seeded positions: with the least budget about a hundred runs"""
    return _one_per_segment([3000 + k % 7 for k in range(150)], 2500, 29), 600, 16384


def runs_257():
    """400 records of 8,000 bytes and a little more: with the least budget more than 257 runs"""
    return _one_per_segment([8000 + k % 7 for k in range(400)], 4000, 31), 1000, 65536


LONG_AT = 6


def long_record():
    """sortcases.lengths' record of 70,000 bytes between twelve of 5,000 and more: a segment, a run and a window of its own"""
    return _one_per_segment([5000 + 11 * k for k in range(LONG_AT)] + [70000] + [5100 + 13 * k for k in range(6)], 4000, 37), 1000, 4096


def exact():
    """three records of 5,200, 5,000 and 5,100 bytes, one per segment.  With resident_bytes = 5,000 + 5,100 + 3 * PER_RECORD the second
    does not fit beside the first (a spill) and the third fits beside the second with the budget exactly full; one byte less spills it"""
    return _one_per_segment([5200, 5000, 5100], 4000, 41), 1000, 4096


EXACT_BUDGET = 5000 + 5100 + 3 * PER_RECORD
RUN_CASES = dict(runs_65=runs_65, runs_257=runs_257, long_record=long_record, exact=exact)
