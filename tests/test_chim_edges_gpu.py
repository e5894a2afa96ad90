"""K-CHIM on the hand-built edges of tests/chimcases.py (tile seams, scan bounds, the thresholds of the reference's rules, the skip rule and the closure, the
caps and the hand-over between the kernel generations): every read of every batch == the oracle, the six kernel generations agree word for word, and the
counters of smi_chimera_last_counts say which path a read took.  tests/test_chim_cases_cpu.py proves that the cases sit where they claim to."""
import numpy as np
import pytest

import chimcases as cc

CASES = cc.all_cases()
BY_NAME = cc.by_name()
ORDER = {"S": 0, "T": 1, "K": 2, "C": 3, "Cq": 4}
NAMES = [c["name"] for c in sorted(CASES, key=lambda c: ORDER[c["intent"]["family"]])]  # S, T, K, C per read, C per chunk
GENERATIONS = [(), ("SMI_CHIM_A1",), ("SMI_CHIM_V1",), ("SMI_CHIM_GENERIC",), ("SMI_CHIM_NO_PREFILTER",), ("SMI_CHIM_NO_PREFILTER", "SMI_CHIM_V1")]
pytestmark = pytest.mark.gpu


def run(pkg, ctx, seqs, five_prime):
    """the packing and launching of test_chimera_gpu._run: planes pre-filled with garbage -> (results, their words)"""
    import torch

    dev = torch.device("cuda:0")
    n = len(seqs)
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    total = int(offs[-1])
    ra = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    d_reads = torch.from_numpy(ra.copy()).to(dev) if total else torch.zeros(1, dtype=torch.uint8, device=dev)
    d_offs = torch.from_numpy(offs).to(dev)
    d_planes = torch.full((ctx.read_planes_words(total, n),), -1, dtype=torch.int32, device=dev)
    ctx.pack_reads_device(d_reads, d_offs, n, total, d_planes)
    d_out = torch.full((n, 4), -1, dtype=torch.int32, device=dev)
    ctx.chimera_device(d_planes, d_offs, n, total, ctx.chimera_config(five_prime), d_out)
    torch.cuda.synchronize()
    words = d_out.cpu().numpy().copy()
    return words.view(pkg.CHIMERA_RESULT_DTYPE).reshape(-1), words


def assert_equals_oracle(pkg, sor, case, res):
    fp = case["five_prime"]
    for i, s in enumerate(case["reads"]):
        rc, splits, multi, n_matches = cc.expected(sor, s, fp)
        flags = int(res["flags"][i])
        assert not flags & pkg.lib.CHIM_OVERFLOW, (case["name"], i)
        assert bool(flags & pkg.lib.CHIM_RANGE) == (rc != 0), (case["name"], i)
        if rc != 0:
            continue
        got = [(sor.SPLIT_REASONS[res["reason"][i][k]], int(res["pos"][i][k])) for k in range(res["n_split"][i])]
        assert (got, bool(flags & 1), int(res["n_matches"][i])) == (splits, multi, n_matches), (case["name"], i, len(s))


def test_last_counts_before_the_first_call(pkg):
    ctx = pkg.Context(0)
    try:
        with pytest.raises(pkg.lib.SmiError):
            ctx.chimera_last_counts()
    finally:
        ctx.close()


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_oracle_and_took_its_path(pkg, sor, gpu_ctx, monkeypatch, name):
    case = BY_NAME[name]
    fp, it = case["five_prime"], case["intent"]
    for var in {v for g in GENERATIONS for v in g}:
        monkeypatch.delenv(var, raising=False)
    if it.get("cap_switch"):
        monkeypatch.setenv(it["cap_switch"], "1")  # a cap only this generation has
    res, _ = run(pkg, gpu_ctx, case["reads"], fp)
    counts = gpu_ctx.chimera_last_counts()
    assert_equals_oracle(pkg, sor, case, res)
    caps = counts["caps"]
    fam = it["family"]
    if fam in ("S", "T"):
        # the filter did not clear a read with a site by accident
        assert counts["queued"] >= sum(1 for s in set(case["reads"]) if cc.expected(sor, s, fp)[3] > 0), counts
    if fam in ("S", "T", "K"):
        assert not any(caps.values()) and counts["second_chance"] == 0 and counts["serial"] == 0, counts
    if "cap" in it:
        named = {it["cap"]} | ({it["also"]} if "also" in it else set())
        if it["cap"] == "gated_per_read":
            named.add("tso_slot")  # the select kernel hands the read over through the slot's overflow mark
        if not it["over"]:
            assert not any(caps.values()) and counts["second_chance"] == 0 and counts["serial"] == 0, counts
        else:
            assert {k for k, v in caps.items() if v} == named and all(caps[k] == 1 for k in named), counts
            assert counts["second_chance"] == 1, counts
            # the first-generation kernels hold 64 accepted positions and 64 matches: what is over those goes on to the serial kernel
            assert counts["serial"] == (1 if it["cap"] in ("matches_per_read", "accepted_positions") else 0), counts
    if "queue" in it:
        assert caps[it["queue"][0]] > 0 and counts["second_chance"] > 0, counts


@pytest.mark.parametrize("name", [n for n in NAMES if BY_NAME[n]["intent"]["family"] != "Cq"])
def test_generations_agree_word_for_word(pkg, gpu_ctx, monkeypatch, name):
    case = BY_NAME[name]
    first = None
    for gen in GENERATIONS:
        for var in {v for g in GENERATIONS for v in g}:
            monkeypatch.delenv(var, raising=False)
        for var in gen:
            monkeypatch.setenv(var, "1")
        _, words = run(pkg, gpu_ctx, case["reads"], case["five_prime"])
        if first is None:
            first = words
        assert (words == first).all(), (name, gen, np.argwhere(words != first)[:4].tolist())


@pytest.mark.parametrize("five_prime", [False, True])
def test_closure_takes_a_gap_of_31_and_not_of_32(pkg, gpu_ctx, monkeypatch, five_prime):
    """K1: four reads that differ only in the distance d of a gated position over the bound to the exact TSO behind it.  The result cannot tell a closure of
    31 from one of 32 (chimcases' docstring); the number of positions the select kernel queues can: with d <= 31 the decoy is needed, with d >= 32 it is not.
    SMI_CHIM_A1: the generation whose queue has one counter."""
    for var in {v for g in GENERATIONS for v in g}:
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("SMI_CHIM_A1", "1")
    n = {}
    for d in (30, 31, 32, 33):
        case = BY_NAME[("5p_" if five_prime else "3p_") + f"K1_d{d}"]
        run(pkg, gpu_ctx, case["reads"], five_prime)
        n[d] = gpu_ctx.chimera_last_counts()["positions"]
    assert n[30] == n[31] == n[32] + 1 == n[33] + 1, n


@pytest.mark.parametrize("five_prime", [False, True])
def test_chunk_worker_writes_the_oracle_s_fragment_count(pkg, sor, five_prime):
    """the S and T batches as FASTQ text through the native chunk worker (empty reads left out: a FASTQ record has a base)"""
    seqs = []
    for name in NAMES:
        case = BY_NAME[name]
        if case["five_prime"] == five_prime and case["intent"]["family"] in ("S", "T"):
            seqs += [s for s in case["reads"] if s]
    want = sum(len(cc.expected(sor, s, five_prime)[1]) + 1 for s in seqs)
    text = "".join(f"@r{i} x\n{s}\n+\n{'5' * len(s)}\n" for i, s in enumerate(seqs)).encode()
    ctx = pkg.Context(0)
    try:
        ctx.set_barcode_set(np.arange(100, dtype=np.uint64) * 977, mode=0)
        _, _, info = ctx.scanfastq_pass2_chunk(text, five_prime=five_prime)
        assert info["n_records_in"] == len(seqs) and info["n_records_out"] == want
        assert want > len(seqs)
    finally:
        ctx.close()
