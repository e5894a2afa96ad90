"""K-UPARSE (k_umi_parse of smi_umi_stage.hip) at its edges: every chunk of tests/uparsecases.py through smi_assignumis_chunk with the UMI stage
on the device, held record by record to tests/uparsemodel.py (the reference-pinned name parser, window, CIGAR walk and region grouping, the
oracle's K-UMI matrices and clusterer) and to the host path -- and held to having STAYED on the device (smi_assignumis_last_path): a parser
that handed every chunk to the host path would otherwise pass any comparison with it.  tests/test_uparse_cases_cpu.py shows that the chunks
hold the edges they are named for."""
import numpy as np
import pytest

import uparsecases as uc
import uparsemodel as um

pytestmark = pytest.mark.gpu
FIELDS = ("region", "center", "u1", "u2", "flags", "u8", "u7")


def _run(ctx, case, monkeypatch, host=False, **extra):
    names, flags, pos0, cigars, kw = case
    if host:
        monkeypatch.setenv("SMI_AU_HOST", "1")
    else:
        monkeypatch.delenv("SMI_AU_HOST", raising=False)
    try:
        tags, n_done = ctx.assignumis_chunk(names, flags, pos0, cigars, **{**kw, **extra})
    finally:
        monkeypatch.delenv("SMI_AU_HOST", raising=False)
    return tags.copy(), n_done, ctx.assignumis_last_path()


def _hold_to_model(names, got, n_done, exp, exp_done):
    assert n_done == exp_done
    for i, (nm, t) in enumerate(zip(names, exp)):
        g = got[i]
        have = dict(region=int(g["region"]), center=int(g["center"]), u1=int(g["u1"]), u2=int(g["u2"]), flags=int(g["flags"]), u8=g["u8"].decode(),
                    u7=g["u7"].decode())
        for f in FIELDS:
            assert have[f] == t[f], f"record {i} {nm}: {f} is {have[f]!r}, the model says {t[f]!r}"
    assert not got["reserved"].any()


def _hold_to_floors(cid, names, got):
    from sicelore_amd import lib as libmod

    need = um.least(cid)
    have = dict(window=int((got["flags"] & libmod.UMI_HAS_U7 != 0).sum()), region=int((got["region"] >= 0).sum()),
                clustered=int((got["flags"] & libmod.UMI_CLUSTERED != 0).sum()), long=um.long_names(names, uc.NAME_STAGE))
    print(cid, "exercised", have, "of at least", need)
    assert all(have[k] >= need[k] for k in have), (cid, have, need)


@pytest.mark.parametrize("cid", list(uc.CASES))
def test_device_stage_equals_model_and_stays_on_the_device(pkg, sor, gpu_ctx, monkeypatch, cid):
    from sicelore_amd import lib as libmod

    case = uc.case(cid)
    exp, exp_done, _ = um.expected(sor, cid, case)
    got, n_done, path = _run(gpu_ctx, case, monkeypatch)
    assert path == libmod.AU_PATH_DEVICE == 1, f"{cid}: the chunk left the device stage (path {path})"
    _hold_to_model(case[0], got, n_done, exp, exp_done)
    _hold_to_floors(cid, case[0], got)
    host, host_done, host_path = _run(gpu_ctx, case, monkeypatch, host=True)
    assert host_path == libmod.AU_PATH_HOST_FORCED == 2
    assert host_done == n_done and host.tobytes() == got.tobytes()


@pytest.mark.parametrize("which", [k for k, _, kind in uc.FALLBACKS if kind == "model"])
def test_names_the_kernel_does_not_evaluate_hand_the_chunk_to_the_host_path(pkg, sor, gpu_ctx, monkeypatch, which):
    """one odd name among 70: path 3, the host path's answer, and the model's (Integer.parseInt and float32 read the name)"""
    from sicelore_amd import lib as libmod

    case = uc.fallback_cases(which)
    got, n_done, path = _run(gpu_ctx, case, monkeypatch)
    assert path == libmod.AU_PATH_HOST_NAMES == 3
    host, host_done, host_path = _run(gpu_ctx, case, monkeypatch, host=True)
    assert host_path == 2 and host_done == n_done and host.tobytes() == got.tobytes()
    exp, exp_done, _ = um.expected(sor, "fallback-" + which, case)
    _hold_to_model(case[0], got, n_done, exp, exp_done)
    assert int((got["flags"] & libmod.UMI_CLUSTERED != 0).sum()) >= 30


@pytest.mark.parametrize("which", [k for k, _, kind in uc.FALLBACKS if kind == "error"])
def test_names_without_an_adapter_end_fail_on_both_paths(pkg, gpu_ctx, monkeypatch, which):
    from sicelore_amd import lib as libmod

    case = uc.fallback_cases(which)
    with pytest.raises(pkg.SmiError, match="AE="):
        _run(gpu_ctx, case, monkeypatch)
    assert gpu_ctx.assignumis_last_path() == libmod.AU_PATH_HOST_NAMES
    with pytest.raises(pkg.SmiError, match="AE="):
        _run(gpu_ctx, case, monkeypatch, host=True)
    assert gpu_ctx.assignumis_last_path() == libmod.AU_PATH_HOST_FORCED


def test_keep_data_end_on_a_partial_wave(pkg, sor, gpu_ctx, monkeypatch):
    """129 records (two waves and one record), more of the chromosome to follow: the records from n_done on carry no region and no flags"""
    case = uc.tail_cases(129, keep_data_end=True)
    exp, exp_done, _ = um.expected(sor, "tail-129-keep", case)
    got, n_done, path = _run(gpu_ctx, case, monkeypatch)
    assert path == 1 and 0 < n_done < 129
    _hold_to_model(case[0], got, n_done, exp, exp_done)
    assert (got["region"][n_done:] == -1).all() and not got["flags"][n_done:].any() and got["flags"][:n_done].any()
    host, host_done, host_path = _run(gpu_ctx, case, monkeypatch, host=True)
    assert host_path == 2 and host_done == n_done and host.tobytes() == got.tobytes()


@pytest.mark.parametrize("five", [False, True])
def test_random_umi_windows_in_a_wave_staged_row_by_row(pkg, sor, gpu_ctx, monkeypatch, five):
    """assignumis -f on the chunk of three waves whose middle one is not flat: U7 follows (seed, record index) there too"""
    case = uc.long_name_cases("b", five, seed=11)
    names = case[0]
    exp, exp_done, recs = um.expected(sor, f"long-b-seed11-{five}", case)
    got, n_done, path = _run(gpu_ctx, case, monkeypatch)
    assert path == 1
    _hold_to_model(names, got, n_done, exp, exp_done)
    dec = {0: "A", 1: "G", 2: "C", 3: "T"}
    n_in_block = 0
    for i, r in enumerate(recs):
        if r["window"] is None:
            assert got["u7"][i] == b""
            continue
        z = um.splitmix(11, i)
        assert got["u7"][i].decode() == "".join(dec[(z >> (2 * k)) & 3] for k in range(1, 13)), (i, names[i])
        n_in_block += 64 <= i < 128
    assert n_in_block >= 50
    host, host_done, host_path = _run(gpu_ctx, case, monkeypatch, host=True)
    assert host_path == 2 and host_done == n_done and host.tobytes() == got.tobytes()


def test_a_lane_keeps_its_own_path(pkg, gpu_ctx, monkeypatch):
    from sicelore_amd import lib as libmod

    lane = gpu_ctx.lane()
    try:
        assert lane.assignumis_last_path() == libmod.AU_PATH_NONE == 0
        _run(gpu_ctx, uc.case("tail-65"), monkeypatch, host=True)
        assert gpu_ctx.assignumis_last_path() == 2 and lane.assignumis_last_path() == 0
        got, n_done, path = _run(lane, uc.case("tail-65"), monkeypatch)
        assert path == 1 and gpu_ctx.assignumis_last_path() == 2
        again, again_done, _ = _run(gpu_ctx, uc.case("tail-65"), monkeypatch)
        assert again_done == n_done and again.tobytes() == got.tobytes()
    finally:
        lane.close()


def test_odd_names_as_the_reference_reads_them(pkg, sor, gpu_ctx, monkeypatch):
    """tests/golden/ref_exec_umi_odd_names.json (FastqRecordExt.getScanDatFromReadName executed from the reference's class files on names with
    one odd field), each name inside the ordinary chunk of 70, on both paths: a name the reference parsed gives the model's tags (and
    tests/test_uparse_cases_cpu.py holds the model's fields to the reference's); an AE= the reference refuses fails the chunk; a PS= / ed= /
    bcEnd= it refuses counts as absent here (the reference throws NumberFormatException there too: the product's reading, not the reference's)"""
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_exec_umi_odd_names.json")) as f:
        sec = [s for s in json.load(f)["sections"] if not s["five_prime"]][0]
    n_parsed = n_error = n_absent = n_device = 0
    for k, c in enumerate(sec["cases"]):
        nm = c["name"]
        if "_Q=abc" in nm:
            continue                                     # (Float.parseFloat throws; strtof reads 0: not settled here)
        case = uc.fallback_cases(None, name=nm)
        fails = "throws" in c and ("AdapterInfoNotFound" in c["throws"] or "_AE=743_" not in nm)
        if fails:
            for host in (False, True):
                with pytest.raises(pkg.SmiError, match="AE="):
                    _run(gpu_ctx, case, monkeypatch, host=host)
            n_error += 1
            continue
        exp, exp_done, _ = um.expected(sor, f"odd-{k}", case)
        got, n_done, path = _run(gpu_ctx, case, monkeypatch)
        assert path == (1 if uc.evaluated_on_device(nm) else 3), nm
        _hold_to_model(case[0], got, n_done, exp, exp_done)
        host, host_done, _ = _run(gpu_ctx, case, monkeypatch, host=True)
        assert host_done == n_done and host.tobytes() == got.tobytes(), nm
        n_parsed += "throws" not in c
        n_absent += "throws" in c
        n_device += path == 1
    assert n_parsed >= 20 and n_error >= 8 and n_absent >= 8 and n_device >= 8
