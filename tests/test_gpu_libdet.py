"""Library-format detection on the device (sfgpu_hits_library_kinds, csrc/libdet.hip; lib_format="A" and aux/lib_format_counts.json of
quant.quantify and its doors) against the Python statement hits.library_kinds_host: every counter over the shared corpus
(tests/libdet_corpus.py) under the CPU tests' splits and budgets, the contract's edges and errors, the hit filter as a cross-check of
reads_compatible, and six simulated libraries end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import libdet_corpus as corpus

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def on_device(gpu):
    import torch
    h, o, _, _ = corpus.batch()
    return torch.from_numpy(h.view(np.uint8).reshape(-1).copy()).to(gpu), torch.from_numpy(o.astype(np.int32)).to(gpu)


def _slice(d_hits, d_off, o, a, b):
    """reads [a, b) of the batch where it lies: the records' bytes are not moved (they begin at a multiple of 24 bytes)"""
    return d_hits[int(o[a]) * 24:int(o[b]) * 24], (d_off[a:b + 1] - int(o[a])).contiguous()


@pytest.mark.parametrize("paired", [True, False])
def test_device_equals_the_statement(gpu, on_device, paired):
    """every counter and the rest of the budget, in one call and in calls of 100 reads with remaining_votes and the stats carried, for
    a budget of 0, 1, one that ends inside a block, exactly the voters and more; with and without dovetailing and an expected format"""
    from sailfish_amd import hits as H
    _, o, _, _ = corpus.batch()
    d_hits, d_off = on_device
    for dovetail, fmt in ((False, None), (True, "ISF" if paired else "SR"), (False, "OU" if paired else "U")):
        for budget in corpus.budgets(paired, dovetail):
            want = corpus.expected(paired, dovetail, budget, fmt)
            for calls in corpus.splits():
                rem, st = budget, None
                for a, b in calls:
                    hh, oo = _slice(d_hits, d_off, o, a, b)
                    rem, st = H.library_kinds(hh, oo, paired_library=paired, max_read_occs=corpus.MAX_READ_OCCS, allow_dovetail=dovetail, remaining_votes=rem,
                                              expected=fmt, stats=st)
                assert (rem, st) == want, (dovetail, fmt, budget, len(calls))


@pytest.mark.parametrize("n_reads", [0, 1, 255, 256, 257])
def test_block_edges(gpu, on_device, n_reads):
    """no read at all, and batches that end one read before, at and after a block's last lane; host arrays go in as well"""
    from sailfish_amd import hits as H
    h, o, _, _ = corpus.batch()
    d_hits, d_off = on_device
    hh, oo = corpus.slice_batch(h, o, 0, n_reads)
    want = H.library_kinds_host(hh, oo, paired_library=True, max_read_occs=corpus.MAX_READ_OCCS, remaining_votes=40, expected="IU")
    got = H.library_kinds(*_slice(d_hits, d_off, o, 0, n_reads), paired_library=True, max_read_occs=corpus.MAX_READ_OCCS, remaining_votes=40, expected="IU")
    assert got == want and got[1]["reads"] == n_reads
    assert H.library_kinds(hh, oo, paired_library=True, max_read_occs=corpus.MAX_READ_OCCS, remaining_votes=40, expected="IU", device=gpu) == want


def test_stats_accumulate_and_null_pointers(gpu, on_device):
    """a second call adds to the first's counters; NULL offsets, options, budget or stats, and NULL records where there are records:
    SFGPU_ERR_INVALID, nothing added and the budget untouched; NULL offsets with n_reads == 0 is a valid call"""
    from sailfish_amd import _lib
    from sailfish_amd import hits as H
    d_hits, d_off = on_device
    R = int(d_off.numel()) - 1
    kw = dict(paired_library=True, max_read_occs=corpus.MAX_READ_OCCS, expected="ISF")
    rem, once = H.library_kinds(d_hits, d_off, remaining_votes=100, **kw)
    rem, twice = H.library_kinds(d_hits, d_off, remaining_votes=rem, stats=once, **kw)
    assert rem == 0 and once["votes"] == 100 and twice["votes"] == 100
    for k in ("reads", "reads_mapped", "reads_over_occs", "reads_mixed", "reads_compatible"):
        assert twice[k] == 2 * once[k] > 0
    assert twice["records_kind"] == [2 * v for v in once["records_kind"]] and twice["votes_kind"] == once["votes_kind"]
    L = _lib.lib()
    o = _lib.LibdetOpts(corpus.MAX_READ_OCCS, 1, 0, 0, _lib.LibFmt(0, 0, 0, 0))
    st = _lib.LibdetStats()
    st.reads, st.votes = 7, 7
    st.records_kind[3] = 7
    rem = C.c_int64(55)
    args = [_lib.ptr(d_hits), _lib.ptr(d_off), R, C.byref(o), C.byref(rem), C.byref(st), _lib.current_stream_ptr()]
    for null in (0, 1, 3, 4, 5):
        bad = list(args)
        bad[null] = None
        assert L.sfgpu_hits_library_kinds(*bad) == _lib.ERR_INVALID, null
        assert b"null" in L.sfgpu_last_error()
        assert (st.reads, st.votes, st.records_kind[3], st.reads_mapped, rem.value) == (7, 7, 7, 0, 55), null
    assert L.sfgpu_hits_library_kinds(None, None, 0, C.byref(o), C.byref(rem), C.byref(st), _lib.current_stream_ptr()) == _lib.OK
    assert (st.reads, st.votes, rem.value) == (7, 7, 55)


@pytest.mark.parametrize("dovetail", [False, True])
def test_reads_compatible_is_the_filters_n_mapped(gpu, dovetail):
    """on the part of the corpus that keeps the mapper's contract, for each of the twelve formats: reads_compatible equals n_mapped of
    the hit filter run with enforce_lib_compat and allow_orphans, the same max_read_occs and dovetail setting"""
    from sailfish_amd import hits as H
    h, o = corpus.abiding()
    seen = set()
    for fmt in corpus.FORMATS:
        paired = H.LIBRARY_FORMATS[fmt][0] == 1
        _, st = H.library_kinds(h, o, paired_library=paired, max_read_occs=corpus.MAX_READ_OCCS, allow_dovetail=dovetail, expected=fmt, device=gpu)
        _, _, _, fst = H.filter_hits(h, o, fmt, enforce_lib_compat=True, allow_orphans=True, allow_dovetail=dovetail, max_read_occs=corpus.MAX_READ_OCCS, device=gpu)
        assert st["reads_compatible"] == fst["n_mapped"] > 0, fmt
        assert st == H.library_kinds_host(h, o, paired_library=paired, max_read_occs=corpus.MAX_READ_OCCS, allow_dovetail=dovetail, expected=fmt)[1]
        seen.add(st["reads_compatible"])
    assert len(seen) >= 10


def _sopt(log):
    import sailfish_amd as sf
    return sf.SailfishOpts(jointLog=lambda lvl, msg: log.append((lvl, msg)))


@pytest.mark.parametrize("protocol", corpus.PROTOCOLS)
def test_quantify_reads_detects_the_protocol(gpu, tmp_path, protocol):
    """quantify_reads(..., "A") at batch_reads 64 and 1000: the detected name is the protocol, quant.sf is byte-equal to the run given
    that name, lib_format_counts.json is identical for both batch sizes and equals the writer's text over the statement's counters on
    map_reads of the same reads; the run given the name leaves no counts file"""
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    names, seqs, r1, r2 = corpus.simulated(protocol)
    paired = r2 is not None
    log = []
    texts = []
    for batch_reads in (64, 1000):
        out = tmp_path / f"a{batch_reads}"
        rc, exp = sf.mapper.quantify_reads(names, seqs, r1, r2, "A", str(out), _sopt(log), device=gpu, batch_reads=batch_reads, detect_votes=250)
        assert rc == 0 and exp.lib_format_detected["name"] == exp.lib_format_detected["detected"] == protocol and not exp.lib_format_detected["fallback"]
        texts.append((out / "aux" / "lib_format_counts.json").read_bytes())
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1, r2, protocol, str(tmp_path / "named"), _sopt(log), device=gpu, batch_reads=64)
    assert rc == 0 and not hasattr(exp, "lib_format_detected")
    assert not (tmp_path / "named" / "aux" / "lib_format_counts.json").exists()
    for out in ("a64", "a1000"):
        assert (tmp_path / out / "quant.sf").read_bytes() == (tmp_path / "named" / "quant.sf").read_bytes(), out
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    try:
        h, o = idx.map_reads(r1, r2)
        h, o = h.cpu().numpy().view(H.HIT_DTYPE), o.cpu().numpy().view(np.uint32)
    finally:
        idx.close()
    _, votes = H.library_kinds_host(h, o, paired_library=paired, remaining_votes=250)
    _, counts = H.library_kinds_host(h, o, paired_library=paired, expected=protocol)
    assert votes["votes"] == 250
    want = sf.writer.lib_format_counts_text(protocol, counts, votes=votes, detected=protocol, fallback=False).encode()
    assert texts[0] == texts[1] == want
    assert sum("lib_format A: detected " + protocol in msg for _, msg in log) == 2
    assert sum(msg.startswith("library format " + protocol) for _, msg in log) == 2


def test_quantify_files_and_the_counts_option(gpu, tmp_path):
    """quantify_files("A") from FASTQ names the ISR library; lib_format_counts=True with an explicit (here: wrong) format writes the
    file without any detection, and its ratio shows the mistake"""
    import sailfish_amd as sf
    names, seqs, r1, r2 = corpus.simulated("ISR")
    (tmp_path / "t.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    for path, reads in (("r1.fq", r1), ("r2.fq", r2)):
        (tmp_path / path).write_bytes(b"".join(b"@q%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads)))
    log = []
    run = lambda fmt, out, **kw: sf.mapper.quantify_files(str(tmp_path / "t.fa"), str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq"), fmt, str(tmp_path / out), _sopt(log),
                                                          device=gpu, batch_reads=150, **kw)
    rc, exp = run("A", "auto")
    assert rc == 0 and exp.lib_format_detected["detected"] == "ISR"
    auto = json.loads((tmp_path / "auto" / "aux" / "lib_format_counts.json").read_text())
    assert auto["expected_format"] == auto["detected"] == "ISR" and auto["compatible_fragment_ratio"] > 0.9 and auto["num_reads"] == corpus.SIM_READS
    rc, exp = run("ISF", "wrong", lib_format_counts=True)
    assert rc == 0 and not hasattr(exp, "lib_format_detected")
    wrong = json.loads((tmp_path / "wrong" / "aux" / "lib_format_counts.json").read_text())
    assert wrong["expected_format"] == "ISF" and wrong["detected"] is None and wrong["num_votes"] == 0 and wrong["compatible_fragment_ratio"] < 0.1
    assert wrong["reads"] == auto["reads"] and wrong["num_mapped"] == auto["num_mapped"]


def test_quantify_sam_detects_pairs_on_one_strand(gpu, tmp_path):
    """a SAM file whose pairs lie on one strand -- which the device mapper never makes -- is MSF"""
    import sailfish_amd as sf
    from sailfish_amd import samfile
    rng = np.random.default_rng(3)
    names, ref_len = ["ta", "tb", "tc"], np.array([900, 1200, 700], np.uint32)
    recs = []
    for _ in range(300):
        tid = int(rng.integers(0, 3))
        p = int(rng.integers(0, int(ref_len[tid]) - 300))
        recs.append((tid, p, p + 150, 200, 50, 50, 1, 1, 3, 0))
    hits = np.array(recs, dtype=corpus.HIT_DTYPE)
    off = np.arange(len(recs) + 1, dtype=np.uint32)
    samfile.write_sam(str(tmp_path / "same.sam"), names, ref_len, hits, off)
    log = []
    rc, exp = sf.quant.quantify_sam(str(tmp_path / "same.sam"), "A", str(tmp_path / "out"), _sopt(log), paired=True, device=gpu)
    assert rc == 0 and exp.lib_format_detected["detected"] == "MSF" and exp.lib_format_detected["votes"] == {"MSF": 300}
    counts = json.loads((tmp_path / "out" / "aux" / "lib_format_counts.json").read_text())
    assert counts["expected_format"] == "MSF" and counts["num_compatible"] == counts["num_mapped"] == 300 and counts["strand_mapping_bias"] == 0.0
    with pytest.raises(ValueError, match="paired"):
        sf.quant.quantify_sam(str(tmp_path / "same.sam"), "A", str(tmp_path / "never"), device=gpu)
    assert not (tmp_path / "never").exists()


def test_too_few_votes_fall_back(gpu, tmp_path):
    """ten reads: undetermined, IU stands in, the log carries the level-1 warning, and the files are those of the IU run"""
    import sailfish_amd as sf
    names, seqs, r1, r2 = corpus.simulated("ISF")
    log = []
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1[:10], r2[:10], "A", str(tmp_path / "few"), _sopt(log), device=gpu)
    det = exp.lib_format_detected
    assert rc == 0 and det["name"] == "IU" and det["detected"] is None and det["fallback"] and 0 < det["detail"]["votes"] <= 10
    warnings = [msg for lvl, msg in log if lvl == 1 and msg.startswith("lib_format A: the library format is undetermined")]
    assert len(warnings) == 1 and "falling back to IU" in warnings[0]
    counts = json.loads((tmp_path / "few" / "aux" / "lib_format_counts.json").read_text())
    assert counts["expected_format"] == "IU" and counts["detected"] is None and counts["fallback"] is True and counts["num_reads"] == 10
    rc, _ = sf.mapper.quantify_reads(names, seqs, r1[:10], r2[:10], "IU", str(tmp_path / "iu"), device=gpu)
    assert rc == 0 and (tmp_path / "few" / "quant.sf").read_bytes() == (tmp_path / "iu" / "quant.sf").read_bytes()
    assert sorted(os.listdir(tmp_path / "iu" / "aux")) == sorted(set(os.listdir(tmp_path / "few" / "aux")) - {"lib_format_counts.json"})


def test_value_errors_on_the_device(gpu, tmp_path):
    """"A" without paired_library, "A" with rescue_mates: ValueError before anything is written"""
    import sailfish_amd as sf
    names, seqs, r1, r2 = corpus.simulated("ISF")
    out = tmp_path / "never"
    with pytest.raises(ValueError, match="paired_library"):
        sf.quant.quantify(names, np.array([len(s) for s in seqs], np.uint32), [], "A", str(out), device=gpu)
    with pytest.raises(ValueError, match="rescue_mates"):
        sf.mapper.quantify_reads(names, seqs, r1, r2, "A", str(out), rescue_mates=True, device=gpu)
    assert not out.exists()
