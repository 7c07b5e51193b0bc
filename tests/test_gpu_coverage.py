"""The coverage pass on the device (sfgpu_cov_*, csrc/coverage.hip; coverage.CoverageDevice) against the statement
hits.coverage_host over the shared corpus (tests/coverage_corpus.py): runs, the bits of the summary, counters; the bytes of the
bedGraph file, plain and BGZF, with a 4 KB tile edge on every byte of some row; the contract through the raw entries; and
write_coverage= of mapper.quantify_reads end to end.  Every comparison is equality of integers or bytes."""
import ctypes as C
import gzip
import io

import numpy as np
import pytest

import coverage_corpus as corpus
import rescue_corpus

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _device_result(c):
    tid, start, end, total = (t.cpu().numpy() for t in c.runs())
    summary = tuple(t.cpu().numpy() for t in c.summary())
    return (tid.view(np.uint32), start.view(np.uint32), end.view(np.uint32), total.view(np.uint64)), summary


def _same(c, want):
    (w_runs, w_sum, w_st) = want
    res = c.finish()
    g_runs, g_sum = _device_result(c)
    assert res["residue"] == 0 and res["runs"] == w_st["runs"] and res["bases_covered"] == w_st["bases_covered"] and res["bases_total"] == w_st["bases_total"]
    assert all(np.array_equal(g, w) for g, w in zip(g_runs, w_runs))
    assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(g_sum, w_sum))
    assert c.stats == {k: w_st[k] for k in c.stats}


@pytest.mark.parametrize("mode", corpus.MODES)
def test_device_equals_the_statement(gpu, mode):
    """CoverageDevice over the corpus equals coverage_host in the runs, the bits of the three columns, every counter and residue == 0,
    adding the corpus in 1, 2 and 7 batches"""
    from sailfish_amd import coverage as cov
    want = corpus.expected(mode)
    for k in (1, 2, 7):
        with cov.CoverageDevice(corpus.REF_LEN, gpu) as c:
            for h, o, p, a in corpus.mode_batches(mode, k):
                c.add(h, o, posteriors=p, alignments=a)
            _same(c, want)
            assert c.result["state_bytes"] >= 8 * (int(corpus.REF_LEN.sum()) + 2 * corpus.M + 1)


@pytest.fixture(scope="module")
def finished(gpu):
    from sailfish_amd import coverage as cov
    c = cov.CoverageDevice(corpus.REF_LEN, gpu)
    for h, o, p, a in corpus.mode_batches("posterior", 2):
        c.add(h, o, posteriors=p)
    c.finish()
    yield c
    c.close()


def test_the_text_with_a_tile_edge_on_every_byte_of_a_row(gpu, finished):
    """the device bytes equal coverage_text_host while the first transcript's name grows over 64 consecutive lengths, from 0 bytes
    across the 48 bytes a lane copies: every later row moves byte by byte over the 4 KB tile edges.  chunk_bytes = 8 KB gives more
    than ten chunks; compress=True inflates to the same bytes"""
    from sailfish_amd import coverage as cov
    runs = corpus.expected("posterior")[0]
    for n in range(64):
        names = corpus.names(b"x" * n)
        want = cov.coverage_text_host(names, runs)
        f = io.BytesIO()
        res = finished.write(f, names, chunk_bytes=8192)
        assert f.getvalue() == want, n
        assert res["n_bytes"] == len(want) and res["n_chunks"] > 10 and res["max_row_bytes"] > 5000
        if n % 21 == 0:
            f = io.BytesIO()
            finished.write(f, names)
            assert f.getvalue() == want
            z = io.BytesIO()
            finished.write(z, names, compress=True, chunk_bytes=0 if n else 8192)
            assert z.getvalue()[:4] == b"\x1f\x8b\x08\x04" and gzip.decompress(z.getvalue()) == want


def test_the_summary_file(gpu, finished, tmp_path):
    from sailfish_amd import coverage as cov
    finished.write_summary(str(tmp_path / "s.tsv"), corpus.names())
    want = cov.summary_text_host(corpus.names(), corpus.REF_LEN, corpus.expected("posterior")[1])
    assert (tmp_path / "s.tsv").read_bytes() == want and want.count(b"\n") == corpus.M + 1
    assert b"deep\t65535\t1\t70000\t70000\n" in want


def _raw_add(L, lib, h, hits, off, p=None, stats=None):
    import torch
    dev = torch.device("cuda:0")
    d_h = torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).reshape(-1).copy()).to(dev)
    d_o = torch.from_numpy(np.ascontiguousarray(off, np.uint32).view(np.int32).copy()).to(dev)
    d_p = None if p is None else torch.from_numpy(np.ascontiguousarray(p, np.float64).copy()).to(dev)
    st = lib.CovStats() if stats is None else stats
    rc = L.sfgpu_cov_add(h, lib.ptr(d_h) if len(hits) else None, lib.ptr(d_o), len(off) - 1, lib.ptr(d_p) if d_p is not None else None, None, None, None, C.byref(st), None)
    torch.cuda.synchronize()
    return rc, st


def test_the_contract_through_the_raw_entries(gpu):
    """each error names the lowest offender and leaves state and stats untouched -- the following finish equals the run without the
    bad call; n_reads == 0; the calls out of order; M == 0"""
    import torch
    from sailfish_amd import _lib as lib, coverage as cov, hits as H
    L = lib.lib()
    good = corpus.mode_batches("posterior", 2)
    h, o, p, _ = good[1]
    bad_tid, bad_p = h.copy(), p.copy()
    bad_tid["tid"][[40, 7, 300]] = corpus.M
    bad_p[[90, 33]] = [float("nan"), 1.5]
    c = cov.CoverageDevice(corpus.REF_LEN, gpu)
    res = lib.CovResult()
    assert L.sfgpu_cov_runs(c._h, None, None, None, None) == lib.ERR_STATE and L.sfgpu_cov_summary(c._h, None, None, None) == lib.ERR_STATE
    assert L.sfgpu_cov_write_text(c._h, None, None, 0, lib.TEXT_SINK(0), None, C.byref(res), None) == lib.ERR_STATE
    c.add(*good[0][:3])
    before = dict(c.stats)
    st = lib.CovStats(reads=5)
    rc, st = _raw_add(L, lib, c._h, bad_tid, o, bad_p, st)
    assert rc == lib.ERR_RANGE and b"record 7 " in L.sfgpu_last_error() and st.as_dict() == dict(dict.fromkeys(H.COVERAGE_STATS, 0), reads=5)
    rc, st = _raw_add(L, lib, c._h, h, o, bad_p, st)
    assert rc == lib.ERR_INVALID and b"record 33 " in L.sfgpu_last_error() and st.reads == 5 and st.lines == 0
    rc, st = _raw_add(L, lib, c._h, h[:0], [0], None, st)                      # one entry of offsets, no read
    assert rc == lib.OK and st.reads == 5
    rc, st = _raw_add(L, lib, c._h, h[:0], [0, 0, 0], None, st)                # two reads without records
    assert rc == lib.OK and st.reads == 7 and st.records == 0
    d_o = torch.zeros(3, dtype=torch.int32, device=gpu)
    assert L.sfgpu_cov_add(c._h, None, lib.ptr(d_o), 2, None, lib.ptr(d_o), None, None, C.byref(st), None) == lib.ERR_INVALID      # pos without op_off
    assert L.sfgpu_cov_add(c._h, None, lib.ptr(d_o), 2, None, None, None, None, None, None) == lib.ERR_INVALID                     # no stats
    assert c.stats == before
    c.add(h, o)                                                                 # (uniform weights: the refused p is not read)
    want = H.coverage_host(corpus.REF_LEN, [good[0], (h[:0], [0, 0, 0], None, None), (h, o, None, None)])
    c.stats["reads"] += 2
    _same(c, want)
    rc, _ = _raw_add(L, lib, c._h, h, o)
    assert rc == lib.ERR_INVALID and b"after sfgpu_cov_finish" in L.sfgpu_last_error()
    again = lib.CovResult()
    assert L.sfgpu_cov_finish(c._h, C.byref(again), None) == lib.OK and again.n_runs == want[2]["runs"] and again.residue == 0
    _same(c, want)
    c.close()
    # M == 0: a record is refused, nothing is a valid coverage
    with cov.CoverageDevice(np.zeros(0, np.uint32), gpu) as e:
        rc, _ = _raw_add(L, lib, e._h, h[:1], [0, 1])
        assert rc == lib.ERR_RANGE and b"record 0 " in L.sfgpu_last_error()
        rc, _ = _raw_add(L, lib, e._h, h[:0], [0, 0])
        assert rc == lib.OK
        assert e.finish()["runs"] == 0 and e.result["bases_total"] == 0
        f = io.BytesIO()
        assert e.write(f, [])["n_bytes"] == 0 and f.getvalue() == b""
    # transcripts of no bases only
    with cov.CoverageDevice(np.zeros(3, np.uint32), gpu) as e:
        e.add(h[:0], [0])
        assert e.finish()["runs"] == 0 and [t.tolist() for t in e.summary()] == [[0.0] * 3] * 3


def _statement(idx, r1, r2, batch, weights, **map_kw):
    """coverage_host over the records the device maps batch by batch, under the host statement of the posteriors"""
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    batches = []
    for a in range(0, len(r1), batch):
        h, o = sf.mapper.hits_to_numpy(*idx.map_reads(r1[a:a + batch], r2[a:a + batch], **map_kw))
        aln = None
        if map_kw.get("validate", {}).get("align"):
            pos, _, op_off, ops = (t.cpu().numpy() for t in idx.last_alignments)
            aln = (pos, op_off.view(np.uint64), ops.view(np.uint32))
        batches.append((h, o, None if weights is None else H.posteriors_host(h, o, weights)[0], aln))
    return H.coverage_host(idx.ref_len.cpu().numpy().view(np.uint32), batches)


def test_quantify_reads_writes_the_coverage(gpu, tmp_path):
    """quantify_reads(write_coverage=) on the spliced synthetic transcriptome, 400 pairs in three batches: with uniform and with
    posterior weights, with and without write_mappings, with mappings_gapped, compressed.  The file is coverage_text_host of the
    statement over the batches; quant.sf, aux/ and the mappings file are byte for byte those of the run without the option"""
    import os
    import sailfish_amd as sf
    from sailfish_amd import coverage as cov
    names, seqs, r1, r2, _ = rescue_corpus.end_to_end()
    log = []
    sopt = lambda: sf.SailfishOpts(jointLog=lambda lvl, msg: log.append(msg))      # noqa: E731
    base = dict(batch_reads=150, device=gpu, cmd_options={"libType": "IU"})
    run = lambda tag, **kw: sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / tag), sopt(), **base, **kw)      # noqa: E731

    def same_outputs(tag, plain):
        skip = {"coverage_summary.tsv", "meta_info.json", "cmd_info.json"}
        for d in ("", "aux"):
            a, b = sorted(os.listdir(tmp_path / tag / d)), sorted(os.listdir(tmp_path / plain / d))
            assert [x for x in a if x not in skip] == [x for x in b if x not in skip]
            for x in a:
                if x not in skip and os.path.isfile(tmp_path / tag / d / x):
                    read = gzip.decompress if x.endswith(".gz") else bytes        # (a gzip header carries the time it was written at)
                    assert read((tmp_path / tag / d / x).read_bytes()) == read((tmp_path / plain / d / x).read_bytes()), (tag, d, x)

    rc, exp0 = run("plain", write_mappings=str(tmp_path / "plain.sam"))
    assert rc == 0 and exp0.coverage_stats is None and not [m for m in log if m.startswith("coverage")]
    assert not (tmp_path / "plain" / "aux" / "coverage_summary.tsv").exists()
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)

    def check(tag, exp, want, path, compressed=False):
        got = (tmp_path / path).read_bytes()
        assert (gzip.decompress(got) if compressed else got) == cov.coverage_text_host(names, want[0])
        assert (tmp_path / tag / "aux" / "coverage_summary.tsv").read_bytes() == cov.summary_text_host(names, ref_len, want[1])
        assert {k: exp.coverage_stats[k] for k in want[2]} == want[2] and want[2]["residue"] == 0 and want[2]["runs"] > 100
        assert exp.coverage_stats["state_bytes"] >= 8 * (int(ref_len.sum()) + len(ref_len))

    # uniform weights, no mappings file: one pass
    del log[:]
    rc, exp = run("uni", write_coverage=str(tmp_path / "uni.bedgraph"), coverage_weights="uniform")
    assert rc == 0 and exp.posterior_stats is None
    want_uni = _statement(idx, r1, r2, 150, None)
    check("uni", exp, want_uni, "uni.bedgraph")
    line = [m for m in log if m.startswith("coverage (uniform weights)")]
    assert len(line) == 1 and f"{want_uni[2]['lines']} lines, {want_uni[2]['empty_intervals']} empty intervals; {want_uni[2]['runs']} runs" in line[0]
    same_outputs("uni", "plain")
    # posterior weights, no mappings file: the second pass runs for the coverage alone
    rc, exp = run("post", write_coverage=str(tmp_path / "post.bedgraph"))
    assert rc == 0 and exp.posterior_stats is None
    weights = exp.posterior_weights.cpu().numpy()
    want = _statement(idx, r1, r2, 150, weights)
    check("post", exp, want, "post.bedgraph")
    assert want[0][3].tolist() != want_uni[0][3].tolist()
    same_outputs("post", "plain")
    # ... with the mappings file, written in the first pass as ever; compressed, into a file object
    z = io.BytesIO()
    rc, exp = run("post_sam", write_coverage=z, coverage_compress=True, write_mappings=str(tmp_path / "post.sam"))
    assert rc == 0 and gzip.decompress(z.getvalue()) == cov.coverage_text_host(names, want[0])
    assert (tmp_path / "post.sam").read_bytes() == (tmp_path / "plain.sam").read_bytes()
    same_outputs("post_sam", "plain")
    # ... sharing the second pass with mappings_posteriors
    rc, exp0 = run("zw", write_mappings=str(tmp_path / "zw.sam"), mappings_posteriors=True)
    rc, exp = run("zw_cov", write_mappings=str(tmp_path / "zw_cov.sam"), mappings_posteriors=True, write_coverage=str(tmp_path / "zw.bedgraph"))
    assert rc == 0 and (tmp_path / "zw_cov.sam").read_bytes() == (tmp_path / "zw.sam").read_bytes() and exp.posterior_stats == exp0.posterior_stats
    check("zw_cov", exp, want, "zw.bedgraph")
    same_outputs("zw_cov", "zw")
    # rescue, validation and gapped alignments: the coverage follows the alignments' intervals, with either weight
    opts = dict(rescue_mates=True, validate_mappings=True, max_indel=3, mappings_gapped=True)
    map_kw = dict(validate=dict(min_identity=0.9, keep_best=False, max_indel=3, align=True), rescue=dict(min_identity=0.9, window=sf.SailfishOpts().maxFragLen))
    rc, exp0 = run("gap", write_mappings=str(tmp_path / "gap.sam"), **opts)
    for tag, kw in (("gap_post", {}), ("gap_uni", dict(coverage_weights="uniform")), ("gap_zw", dict(mappings_posteriors=True))):
        rc, exp = run(tag, write_mappings=str(tmp_path / (tag + ".sam")), write_coverage=str(tmp_path / (tag + ".bedgraph")), **opts, **kw)
        assert rc == 0 and exp.align_stats == exp0.align_stats and exp.verify_stats == exp0.verify_stats and exp.rescue_stats == exp0.rescue_stats
        w = None if tag == "gap_uni" else exp.posterior_weights.cpu().numpy()
        check(tag, exp, _statement(idx, r1, r2, 150, w, **map_kw), tag + ".bedgraph")
        if tag != "gap_zw":
            assert (tmp_path / (tag + ".sam")).read_bytes() == (tmp_path / "gap.sam").read_bytes()
        same_outputs(tag, "gap")
    idx.close()


def test_no_coverage_file_where_the_quantification_fails(gpu, tmp_path):
    """Gibbs samples and bootstraps both asked for: quantify returns non-zero, the second pass does not run, no coverage file appears
    and the log says so"""
    import sailfish_amd as sf
    names, seqs, r1, r2, _ = rescue_corpus.end_to_end()
    log = []
    sopt = sf.SailfishOpts(numGibbsSamples=2, numBootstraps=2, jointLog=lambda lvl, msg: log.append(msg))
    path = tmp_path / "never.bedgraph"
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1[:50], r2[:50], "IU", str(tmp_path / "out"), sopt, write_coverage=str(path), device=gpu,
                                       cmd_options={"libType": "IU"})
    assert rc != 0 and exp is None and not path.exists()
    assert [m for m in log if "no coverage file is written" in m]
