"""The genome coverage on the device (sfgpu_covg_*, csrc/coverage_genome.hip; coverage.GenomeCoverageDevice) against the statement
hits.coverage_genome_host over the shared corpus (tests/covgenome_corpus.py): runs and counters; the bytes of the bedGraph file, plain
and BGZF, with a 4 KB tile edge on every byte of some row; the contract through the raw entries; and write_genome_coverage= of
mapper.quantify_reads end to end on a small spliced genome.  Every comparison is equality of integers or bytes."""
import ctypes as C
import functools
import gzip
import io
import os

import numpy as np
import pytest

import covgenome_corpus as corpus
import rescue_corpus

pytestmark = pytest.mark.gpu
STATS = ("n_pieces", "n_events", "n_keys", "n_runs", "bases_covered", "runs_unplaced", "bases_unplaced", "bases_off_model", "transcripts_placed",
         "transcripts_length_mismatch")


def _device_runs(g):
    chrom, start, end, total = (t.cpu().numpy() for t in g.runs())
    return chrom.view(np.uint32), start.view(np.uint32), end.view(np.uint32), total.view(np.uint64)


@pytest.fixture(scope="module")
def finished(gpu):
    """the corpus' records added through CoverageDevice.add and finished: its runs are corpus.transcript_runs()"""
    from sailfish_amd import coverage as cov
    _, ref_len, _, (h, o, p, _) = corpus.corpus()
    c = cov.CoverageDevice(ref_len, gpu)
    c.add(h, o, posteriors=p)
    c.finish()
    got = tuple(t.cpu().numpy() for t in c.runs())
    assert all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, corpus.transcript_runs()))
    yield c
    c.close()


@pytest.fixture(scope="module")
def projected(gpu, finished):
    g = finished.project(corpus.corpus()[2])
    yield g
    g.close()


def test_device_equals_the_statement(gpu, projected):
    runs, st = corpus.expected()
    assert {k: projected.result[k] for k in STATS} == {k: st[k] for k in STATS}
    assert all(np.array_equal(g, w) for g, w in zip(_device_runs(projected), runs))
    assert projected.result["state_bytes"] >= 40 * st["n_events"] and projected.result["project_ms"] > 0


@pytest.mark.parametrize("what, n_rand, n_long, want", corpus.EDGES)
def test_device_equals_the_statement_at_the_block_edges(gpu, what, n_rand, n_long, want):
    """the edge corpora (tests/covgenome_corpus.py: EDGES): each puts one count that sizes a kernel's grid one below, on or one above a
    multiple of the block -- the events two a piece -- or the long runs around the 4 wavefronts of a block; runs and counters equal the
    statement's"""
    from sailfish_amd import coverage as cov
    runs, st = corpus.edge_expected(what, n_rand, n_long, want)
    _, ref_len, pl, (h, o, p, _) = corpus.corpus(n_rand, n_long)
    with cov.CoverageDevice(ref_len, gpu) as c:
        c.add(h, o, posteriors=p)
        c.finish()
        got = tuple(t.cpu().numpy() for t in c.runs())
        assert all(np.array_equal(g.view(w.dtype), w) for g, w in zip(got, corpus.transcript_runs(n_rand, n_long)))
        with c.project(pl) as g:
            assert {k: g.result[k] for k in STATS} == {k: st[k] for k in STATS}
            assert all(np.array_equal(a, w) for a, w in zip(_device_runs(g), runs))


def test_the_text_with_a_tile_edge_on_every_byte_of_a_row(gpu, projected):
    """the device bytes equal genome_text_host while the first chromosome's name grows over 64 consecutive lengths, across the 48 bytes
    a lane copies: every later row moves byte by byte over the 4 KB tile edges.  compress=True inflates to the same bytes"""
    from sailfish_amd import coverage as cov
    runs = corpus.expected()[0]
    for n in range(64):
        names = [b"c" * n] + corpus.CHROM_NAMES[1:]
        want = cov.genome_text_host(names, runs)
        f = io.BytesIO()
        res = projected.write(f, names, chunk_bytes=8192)
        assert f.getvalue() == want, n
        assert res["n_bytes"] == len(want) and res["n_chunks"] > 2 and res["max_row_bytes"] > 5000
        if n % 21 == 0:
            z = io.BytesIO()
            projected.write(z, names, compress=True, chunk_bytes=0 if n else 8192)
            assert z.getvalue()[:4] == b"\x1f\x8b\x08\x04" and gzip.decompress(z.getvalue()) == want
    f = io.BytesIO()
    projected.write(f, corpus.CHROM_NAMES)
    assert f.getvalue() == cov.genome_text_host(corpus.CHROM_NAMES, runs)
    with pytest.raises(ValueError, match="names for 4 chromosomes"):
        projected.write(io.BytesIO(), corpus.CHROM_NAMES[:3])


def _edit(a, at, v):
    return np.concatenate([a[:at], [v], a[at + 1:]]).astype(a.dtype)


def test_the_contract_through_the_raw_entries(gpu, finished):
    """project before finish and with another M; a bad model refused by open with the lowest transcript named; an event count at the cap
    refused with the handle unchanged and a following legal call correct; runs and write before project"""
    from sailfish_amd import _lib as lib, coverage as cov
    L = lib.lib()
    names, ref_len, pl, (h, o, p, _) = corpus.corpus()
    runs, st = corpus.expected()
    res = lib.CovgResult()
    # a model that is refused: the lowest offending transcript is named
    lo, hi = corpus.tid("plus3"), corpus.tid("iso_a")
    e = lambda t: int(pl.exon_off[t])                      # noqa: E731
    for change, t in ((dict(chrom=_edit(_edit(pl.chrom, hi, 4), lo, 4)), lo), (dict(strand=_edit(pl.strand, hi, 0)), hi),
                      (dict(exon_start=_edit(pl.exon_start, e(lo) + 1, 1005)), lo), (dict(exon_len=_edit(pl.exon_len, e(hi), 0)), hi),
                      (dict(exon_start=_edit(pl.exon_start, e(hi) + 1, 4294967200)), hi), (dict(strand=_edit(pl.strand, lo, -1)), lo),
                      (dict(exon_off=_edit(_edit(pl.exon_off, hi, e(hi) + 3), lo + 1, e(lo) - 1)), lo), (dict(exon_off=_edit(pl.exon_off, 0, 1)), 0)):
        with pytest.raises(lib.SfgpuError, match=rf"transcript {t}\b") as err:
            cov.GenomeCoverageDevice(finished, pl._replace(**change))
        assert err.value.code == lib.ERR_INVALID
    # the calls out of order
    with cov.CoverageDevice(ref_len, gpu) as c:
        c.add(h, o, posteriors=p)
        with cov.GenomeCoverageDevice(finished, pl) as g:
            assert L.sfgpu_covg_project(g._h, c._h, C.byref(res), None) == lib.ERR_STATE and b"before sfgpu_cov_finish" in L.sfgpu_last_error()
    with cov.CoverageDevice(ref_len[:-1], gpu) as c, cov.GenomeCoverageDevice(finished, pl) as g:
        c.finish()
        assert L.sfgpu_covg_project(g._h, c._h, C.byref(res), None) == lib.ERR_INVALID and b"transcripts" in L.sfgpu_last_error()
        assert all(np.array_equal(a, w) for a, w in zip(_device_runs(g), runs))          # the handle keeps what it had
    # the cap: exactly n_events is refused, one more is not
    with pytest.raises(lib.SfgpuError, match=rf"{st['n_events']} events") as err:
        cov.GenomeCoverageDevice(finished, pl, _event_cap=st["n_events"])
    assert err.value.code == lib.ERR_RANGE
    with cov.GenomeCoverageDevice(finished, pl, _event_cap=st["n_events"] + 1) as g:
        assert g.result["n_events"] == st["n_events"]
        assert L.sfgpu_covg_event_cap(g._h, 100) == lib.OK
        assert L.sfgpu_covg_project(g._h, finished._h, C.byref(res), None) == lib.ERR_RANGE
        assert all(np.array_equal(a, w) for a, w in zip(_device_runs(g), runs))          # nothing changed
        f = io.BytesIO()
        g.write(f, corpus.CHROM_NAMES)
        assert f.getvalue() == cov.genome_text_host(corpus.CHROM_NAMES, runs)
        assert L.sfgpu_covg_event_cap(g._h, 0) == lib.OK
        assert g.project(finished)["n_runs"] == st["n_runs"] and all(np.array_equal(a, w) for a, w in zip(_device_runs(g), runs))
    # nothing to project: no transcripts, and transcripts without a run
    empty = corpus.Placement(*(a[:0] for a in pl[:3]), pl.exon_off[:1], pl.exon_start[:0], pl.exon_len[:0], 0, [])
    with cov.CoverageDevice(np.zeros(0, np.uint32), gpu) as c, c.project(empty) as g:
        f = io.BytesIO()
        assert g.result["n_runs"] == 0 and g.result["n_events"] == 0 and g.write(f, [])["n_bytes"] == 0 and f.getvalue() == b""
    with cov.CoverageDevice(ref_len, gpu) as c, c.project(pl) as g:
        assert g.result["n_runs"] == 0 and g.result["transcripts_placed"] == st["transcripts_placed"] and [len(t) for t in g.runs()] == [0] * 4


@functools.lru_cache(maxsize=None)
def _genome():
    """three chromosomes, six genes of three isoforms on both strands, exons of 40 to 120 bases; 300 pairs of 2 x 40
    -> (names, transcripts, mate 1, mate 2, the GTF's bytes)"""
    rng = np.random.default_rng(439)
    chroms = {b"chrB": rescue_corpus.rand(rng, 3000), b"chrA": rescue_corpus.rand(rng, 2500), b"chr10": rescue_corpus.rand(rng, 2500)}
    names, seqs, gtf = [], [], [b"# a spliced genome\n"]
    for gi, (c, strand, at) in enumerate(((b"chrB", b"+", 100), (b"chrB", b"-", 1500), (b"chrA", b"+", 50), (b"chrA", b"-", 1200), (b"chr10", b"+", 200),
                                          (b"chr10", b"-", 1000))):
        exons = []
        for _ in range(5):
            n = int(rng.integers(40, 121))
            exons.append((at, n))
            at += n + int(rng.integers(30, 90))
        for ii, keep in enumerate(((0, 1, 2, 3, 4), (0, 2, 4), (1, 2, 3))):
            name = b"g%d.i%d" % (gi, ii)
            s = b"".join(chroms[c][exons[k][0]:exons[k][0] + exons[k][1]] for k in keep)
            names.append(name.decode()); seqs.append(s if strand == b"+" else rescue_corpus.revcomp(s))
            gtf.append(b'%s\ttest\ttranscript\t%d\t%d\t.\t%s\t.\tgene_id "g%d"; transcript_id "%s";\n' % (c, exons[keep[0]][0] + 1, at, strand, gi, name))
            for k in keep[::-1] if ii == 1 else keep:      # (the file's order of a transcript's exons does not matter)
                gtf.append(b'%s\ttest\texon\t%d\t%d\t.\t%s\t.\tgene_id "g%d"; transcript_id "%s";\n' % (c, exons[k][0] + 1, exons[k][0] + exons[k][1], strand, gi, name))
    r1, r2, _ = rescue_corpus.fragments(rng, seqs, 300, 40, frag_mean=130, frag_sd=15)
    return names, seqs, r1, r2, b"".join(gtf)


def _statement(idx, r1, r2, batch, weights):
    """coverage_host over the records the device maps batch by batch, under the host statement of the posteriors"""
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    batches = []
    for a in range(0, len(r1), batch):
        h, o = sf.mapper.hits_to_numpy(*idx.map_reads(r1[a:a + batch], r2[a:a + batch]))
        batches.append((h, o, None if weights is None else H.posteriors_host(h, o, weights)[0], None))
    return H.coverage_host(idx.ref_len.cpu().numpy().view(np.uint32), batches)


def test_quantify_reads_writes_the_genome_coverage(gpu, tmp_path):
    """quantify_reads(write_genome_coverage=, coverage_annotation=) on the spliced genome, 300 pairs in three batches, with posterior
    and with uniform weights: the genome file is genome_text_host(coverage_genome_host(...)) of the statement's transcript runs;
    quant.sf, aux/, the transcript coverage file and the mappings file are byte for byte those of the run without the two keywords;
    with write_genome_coverage alone no transcript file appears"""
    import sailfish_amd as sf
    from sailfish_amd import coverage as cov, genes, hits as H
    names, seqs, r1, r2, gtf_bytes = _genome()
    gtf = tmp_path / "genome.gtf"
    gtf.write_bytes(gtf_bytes)
    log = []
    sopt = lambda: sf.SailfishOpts(jointLog=lambda lvl, msg: log.append((lvl, msg)))      # noqa: E731
    base = dict(batch_reads=100, device=gpu, cmd_options={"libType": "IU"})
    run = lambda tag, **kw: sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / tag), sopt(), **base, **kw)      # noqa: E731

    def same_outputs(tag, plain):
        skip = {"meta_info.json", "cmd_info.json"}
        for d in ("", "aux"):
            a, b = sorted(os.listdir(tmp_path / tag / d)), sorted(os.listdir(tmp_path / plain / d))
            assert a == b
            for x in a:
                if x not in skip and os.path.isfile(tmp_path / tag / d / x):
                    read = gzip.decompress if x.endswith(".gz") else bytes        # (a gzip header carries the time it was written at)
                    assert read((tmp_path / tag / d / x).read_bytes()) == read((tmp_path / plain / d / x).read_bytes()), (tag, d, x)

    model = genes.ExonModel.from_gtf(str(gtf))
    placement = model.for_names(names)
    assert model.chrom_names == [b"chr10", b"chrA", b"chrB"] and placement.status.tolist() == [0] * 18
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)
    for weights in ("posterior", "uniform"):
        kw = dict(coverage_weights=weights)
        rc, exp0 = run("plain_" + weights, write_coverage=str(tmp_path / f"plain_{weights}.bg"), write_mappings=str(tmp_path / f"plain_{weights}.sam"), **kw)
        assert rc == 0 and exp0.genome_coverage_stats is None
        del log[:]
        rc, exp = run("both_" + weights, write_coverage=str(tmp_path / f"both_{weights}.bg"), write_mappings=str(tmp_path / f"both_{weights}.sam"),
                      write_genome_coverage=str(tmp_path / f"both_{weights}.genome.bg"), coverage_annotation=str(gtf), **kw)
        assert rc == 0
        w = exp.posterior_weights.cpu().numpy() if weights == "posterior" else None
        t_runs = _statement(idx, r1, r2, 100, w)[0]
        g_runs, st = H.coverage_genome_host(t_runs, placement, ref_len)
        want = cov.genome_text_host(placement.chrom_names, g_runs)
        assert (tmp_path / f"both_{weights}.genome.bg").read_bytes() == want and st["n_runs"] > 100 and st["transcripts_length_mismatch"] == 0
        assert {k: exp.genome_coverage_stats[k] for k in STATS} == {k: st[k] for k in STATS}
        assert exp.genome_coverage_stats["bytes"] == len(want) and exp.genome_coverage_stats["transcripts"] == 18
        line = [m for lvl, m in log if m.startswith("genome coverage:")]
        assert len(line) == 1 and f"18 of 18 transcripts placed; {st['n_pieces']} pieces, {st['n_events']} events; {st['n_runs']} runs" in line[0]
        assert not [m for lvl, m in log if lvl == 1 and "write_genome_coverage" in m]
        for ext in ("bg", "sam"):
            assert (tmp_path / f"both_{weights}.{ext}").read_bytes() == (tmp_path / f"plain_{weights}.{ext}").read_bytes()
        assert (tmp_path / f"both_{weights}.bg").read_bytes() == cov.coverage_text_host(names, t_runs)
        same_outputs("both_" + weights, "plain_" + weights)
        # the genome file alone, compressed, into a file object: no transcript file, the summary all the same
        z = io.BytesIO()
        rc, exp = run("alone_" + weights, write_genome_coverage=z, coverage_annotation=str(gtf), coverage_compress=True, **kw)
        assert rc == 0 and gzip.decompress(z.getvalue()) == want and exp.coverage_stats["bytes"] == 0
        assert (tmp_path / ("alone_" + weights) / "aux" / "coverage_summary.tsv").read_bytes() == (tmp_path / ("both_" + weights) / "aux" / "coverage_summary.tsv").read_bytes()
        assert not [x for x in os.listdir(tmp_path) if x.startswith("alone_") and os.path.isfile(tmp_path / x)]
    # an annotation that knows other names: nothing is placed, every run is dropped, the log warns
    other = tmp_path / "other.gtf"
    other.write_bytes(gtf_bytes.replace(b'transcript_id "g', b'transcript_id "G'))
    del log[:]
    rc, exp = run("none", write_genome_coverage=str(tmp_path / "none.bg"), coverage_annotation=str(other), coverage_weights="uniform")
    assert rc == 0 and (tmp_path / "none.bg").read_bytes() == b"" and exp.genome_coverage_stats["transcripts_placed"] == 0
    assert exp.genome_coverage_stats["runs_unplaced"] == exp.coverage_stats["runs"] and [m for lvl, m in log if lvl == 1 and "places none of the 18" in m]
    idx.close()


def test_no_genome_file_where_the_quantification_fails(gpu, tmp_path):
    """Gibbs samples and bootstraps both asked for: quantify returns non-zero, the second pass does not run, neither file appears and
    the log says so for each"""
    import sailfish_amd as sf
    names, seqs, r1, r2, gtf_bytes = _genome()
    gtf = tmp_path / "genome.gtf"
    gtf.write_bytes(gtf_bytes)
    log = []
    sopt = sf.SailfishOpts(numGibbsSamples=2, numBootstraps=2, jointLog=lambda lvl, msg: log.append(msg))
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1[:50], r2[:50], "IU", str(tmp_path / "out"), sopt, write_coverage=str(tmp_path / "t.bg"),
                                       write_genome_coverage=str(tmp_path / "g.bg"), coverage_annotation=str(gtf), device=gpu, cmd_options={"libType": "IU"})
    assert rc != 0 and exp is None and not (tmp_path / "t.bg").exists() and not (tmp_path / "g.bg").exists()
    assert [m for m in log if "no coverage file is written" in m] and [m for m in log if "no genome coverage file is written" in m]
