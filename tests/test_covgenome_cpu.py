"""The genome coverage without a GPU: the Python statement hits.coverage_genome_host against a dense per-base restatement written here
and against the invariant of the weighted bases; csrc/covgfmt.h alone (tests/covgenome_harness.cpp, g++ -Wall -Wextra -Werror) against
the statement in the runs, the counters and the bytes of the text; the named cases of the corpus worked by hand; genes.ExonModel on
written GTF text; and the options' ValueErrors.  Every comparison is equality of integers or bytes."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import covgenome_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "covgenome_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p
STATS = ("n_pieces", "n_events", "n_keys", "n_runs", "bases_covered", "runs_unplaced", "bases_unplaced", "bases_off_model", "transcripts_placed",
         "transcripts_length_mismatch")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("covgh")), "libcovgenome_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.cgh_check.restype = C.c_int64
    L.cgh_check.argtypes = [_P] * 6 + [C.c_uint64, C.c_uint32]
    L.cgh_project.restype = _P
    L.cgh_project.argtypes = [_P] * 7 + [C.c_uint64] + [_P] * 4 + [C.c_uint64]
    L.cgh_close.argtypes = [_P]
    L.cgh_stats.argtypes = [_P, _P]
    L.cgh_runs.argtypes = [_P] * 5
    L.cgh_text.restype = C.c_uint64
    L.cgh_text.argtypes = [_P] * 4
    return L


def _model_arrays(pl):
    return (np.ascontiguousarray(pl.status, np.uint8), np.ascontiguousarray(pl.chrom, np.int32), np.ascontiguousarray(pl.strand, np.int8),
            np.ascontiguousarray(pl.exon_off, np.uint64), np.ascontiguousarray(np.concatenate([pl.exon_start, [0]]), np.uint32),
            np.ascontiguousarray(np.concatenate([pl.exon_len, [0]]), np.uint32))


def _ptr(a):
    return a.ctypes.data


def _harness_result(L, pl, ref_len, t_runs, names):
    model = _model_arrays(pl)
    runs = [np.ascontiguousarray(np.concatenate([x, [0]]), dt) for x, dt in zip(t_runs, (np.uint32, np.uint32, np.uint32, np.uint64))]
    h = L.cgh_project(*(_ptr(a) for a in model), _ptr(np.ascontiguousarray(np.concatenate([ref_len, [0]]), np.uint32)), len(pl.status), *(_ptr(a) for a in runs),
                      len(t_runs[0]))
    try:
        st = np.zeros(10, np.uint64)
        L.cgh_stats(h, _ptr(st))
        n = int(st[3])
        out = np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n + 1, np.uint64)
        L.cgh_runs(h, *(_ptr(a) for a in out))
        blob = np.frombuffer(b"".join(names) + b"\0", np.uint8).copy()
        off = np.zeros(len(names) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in names])
        size = L.cgh_text(h, _ptr(blob), _ptr(off), None)
        text = np.zeros(size + 1, np.uint8)
        assert L.cgh_text(h, _ptr(blob), _ptr(off), _ptr(text)) == size
        return tuple(a[:n] for a in out), dict(zip(STATS, st.tolist())), text[:size].tobytes()
    finally:
        L.cgh_close(h)


def _dense(t_runs, pl):
    """every covered transcript base mapped to its genome base one at a time, the values summed in Python integers (a dict over the
    covered bases, so the block at 4 000 000 000 can stay where it is) and run-length encoded -> (runs, dropped weight)"""
    eo = pl.exon_off.tolist()
    depth, dropped = {}, 0
    for t, a, b, s in zip(*(x.tolist() for x in t_runs)):
        where = []                                         # the genome base of every transcript base, block by block
        for e in range(eo[t], eo[t + 1]):
            gs, n = int(pl.exon_start[e]), int(pl.exon_len[e])
            where += list(range(gs, gs + n)) if pl.strand[t] > 0 else list(range(gs + n - 1, gs - 1, -1))
        for x in range(a, b):
            if pl.status[t] != 0 or x >= len(where):
                dropped += s
                continue
            key = (int(pl.chrom[t]), where[x])
            depth[key] = depth.get(key, 0) + s
    out = []
    for (c, g), s in sorted(depth.items()):
        if out and out[-1][0] == c and out[-1][2] == g and out[-1][3] == s:
            out[-1][2] = g + 1
        else:
            out.append([c, g, g + 1, s])
    return [tuple(r) for r in out], dropped


def _rows(runs):
    return list(zip(*(x.tolist() for x in runs)))


@pytest.mark.parametrize("big", [False, True])
def test_statement_equals_the_dense_restatement(built, big):
    _, _, pl, _ = corpus.corpus()
    t_runs = corpus.big_runs() if big else corpus.transcript_runs()
    runs, st = corpus.expected(big)
    dense, _ = _dense(t_runs, pl)
    assert _rows(runs) == dense
    assert st["n_runs"] == len(dense) and st["bases_covered"] == sum(r[2] - r[1] for r in dense)
    assert all(s < 1 << 64 for _, _, _, s in dense)
    if big:
        assert max(r[3] for r in dense) == ((1 << 32) - 2) << 32          # past 2^63, below 2^64: nothing wrapped


@pytest.mark.parametrize("big", [False, True])
def test_weighted_bases_are_kept(built, big):
    """sum (end - start) sum over the genome runs = the same over the transcript runs minus the dropped bases', in Python integers"""
    _, _, pl, _ = corpus.corpus()
    t_runs = corpus.big_runs() if big else corpus.transcript_runs()
    runs, st = corpus.expected(big)
    _, dropped = _dense(t_runs, pl)
    weight = lambda rr: sum((b - a) * s for _, a, b, s in _rows(rr))      # noqa: E731
    assert weight(runs) == weight(t_runs) - dropped
    assert dropped > 0 and st["bases_unplaced"] > 0 and st["bases_off_model"] > 0


@pytest.mark.parametrize("what, n_rand, n_long, want", corpus.EDGES)
def test_edge_corpora_fall_on_the_block_edges(built, harness, what, n_rand, n_long, want):
    """every edge corpus has the count it is listed with (edge_expected asserts it), one below, on or one above a multiple of the
    block; the serial C++ gives the statement's runs on it"""
    assert (want % corpus.BLOCK in (corpus.BLOCK - 1, 0, 1) and want > corpus.BLOCK) or (what == "long_runs" and want in (3, 4, 5))
    runs, st = corpus.edge_expected(what, n_rand, n_long, want)
    assert st["n_events"] == 2 * st["n_pieces"]
    _, ref_len, pl, _ = corpus.corpus(n_rand, n_long)
    g_runs, g_st, _ = _harness_result(harness, pl, ref_len, corpus.transcript_runs(n_rand, n_long), corpus.CHROM_NAMES)
    assert all(np.array_equal(g, w) for g, w in zip(g_runs, runs)) and g_st == {k: st[k] for k in STATS}


def test_named_cases(built):
    """the rows the corpus' named transcripts must give, worked by hand"""
    rows = set(_rows(corpus.expected()[0]))
    h = 1 << 31
    want = [(0, 105, 115, h), (0, 130, 150, h // 2), (0, 200, 210, h // 4),
            (0, 1005, 1010, h), (0, 1020, 1030, h), (0, 1040, 1045, h),
            (0, 2005, 2010, h), (0, 2020, 2030, h), (0, 2040, 2045, h),                               # minus3: [5, 25) read from the far end
            (0, 4294967294, 4294967295, h), (1, 0, 10, h),                                            # edge_hi and single: two rows
            (1, 200, 201, 3 * h // 2), (1, 204, 205, 3 * h // 2),                                     # onebase
            (0, 5010, 5020, h), (0, 5020, 5060, h + h // 2), (0, 5060, 5080, h // 2),                 # the isoforms' shared exon
            (0, 6000, 6100, h),                                                                       # touching, equal: one row
            (0, 6200, 6250, h), (0, 6250, 6300, h // 2),                                              # touching, unequal: two
            (0, 6400, 6450, h), (0, 6450, 6480, h + h // 4), (0, 6480, 6500, h),                      # -s +s +w on 6450
            (0, 7005, 7015, h),                                                                       # an intron of 0 bases
            (1, corpus.FAR + 10, corpus.FAR + 60, h), (1, corpus.FAR + 100, corpus.FAR + 130, h),     # beyond 2^31
            (2, 10, 30, h),
            (0, 8020, 8030, h),                                                                       # short_model: [20, 40) cut at L = 30
            (0, 8100, 8150, h)]
    for row in want:
        assert row in rows, row
    assert sum(1 for r in rows if r[0] == 1 and 1000 <= r[1] < 1600) == 300                           # wave300: a row per 1-base block
    assert not any(r[0] == 3 for r in rows)                                                           # chrE: no row
    st = corpus.expected()[1]
    assert st["runs_unplaced"] == 4 and st["bases_unplaced"] == 10 + 20 + 30 + 40
    assert st["transcripts_placed"] == len(corpus.corpus()[0]) - 4


def test_harness_equals_the_statement(built, harness):
    from sailfish_amd import coverage as cov
    names, ref_len, pl, _ = corpus.corpus()
    model = _model_arrays(pl)
    assert harness.cgh_check(*(_ptr(a) for a in model), len(names), pl.n_chrom) == -1
    for big in (False, True):
        t_runs = corpus.big_runs() if big else corpus.transcript_runs()
        runs, st = corpus.expected(big)
        g_runs, g_st, g_text = _harness_result(harness, pl, ref_len, t_runs, corpus.CHROM_NAMES)
        assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(g_runs, runs))
        assert g_st == {k: st[k] for k in STATS}
        assert g_text == cov.genome_text_host(corpus.CHROM_NAMES, runs)


def test_harness_check_names_the_lowest_bad_transcript(built, harness):
    names, _, pl, _ = corpus.corpus()
    lo, hi = corpus.tid("plus3"), corpus.tid("iso_a")

    def check(**change):
        arrays = list(_model_arrays(pl._replace(**change)))
        return harness.cgh_check(*(_ptr(a) for a in arrays), len(names), pl.n_chrom)

    e = lambda t: int(pl.exon_off[t])                      # noqa: E731
    edit = lambda a, at, v: np.concatenate([a[:at], [v], a[at + 1:]]).astype(a.dtype)      # noqa: E731
    assert check(chrom=edit(edit(pl.chrom, hi, 4), lo, 4)) == lo                      # chromosome >= n_chrom, twice: the lowest
    assert check(strand=edit(pl.strand, hi, 0)) == hi
    assert check(exon_start=edit(pl.exon_start, e(lo) + 1, 1005)) == lo               # overlaps block 0 on +
    assert check(exon_len=edit(pl.exon_len, e(hi), 0)) == hi                          # an empty block
    assert check(exon_start=edit(pl.exon_start, e(hi) + 1, 4294967200)) == hi         # beyond 2^32 - 1
    assert check(strand=edit(pl.strand, lo, -1)) == lo                                # ascending blocks on -
    assert check(exon_off=edit(pl.exon_off, hi, e(hi) + 5)) in (hi - 1, hi)           # the offsets decrease behind it


GTF = (b'#comment line\n'
       b'chrB\tsrc\texon\t101\t150\t.\t+\t.\tgene_id "g1"; transcript_id "tB";\r\n'
       b'chrB\tsrc\texon\t1\t50\t.\t+\t.\tgene_id "g1"; transcript_id "tB";\n'
       b'chrB\tsrc\tExon\t201\t250\t.\t+\t.\tgene_id "g1"; transcript_id "tB";\n'
       b'chrB\tsrc\texons\t201\t250\t.\t+\t.\tgene_id "g1"; transcript_id "tB";\n'
       b'chrB\tsrc\ttranscript\t1\t150\t.\t+\t.\tgene_id "g1"; transcript_id "tB";\n'
       b'chrB\tsrc\texon\t1\t50\n'
       b'chrA\tsrc\texon\t11\t20\t.\t-\t.\tgene_id "g2"; transcript_id tMinus;\n'
       b'chrA\tsrc\texon\t21\t30\t.\t-\t.\ttranscript_id tMinus\n'
       b'chrA\tsrc\texon\t1\t5\t.\t-\t.\tgene_id "g2"; transcript_id "t2chrom";\n'
       b'chrB\tsrc\texon\t1\t5\t.\t-\t.\tgene_id "g2"; transcript_id "t2chrom";\n'
       b'chrA\tsrc\texon\t1\t5\t.\t-\t.\tgene_id "g2"; transcript_id "t2strand";\n'
       b'chrA\tsrc\texon\t7\t9\t.\t+\t.\tgene_id "g2"; transcript_id "t2strand";\n'
       b'chrA\tsrc\texon\t1\t5\t.\t.\t.\tgene_id "g2"; transcript_id "tDot";\n'
       b'chrA\tsrc\texon\t1\t5\t.\t+\t.\tgene_id "g2"; transcript_id "tOver";\n'
       b'chrA\tsrc\texon\t5\t9\t.\t+\t.\tgene_id "g2"; transcript_id "tOver";\n'
       b'chrA\tsrc\texon\t1\t5\t.\t+\t.\tgene_id "g2"; transcript_id "tDup";\n'
       b'chrA\tsrc\texon\t1\t5\t.\t+\t.\tgene_id "g2"; transcript_id "tDup";\n'
       b'chrA\tsrc\texon\t1\t5\t.\t+\t.\tgene_id "g2";\n'
       b'chr10\tsrc\texon\t4294967295\t4294967295\t.\t+\t.\ttranscript_id "tEnd"')      # no final newline


def test_exon_model_from_gtf(built, tmp_path):
    from sailfish_amd import genes
    path = tmp_path / "a.gtf"
    path.write_bytes(GTF)
    gz = tmp_path / "a.gtf.gz"
    with gzip.open(gz, "wb") as f:
        f.write(GTF)
    for p in (path, gz):
        m = genes.ExonModel.from_gtf(str(p))
        assert m.chrom_names == [b"chr10", b"chrA", b"chrB"]                          # bytewise: "1" < "A"
        assert m.transcripts[b"tB"] == (0, 2, 1, [(0, 50), (100, 50)])                # sorted by start; Exon / exons / transcript are no exons
        assert m.transcripts[b"tMinus"] == (0, 1, -1, [(20, 10), (10, 10)])           # unquoted id; touching exons; reversed on -
        assert m.transcripts[b"t2chrom"][0] == 2 and m.transcripts[b"t2strand"][0] == 2
        assert m.transcripts[b"tDot"][0] == 3
        assert m.transcripts[b"tOver"][0] == 4 and m.transcripts[b"tDup"][0] == 4
        assert m.transcripts[b"tEnd"] == (0, 0, 1, [(4294967294, 1)])
        assert len(m.transcripts) == 8
    pl = m.for_names(["tMinus", b"nobody", "tDot", b"tB"])
    assert pl.status.tolist() == [0, 1, 3, 0] and pl.chrom.tolist() == [1, -1, -1, 2] and pl.strand.tolist() == [-1, 0, 0, 1]
    assert pl.exon_off.tolist() == [0, 2, 2, 2, 4] and pl.exon_start.tolist() == [20, 10, 0, 100] and pl.exon_len.tolist() == [10, 10, 50, 50]
    assert (pl.status.dtype, pl.chrom.dtype, pl.strand.dtype, pl.exon_off.dtype, pl.exon_start.dtype, pl.exon_len.dtype) == (
        np.uint8, np.int32, np.int8, np.int64, np.uint32, np.uint32)
    assert pl.n_chrom == 3 and set(genes.EXON_STATUS) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("line, what", [(b'chrA\ts\texon\t0\t5\t.\t+\t.\ttranscript_id "t";', "start"),
                                        (b'chrA\ts\texon\t6\t5\t.\t+\t.\ttranscript_id "t";', "start"),
                                        (b'chrA\ts\texon\t1\t4294967296\t.\t+\t.\ttranscript_id "t";', "4294967295"),
                                        (b'chrA\ts\texon\t1\t5x\t.\t+\t.\ttranscript_id "t";', "decimal"),
                                        (b'chrA\ts\texon\t-1\t5\t.\t+\t.\ttranscript_id "t";', "decimal"),
                                        (b'chrA\ts\texon\t\t5\t.\t+\t.\ttranscript_id "t";', "decimal"),
                                        (b'\ts\texon\t1\t5\t.\t+\t.\ttranscript_id "t";', "chromosome")])
def test_exon_model_errors_name_the_line(built, tmp_path, line, what):
    from sailfish_amd import genes
    path = tmp_path / "bad.gtf"
    path.write_bytes(b"# one\nchrA\ts\texon\t1\t5\t.\t+\t.\ttranscript_id \"ok\";\r\n" + line + b"\n")
    with pytest.raises(ValueError, match=r"line 3\b.*" + what):
        genes.ExonModel.from_gtf(str(path))


def test_option_errors_come_before_the_index(built, tmp_path, monkeypatch):
    from sailfish_amd import mapper
    monkeypatch.setattr(mapper, "QuasiIndex", lambda *a, **k: pytest.fail("an index was built"))
    gtf = tmp_path / "a.gtf"
    gtf.write_bytes(GTF)
    call = lambda **kw: mapper.quantify_reads(["t"], ["ACGT" * 20], ["ACGT" * 10], None, "U", str(tmp_path / "out"), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="come together"):
        call(write_genome_coverage=str(tmp_path / "g.bg"))
    with pytest.raises(ValueError, match="come together"):
        call(coverage_annotation=str(gtf))
    with pytest.raises(ValueError, match="write_genome_coverage: one path"):
        call(write_genome_coverage=7, coverage_annotation=str(gtf))
    with pytest.raises(ValueError, match="needs write_coverage or write_genome_coverage"):
        call(coverage_compress=True)
    bad = tmp_path / "bad.gtf"
    bad.write_bytes(b'chrA\ts\texon\t9\t5\t.\t+\t.\ttranscript_id "t";\n')
    with pytest.raises(ValueError, match="line 1"):                                   # the annotation is read before the index is built
        call(write_genome_coverage=str(tmp_path / "g.bg"), coverage_annotation=str(bad))
    with pytest.raises(ValueError, match="come together"):
        mapper.quantify_files("t.fa", "r.fq", None, "U", str(tmp_path / "out"), write_genome_coverage=str(tmp_path / "g.bg"))
