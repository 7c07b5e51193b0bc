"""The genome alignments without a GPU: csrc/galnfmt.h alone (tests/galn_harness.cpp, g++ -Wall -Wextra -Werror) against the Python
statement hits.project_alignments_host in every array and counter, on the corpus and on every edge corpus; the named cases worked
by hand; the host writers (samfile._sam_text, write_bam(sort="coordinate"), build_bai, fetch) over the projected batch; an independent
cross-check against the genome coverage; genes.ExonModel.chrom_lengths; and the options' ValueErrors.  Every comparison is equality of
integers or bytes."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import galn_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "galn_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p
N_STATS = 13


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("gah")), "libgaln_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.gah_project.restype = _P
    L.gah_project.argtypes = [_P] * 6 + [C.c_uint64, _P, _P, C.c_uint32] + [_P] * 8
    L.gah_close.argtypes = [_P]
    L.gah_sizes.argtypes = [_P, _P]
    L.gah_arrays.argtypes = [_P] * 11
    L.gah_md_reverse.argtypes = [_P, C.c_uint64, _P]
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data


def _pad(a, dt):
    return np.ascontiguousarray(np.concatenate([np.asarray(a, dt), np.zeros(1, dt)]), dt)


def _harness_result(L, pl, hits, offsets, alignments, tags):
    from sailfish_amd import hits as H
    model = (_pad(pl.status, np.uint8), _pad(pl.chrom, np.int32), _pad(pl.strand, np.int8), np.ascontiguousarray(pl.exon_off, np.uint64),
             _pad(pl.exon_start, np.uint32), _pad(pl.exon_len, np.uint32))
    h, o = _pad(hits, corpus.HIT_DTYPE), np.ascontiguousarray(offsets, np.uint32)
    a = [None] * 4 if alignments is None else [_pad(alignments[0], np.int32), np.ascontiguousarray(alignments[2], np.uint64), _pad(alignments[3], np.uint32),
                                               _pad(alignments[1], np.uint32)]
    t = [None] * 3 if tags is None else [_pad(tags[0], np.uint32), np.ascontiguousarray(tags[1], np.uint64), _pad(tags[2], np.uint8)]
    bad = C.c_int64(0)
    g = L.gah_project(*(_ptr(x) for x in model), len(pl.status), _ptr(h), _ptr(o), len(o) - 1, *(_ptr(x) for x in a), *(_ptr(x) for x in t), C.byref(bad))
    if not g:
        return int(bad.value)
    try:
        sz = np.zeros(N_STATS + 3, np.uint64)
        L.gah_sizes(g, _ptr(sz))
        n, n_ops, n_md = (int(x) for x in sz[N_STATS:])
        out = (np.zeros(n + 1, corpus.HIT_DTYPE), np.zeros(len(o), np.uint32), np.zeros(2 * n + 1, np.int32), np.zeros(2 * n + 1, np.uint32),
               np.zeros(2 * n + 1, np.uint64), np.zeros(n_ops + 1, np.uint32), np.zeros(2 * n + 1, np.uint32), np.zeros(2 * n + 1, np.uint64),
               np.zeros(n_md + 1, np.uint8), np.zeros(n + 1, np.uint32))
        L.gah_arrays(g, *(_ptr(x) for x in out))
        return (out[0][:n], out[1], (out[2][:2 * n], out[3][:2 * n], out[4], out[5][:n_ops]), (out[6][:2 * n], out[7], out[8][:n_md]), out[9][:n],
                dict(zip(H.GENOME_ALN_STATS, sz[:N_STATS].tolist())))
    finally:
        L.gah_close(g)


def same_result(got, want, tagged=True):
    """two results of the projection agree in every array and counter"""
    assert got[0].tobytes() == np.ascontiguousarray(want[0], corpus.HIT_DTYPE).tobytes()
    assert np.array_equal(got[1], want[1])
    for g, w in zip(got[2], want[2]):
        assert np.array_equal(np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64))
    if tagged:
        for g, w in zip(got[3], want[3]):
            assert np.array_equal(np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64))
    assert np.array_equal(got[4], want[4])
    assert {k: got[5][k] for k in want[5]} == want[5]


@pytest.mark.parametrize("which", ["gapped", "untagged", "ungapped"])
def test_serial_equals_the_statement(built, harness, which):
    pl = corpus.model()[1]
    b = corpus.ungapped() if which == "ungapped" else corpus.gapped()
    got = _harness_result(harness, pl, b["hits"], b["offsets"], b.get("alignments"), b.get("tags") if which == "gapped" else None)
    same_result(got, corpus.expected(which), tagged=which == "gapped")


@pytest.mark.parametrize("what, delta", corpus.EDGES)
def test_serial_equals_the_statement_at_the_block_edges(built, harness, what, delta):
    b, want = corpus.edge(what, delta)
    same_result(_harness_result(harness, corpus.model()[1], b["hits"], b["offsets"], b["alignments"], b["tags"]), want)


def test_a_record_that_names_no_transcript(built, harness):
    from sailfish_amd import hits as H
    b, pl = corpus.ungapped(), corpus.model()[1]
    hits = b["hits"].copy()
    hits["tid"][[9, 4, 12]] = len(pl.status)
    assert _harness_result(harness, pl, hits, b["offsets"], None, None) == 4
    with pytest.raises(ValueError, match="record 4 names transcript"):
        H.project_alignments_host(hits, b["offsets"], pl)


def _lines(res):
    """the kept lines of a result by source record: {(old record, which): (tid, pos, cigar, md, fwd, mate_fwd)}"""
    h, _, (pos, _, op_off, ops), tags, src, _ = res
    out = {}
    for j, i in enumerate(src.tolist()):
        for w in range(2 if h[j]["mate_status"] == 3 else 1):
            s = 2 * j + w
            md = tags[2][int(tags[1][s]):int(tags[1][s + 1])].tobytes() if tags is not None else None
            out[(i, w)] = (int(h[j]["tid"]), int(pos[s]), corpus.cigar(ops[int(op_off[s]):int(op_off[s + 1])]), md, int(h[j]["fwd"]), int(h[j]["mate_fwd"]))
    return out


def test_the_named_cases_by_hand(built):
    """the corpus' first reads hold one record each, in the order of its docstring"""
    res = corpus.expected("gapped")
    got = _lines(res)
    want = {0: (0, 105, "10M", b"10"), 1: (0, 1005, "5M10N5M", b"10"), 2: (0, 2025, "5M10N5M", b"10"), 3: (0, 1005, "5M10N5M", b"10"), 4: (0, 2025, "5M10N5M", b"10"),
            5: (0, 1000, "10M", b"10"), 6: (0, 2040, "10M", b"10"), 7: (0, 1002, "6M2D10N2D6M", b"6^ACGT6"), 8: (0, 2022, "6M2D10N2D6M", b"6^ACGT6"),
            9: (0, 1002, "6M2D10N6M", b"6^AC6"), 10: (0, 2024, "6M10N2D6M", b"6^GT6"), 11: (0, 1002, "8M10N2D6M", b"8^AC6"), 12: (0, 2022, "6M2D10N8M", b"6^GT8"),
            13: (0, 1005, "5M3I10N5M", b"10"), 14: (0, 2025, "5M10N3I5M", b"10"), 15: (0, 2028, "2S2M10N10M3S", b"12"), 16: (0, 1000, "3S10M10N2M2S", b"12"),
            17: (1, 200, "1M1N1M1N1M1N1M", b"4"), 18: (0, 7005, "10M", b"10"),
            19: (2, 30093, "100M", b"100"), 20: (2, 30093, "100M", b"99T0"), 21: (2, 30176, "17M", b"5G0T10"), 22: (2, 30091, "50M2D50M", b"50^GT50"),
            23: (2, 30182, "4M2D5M", b"3A0^GT5"), 24: (2, 31007, "100M", b"100"), 25: (2, 31007, "100M", b"0A99"), 26: (2, 31007, "17M", b"10A0C5"),
            27: (2, 31007, "50M2D50M", b"50^AC50"), 28: (2, 31007, "5M2D4M", b"5^AC0T3")}
    for i, w in want.items():
        assert got[(i, 0)][:4] == w, i
    b = corpus.gapped()
    assert got[(2, 0)][4] == 1 and b["hits"][2]["fwd"] == 0 and got[(1, 0)][4] == 1                # fwd is inverted on -, kept on +
    # the drops, in the statement's order of tests; the reads that lose records
    h, off, _, _, src, st = res
    assert not {29, 30, 31, 32, 33, 34, 35, 36, 39} & set(src.tolist())
    assert (st["records_unplaced"], st["records_unalignable"], st["records_off_range"]) == (5, 3, 3)
    r = [k for k in range(len(b["offsets"]) - 1) if b["offsets"][k] == 34][0]                        # the read of st1 + st2, then st3 + inside, then three
    assert [int(off[k + 1] - off[k]) for k in (r, r + 1, r + 2)] == [0, 1, 2] and src[off[r + 1]:off[r + 3]].tolist() == [37, 38, 40]
    # the pairs: mates in different blocks, TLEN spanning the intron; on - pos > mate_pos
    pairs = {int(i): h[j] for j, i in enumerate(src.tolist()) if h[j]["mate_status"] == 3 and i in (41, 42, 43)}
    assert (pairs[41]["pos"], pairs[41]["mate_pos"], pairs[41]["frag_len"], pairs[41]["fwd"], pairs[41]["mate_fwd"]) == (10005, 10110, 135, 1, 0)
    assert (pairs[42]["pos"], pairs[42]["mate_pos"], pairs[42]["frag_len"], pairs[42]["fwd"], pairs[42]["mate_fwd"]) == (11115, 11010, 135, 0, 1)
    assert (pairs[43]["pos"], pairs[43]["mate_pos"], pairs[43]["frag_len"]) == (10040, 10000, 120) and got[(43, 0)][2] == "10M50N20M" and got[(43, 1)][2] == "2S20M"
    assert 44 not in src.tolist() and 45 not in src.tolist()                                        # a pair falls as a whole


def test_the_ungapped_cases_by_hand(built):
    res = corpus.expected("ungapped")
    got, st = _lines(res), res[5]
    HI = corpus.HI
    want = {0: (0, 100, "3S7M"), 1: (0, 2023, "7M10N10M3S"), 2: (0, 1005, "5M10N5M"), 3: (0, 2025, "5M10N5M"), 4: (1, 200, "1M1N1M1N1M1N1M"), 5: (0, 7005, "10M"),
            6: (0, 8020, "20M"), 7: (0, 8035, "5M"), 8: (0, 0, "10M"), 10: (0, 0, "5M"), 11: (0, HI - 10, "10M")}
    for i, w in want.items():
        assert got[(i, 0)][:3] == w, i
    for i in (9, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22):
        assert (i, 0) not in got, i
    assert got[(5, 0)][4] == 0 and got[(1, 0)][4] == 1 and got[(3, 0)][4] == 0
    assert (st["records_unplaced"], st["records_unalignable"]) == (5, 3) and st["records_off_range"] >= 4 and st["columns_beyond_model"] >= 10 + 5 + 5 + 5
    assert st["words_out"] - st["words_in"] >= st["n_operations"]


@pytest.mark.parametrize("md", [b"100", b"0A99", b"10A0C5", b"50^AC50", b"5^AC0T3", b"", b"0", b"0N0^NRY0a12"])
def test_md_reverse(built, harness, md):
    from sailfish_amd import hits as H
    want = H.md_reverse(md)
    out = np.zeros(len(md) + 1, np.uint8)
    harness.gah_md_reverse(_ptr(np.frombuffer(md + b"\0", np.uint8).copy()), len(md), _ptr(out))
    assert out[:len(md)].tobytes() == want and len(want) == len(md) and H.md_reverse(want) == md
    assert {b"100": b"100", b"0A99": b"99T0", b"10A0C5": b"5G0T10", b"50^AC50": b"50^GT50", b"5^AC0T3": b"3A0^GT5"}.get(md, want) == want


def _projected_text(which="gapped", posteriors=True):
    from sailfish_amd import samfile
    b = corpus.gapped()
    h, off, aln, tags, src, _ = corpus.expected(which)
    p = ((np.arange(len(b["hits"])) % 7 + 1) / 8.0)[src]
    return samfile._sam_text(corpus.CHROM_NAMES, corpus.CHROM_LENGTHS, h, off, None, b["seqs"], oriented=True, alignments=aln, tags=tags if which == "gapped" else None,
                             posteriors=(p,) if posteriors else None), (h, off, aln, tags, src)


def test_the_host_writers_take_the_projected_batch(built, tmp_path):
    """_sam_text writes the spliced lines; the sorted BAM and its index are built, and fetch inside an intron returns exactly the
    records that span it"""
    from sailfish_amd import samfile
    text, (h, off, aln, tags, src) = _projected_text()
    lines = [ln.split(b"\t") for ln in text.split(b"\n") if ln and not ln.startswith(b"@")]
    assert text.startswith(b"@HD") and b"@SQ\tSN:chr1\tLN:2147483647\n" in text
    first = {ln[0]: ln for ln in reversed(lines)}
    assert first[b"r1"][1:6] == [b"73", b"chr1", b"1006", b"255", b"5M10N5M"] and first[b"r1"][-3:] == [b"MD:Z:10", b"NH:i:1", b"ZW:f:0.25"]
    assert first[b"r2"][1:6] == [b"73", b"chr1", b"2026", b"255", b"5M10N5M"]          # fwd 0 on a - transcript: forward on the genome
    assert first[b"r6"][1] == b"89" and first[b"r23"][5] == b"4M2D5M" and b"MD:Z:3A0^GT5" in first[b"r23"]
    lost = [ln for ln in lines if ln[0] == b"r34"]
    assert [ln[1] for ln in lost] == [b"77", b"141"]                                   # the read that lost both records
    path = str(tmp_path / "genome.bam")
    b = corpus.gapped()
    p = ((np.arange(len(b["hits"])) % 7 + 1) / 8.0)[src]
    samfile.write_bam(path, corpus.CHROM_NAMES, corpus.CHROM_LENGTHS, h, off, seqs=b["seqs"], oriented=True, sort="coordinate", alignments=aln, tags=tags, posteriors=(p,))
    bai = samfile.build_bai(path)
    got = samfile.fetch(path, "chr1", 1012, 1015, bai=bai)                             # inside j_plus' first intron [1010, 1020)
    spans = []
    for j in range(len(h)):
        for w in range(2 if h[j]["mate_status"] == 3 else 1):
            s = 2 * j + w
            span = corpus.ref_len([int(x) for x in aln[3][int(aln[2][s]):int(aln[2][s + 1])]])
            if h[j]["tid"] == 0 and aln[0][s] < 1015 and aln[0][s] + span > 1012:
                spans.append(s)
    assert len(got) == len(spans) >= 8
    for rec in got:                                                                   # every one of them is spliced over the region: it holds an N
        l_name, n_ops = rec[12], struct.unpack_from("<H", rec, 16)[0]
        ops = struct.unpack_from("<%dI" % n_ops, rec, 36 + l_name)
        assert any(op & 15 == 3 for op in ops)


def test_the_pile_of_the_projected_lines_is_the_genome_coverage(built):
    """Independent of the walk: the records the projection keeps and that have no column beyond the model, piled per genomic base over
    the M / = / X columns of their projected CIGARs with weight trunc(p 2^32), give the genome coverage that coverage_genome_host makes
    of coverage_host's transcript runs of the same records and alignments"""
    from sailfish_amd import hits as H
    names, pl = corpus.model()
    L = np.array([int(pl.exon_len[int(pl.exon_off[t]):int(pl.exon_off[t + 1])].sum()) for t in range(len(names))], np.int64)
    for which in ("gapped", "ungapped"):
        b = corpus.gapped() if which == "gapped" else corpus.ungapped()
        hits, aln = b["hits"], b.get("alignments")
        src = corpus.expected(which)[4].tolist()
        take = []
        for i in src:                                      # kept, and every line ends within the blocks
            ok = True
            for w in range(2 if hits[i]["mate_status"] == 3 else 1):
                if aln is not None:
                    x0, span = int(aln[0][2 * i + w]), corpus.ref_len([int(x) for x in aln[3][int(aln[2][2 * i + w]):int(aln[2][2 * i + w + 1])]])
                else:
                    x0, span = max(int(hits[i]["pos"]), 0), int(hits[i]["read_len"]) + min(int(hits[i]["pos"]), 0)
                ok &= x0 + span <= L[hits[i]["tid"]]
            if ok:
                take.append(i)
        assert len(take) > 150
        sub = hits[take]
        off = np.arange(len(take) + 1, dtype=np.uint32)
        sub_aln = None
        if aln is not None:
            slots = [2 * i + w for i in take for w in (0, 1)]
            cnt = [int(aln[2][s + 1] - aln[2][s]) for s in slots]
            sub_aln = (aln[0][slots], aln[1][slots], np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64),
                       np.concatenate([aln[3][int(aln[2][s]):int(aln[2][s + 1])] for s in slots] + [np.zeros(0, np.uint32)]).astype(np.uint32))
        p = (np.arange(len(take)) % 255 + 1) / 256.0
        g_h, g_off, g_aln, _, g_src, st = H.project_alignments_host(sub, off, pl, sub_aln)
        assert st["records_out"] == len(take) and st["columns_beyond_model"] == 0 and g_src.tolist() == list(range(len(take)))
        pile = {}
        for j in range(len(g_h)):
            q = H.coverage_weight(p[j])
            for w in range(2 if g_h[j]["mate_status"] == 3 else 1):
                s = 2 * j + w
                x = int(g_aln[0][s])
                for word in g_aln[3][int(g_aln[2][s]):int(g_aln[2][s + 1])].tolist():
                    n, op = word >> 4, word & 15
                    if op in (0, 7, 8):
                        for k in range(n):
                            key = (int(g_h[j]["tid"]), x + k)
                            pile[key] = pile.get(key, 0) + q
                    if op in (0, 7, 8, 2, 3):
                        x += n
        t_runs, _, _ = H.coverage_host(L.astype(np.uint32), [(sub, off, p, None if sub_aln is None else (sub_aln[0], sub_aln[2], sub_aln[3]))])
        g_runs, _ = H.coverage_genome_host(t_runs, pl)
        want = {}
        for c, a, e, s in zip(*(x.tolist() for x in g_runs)):
            for g in range(a, e):
                want[(c, g)] = s
        assert pile == want and len(want) > 1000


GTF = (b'chrB\ts\texon\t101\t150\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n'
       b'chrB\ts\texon\t301\t400\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n'
       b'chrA\ts\texon\t11\t20\t.\t-\t.\tgene_id "h"; transcript_id "t2";\n'
       b'chrC\ts\texon\t11\t20\t.\t.\t.\tgene_id "h"; transcript_id "t3";\n')


def test_chrom_lengths(built, tmp_path):
    from sailfish_amd import genes
    gtf = tmp_path / "a.gtf"
    gtf.write_bytes(GTF)
    m = genes.ExonModel.from_gtf(str(gtf))
    assert m.chrom_names == [b"chrA", b"chrB", b"chrC"] and m.chrom_lengths() == [20, 400, 1]      # chrC holds no placed transcript
    sizes = tmp_path / "genome.fa.fai"
    sizes.write_bytes(b"chrB\t5000\t6\t60\t61\nchrZ\t9\nchrA\t3000\r\n\nchrC\t77\nchrA\t1\n")
    assert m.chrom_lengths(str(sizes)) == [3000, 5000, 77]
    sizes.write_bytes(b"chrB\t5000\nchrA\t3000\n")
    with pytest.raises(ValueError, match="chrC"):
        m.chrom_lengths(str(sizes))
    sizes.write_bytes(b"chrB\t5000\nchrA\tlong\n")
    with pytest.raises(ValueError, match=r"line 2\b"):
        m.chrom_lengths(str(sizes))


def test_option_errors_come_before_the_index(built, tmp_path, monkeypatch):
    from sailfish_amd import mapper
    monkeypatch.setattr(mapper, "QuasiIndex", lambda *a, **k: pytest.fail("an index was built"))
    gtf, other = tmp_path / "a.gtf", tmp_path / "b.gtf"
    gtf.write_bytes(GTF); other.write_bytes(GTF)
    out = str(tmp_path / "g.bam")
    call = lambda **kw: mapper.quantify_reads(["t"], ["ACGT" * 20], ["ACGT" * 10], None, "U", str(tmp_path / "out"), **kw)      # noqa: E731
    with pytest.raises(ValueError, match="needs genome_annotation"):
        call(write_genome_mappings=out)
    with pytest.raises(ValueError, match="need write_genome_mappings"):
        call(genome_annotation=str(gtf))
    with pytest.raises(ValueError, match="need write_genome_mappings"):
        call(genome_sizes=str(gtf))
    with pytest.raises(ValueError, match="write_genome_mappings: one path"):
        call(write_genome_mappings=7, genome_annotation=str(gtf))
    with pytest.raises(ValueError, match="one run reads one annotation"):
        call(write_genome_mappings=out, genome_annotation=str(gtf), write_genome_coverage=str(tmp_path / "g.bg"), coverage_annotation=str(other))
    with pytest.raises(ValueError, match="mappings_sorted"):
        call(write_genome_mappings=out, genome_annotation=str(gtf), mappings_sorted=True)
    with pytest.raises(ValueError, match="mappings_tags"):
        call(write_genome_mappings=out, genome_annotation=str(gtf), mappings_tags=True)                      # not oriented
    for kw in (dict(mappings_tags=True, mappings_oriented=True), dict(mappings_posteriors=True), dict(mappings_gapped=True, validate_mappings=True, max_indel=3)):
        with pytest.raises(ValueError, match="write_mappings or write_genome_mappings"):
            call(**kw)
    sizes = tmp_path / "sizes"
    sizes.write_bytes(b"chrA\t100\n")
    with pytest.raises(ValueError, match="chrB"):                                                           # the sizes are read before the index is built
        call(write_genome_mappings=out, genome_annotation=str(gtf), genome_sizes=str(sizes))
    bad = tmp_path / "bad.gtf"
    bad.write_bytes(b'chrA\ts\texon\t9\t5\t.\t+\t.\ttranscript_id "t";\n')
    with pytest.raises(ValueError, match="line 1"):
        call(write_genome_mappings=out, genome_annotation=str(bad))
    with pytest.raises(ValueError, match="needs genome_annotation"):
        mapper.quantify_files("t.fa", "r.fq", None, "U", str(tmp_path / "out"), write_genome_mappings=out)
    # with every keyword in order the run gets as far as the index: coverage_annotation alone serves as the annotation
    monkeypatch.setattr(mapper, "QuasiIndex", lambda *a, **k: (_ for _ in ()).throw(KeyError("reached the index")))
    for kw in (dict(genome_annotation=str(gtf)), dict(coverage_annotation=str(gtf)), dict(genome_annotation=str(gtf), coverage_annotation=str(gtf),
                                                                                         write_genome_coverage=str(tmp_path / "g.bg"))):
        with pytest.raises(KeyError, match="reached the index"):
            call(write_genome_mappings=out, mappings_format="bam", mappings_sorted=True, mappings_oriented=True, mappings_tags=True, mappings_posteriors=True, **kw)
