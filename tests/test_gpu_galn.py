"""The genome alignments on the device (sfgpu_galn_*, csrc/genomealn.hip; hits.project_alignments) against the statement
hits.project_alignments_host over the shared corpus (tests/galn_corpus.py) and every edge corpus: records, offsets, positions, words,
nm, MD, src_record and counters; the retry with too little room and the contract through the raw entries; samfile.SamDeviceWriter over
the chromosomes against the host writers; and write_genome_mappings= of mapper.quantify_reads end to end on a small spliced genome,
where every mapped line is walked along its CIGAR over the chromosome's own bases.  Every comparison is equality of integers or bytes."""
import ctypes as C
import gzip
import io
import os
import struct

import numpy as np
import pytest

import galn_corpus as corpus

pytestmark = pytest.mark.gpu


def _host(res):
    """a device result as the statement's arrays"""
    h, off, aln, tags, src, st = res
    n = lambda t, dt: t.cpu().numpy().view(dt).reshape(-1)      # noqa: E731
    return (n(h, corpus.HIT_DTYPE), n(off, np.uint32), (n(aln[0], np.int32), n(aln[1], np.uint32), n(aln[2], np.uint64), n(aln[3], np.uint32)),
            None if tags is None else (n(tags[0], np.uint32), n(tags[1], np.uint64), n(tags[2], np.uint8)), n(src, np.uint32), st)


def _same(got, want):
    assert got[0].tobytes() == np.ascontiguousarray(want[0], corpus.HIT_DTYPE).tobytes()
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[4], want[4])
    for g, w in zip(got[2], want[2]):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert (got[3] is None) == (want[3] is None)
    for g, w in zip(got[3] or (), want[3] or ()):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert {k: got[5][k] for k in want[5]} == want[5]


@pytest.fixture(scope="module")
def model(gpu):
    from sailfish_amd import hits as H
    with H.GenomeAlignments(corpus.model()[1], gpu) as g:
        yield g


@pytest.mark.parametrize("which", ["gapped", "untagged", "ungapped"])
def test_device_equals_the_statement(gpu, model, which):
    from sailfish_amd import hits as H
    b = corpus.ungapped() if which == "ungapped" else corpus.gapped()
    got = H.project_alignments(b["hits"], b["offsets"], model, b.get("alignments"), b.get("tags") if which == "gapped" else None)
    _same(_host(got), corpus.expected(which))


@pytest.mark.parametrize("what, delta", corpus.EDGES)
def test_device_equals_the_statement_at_the_block_edges(gpu, model, what, delta):
    from sailfish_amd import hits as H
    b, want = corpus.edge(what, delta)
    _same(_host(H.project_alignments(b["hits"], b["offsets"], model, b["alignments"], b["tags"])), want)


def test_too_little_room_is_asked_for_again(gpu, model):
    """the wrapper's second call, with the counts the library reported; and the statement through a placement instead of a handle"""
    from sailfish_amd import hits as H
    b, want = corpus.gapped(), corpus.expected("gapped")
    for room in ((1, 1 << 20), (1 << 20, 1), (0, 0), (want[5]["words_out"] - 1, len(want[3][2])), (want[5]["words_out"], len(want[3][2]))):
        _same(_host(H.project_alignments(b["hits"], b["offsets"], model, b["alignments"], b["tags"], _room=room)), want)
    _same(_host(H.project_alignments(b["hits"], b["offsets"], corpus.model()[1], b["alignments"], b["tags"], device=gpu)), want)
    assert all(model.stats[k] >= 5 * want[5][k] for k in H.GENOME_ALN_STATS)             # the handle sums what went through it


def test_the_contract_through_the_raw_entries(gpu, model):
    """too little room: SFGPU_ERR_RANGE with both counts set and nothing written; a tid that is no transcript: SFGPU_ERR_RANGE naming the
    lowest record; offsets that decrease, half an alignment, half the tags: SFGPU_ERR_INVALID; no read: one offset each; a refused
    model names its transcript"""
    import torch
    from sailfish_amd import _lib, hits as H
    L = _lib.lib()
    b, want = corpus.gapped(), corpus.expected("gapped")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(gpu)      # noqa: E731
    hits, off = t(b["hits"].view(np.uint8).reshape(-1), np.uint8), t(b["offsets"], np.int32)
    a_pos, a_nm, a_off, a_ops = (t(x, dt) for x, dt in zip(b["alignments"], (np.int32, np.int32, np.int64, np.int32)))
    t_nm, t_off, t_md = (t(x, dt) for x, dt in zip(b["tags"], (np.int32, np.int64, np.uint8)))
    n, R = len(b["hits"]), len(b["offsets"]) - 1
    sentinel = 0x5A
    o_hits = torch.full((24 * n,), sentinel, dtype=torch.uint8, device=gpu)
    o_off = torch.full((R + 1,), sentinel, dtype=torch.int32, device=gpu)
    o_pos, o_nm, o_tnm, src = (torch.full((2 * n,), sentinel, dtype=torch.int32, device=gpu) for _ in range(4))
    o_aoff, o_moff = (torch.full((2 * n + 1,), sentinel, dtype=torch.int64, device=gpu) for _ in range(2))
    ops = torch.full((want[5]["words_out"],), sentinel, dtype=torch.int32, device=gpu)
    md = torch.full((len(want[3][2]),), sentinel, dtype=torch.uint8, device=gpu)
    outs = (o_hits, o_off, o_pos, o_nm, o_tnm, src, o_aoff, o_moff, ops, md)

    def call(batch, cap_ops, cap_md):
        o = _lib.GalnOut(_lib.ptr(o_hits), _lib.ptr(o_off), _lib.ptr(o_pos), _lib.ptr(o_nm), _lib.ptr(o_aoff), _lib.ptr(ops), cap_ops, _lib.ptr(o_tnm),
                         _lib.ptr(o_moff), _lib.ptr(md), cap_md, _lib.ptr(src))
        st, need_ops, need_md = _lib.GalnStats(), C.c_uint64(7), C.c_uint64(7)
        with torch.cuda.device(gpu):
            rc = L.sfgpu_galn_project(model._h, C.byref(batch), C.byref(o), C.byref(need_ops), C.byref(need_md), C.byref(st), _lib.current_stream_ptr())
            torch.cuda.synchronize()
        return rc, need_ops.value, need_md.value, st

    full = lambda: _lib.GalnBatch(_lib.ptr(hits), _lib.ptr(off), R, 0, _lib.ptr(a_pos), _lib.ptr(a_off), _lib.ptr(a_ops), _lib.ptr(a_nm), _lib.ptr(t_nm),      # noqa: E731
                                  _lib.ptr(t_off), _lib.ptr(t_md))
    untouched = lambda: all(bool((x == sentinel).all()) for x in outs)      # noqa: E731
    for cap_ops, cap_md in ((ops.numel() - 1, md.numel()), (ops.numel(), md.numel() - 1), (0, 0)):
        rc, need_ops, need_md, _ = call(full(), cap_ops, cap_md)
        assert rc == _lib.ERR_RANGE and (need_ops, need_md) == (ops.numel(), md.numel()) and untouched()
    bad = b["hits"].copy()
    bad["tid"][[200, 77, 300]] = model.M
    bad_hits = t(bad.view(np.uint8).reshape(-1), np.uint8)
    batch = full(); batch.hits = _lib.ptr(bad_hits)
    rc, *_ = call(batch, ops.numel(), md.numel())
    assert rc == _lib.ERR_RANGE and "record 77 names transcript" in L.sfgpu_last_error().decode() and untouched()
    down = b["offsets"].copy(); down[5], down[9] = down[6] + 1, down[8] - 1
    bad_off = t(down, np.int32)
    batch = full(); batch.hit_off = _lib.ptr(bad_off)
    rc, *_ = call(batch, ops.numel(), md.numel())
    assert rc == _lib.ERR_INVALID and "read 5" in L.sfgpu_last_error().decode() and untouched()
    for field in ("aln_ops", "tag_md_off"):
        batch = full(); setattr(batch, field, None)
        assert call(batch, ops.numel(), md.numel())[0] == _lib.ERR_INVALID and untouched()
    rc, need_ops, need_md, st = call(full(), ops.numel(), md.numel())
    assert rc == _lib.OK and {k: int(getattr(st, k)) for k in H.GENOME_ALN_STATS} == want[5] and st.project_ms > 0
    m = want[5]["records_out"]
    assert o_hits[:24 * m].cpu().numpy().tobytes() == want[0].tobytes() and bool((o_hits[24 * m:] == sentinel).all()) and bool((src[m:] == sentinel).all())
    assert np.array_equal(ops.cpu().numpy().view(np.uint32), want[2][3]) and np.array_equal(md.cpu().numpy(), want[3][2])
    empty = _lib.GalnBatch(None, _lib.ptr(off[:1].contiguous()), 0, 0)
    assert call(empty, 0, 0)[:3] == (_lib.OK, 0, 0) and int(o_off[0]) == 0 and int(o_aoff[0]) == 0
    pl = corpus.model()[1]
    overlap = pl._replace(exon_start=np.where(np.arange(len(pl.exon_start)) == 4, 1005, pl.exon_start).astype(np.uint32))      # j_plus' second block into its first
    with pytest.raises(_lib.SfgpuError, match="transcript 1 "):
        H.GenomeAlignments(overlap, gpu)


def _device_reads(seqs, gpu):
    import sailfish_amd as sf
    return tuple(tuple(x.to(gpu) for x in sf.mapper.pack_sequences([s[m] for s in seqs])) for m in (0, 1))


@pytest.mark.parametrize("fmt, sort", [("sam", None), ("bam", None), ("bam", "coordinate")])
def test_the_device_writer_over_the_chromosomes(gpu, model, tmp_path, fmt, sort):
    """the projected batch through SamDeviceWriter opened over the chromosomes' names and lengths: the bytes of the host writers over
    the statement's batch, and for the sorted file the index build_bai makes of it"""
    from sailfish_amd import hits as H, samfile
    b, want = corpus.gapped(), corpus.expected("gapped")
    h, off, aln, tags, src, _ = H.project_alignments(b["hits"], b["offsets"], model, b["alignments"], b["tags"])
    p, rec, f32, _ = H.posteriors_host(b["hits"], b["offsets"], np.linspace(0.5, 3.0, model.M))
    import torch
    post = tuple(torch.from_numpy(np.ascontiguousarray(x).copy()).to(gpu)[src.long()] for x in (p, rec.view(np.int32), f32))
    path = str(tmp_path / ("genome." + fmt))
    w = samfile.SamDeviceWriter(path, corpus.CHROM_NAMES, corpus.CHROM_LENGTHS, True, format=fmt, oriented=True, sort=sort)
    w.write(h, off, seqs=_device_reads(b["seqs"], gpu), alignments=aln, tags=tags, posteriors=post)
    w.close()
    kw = dict(seqs=b["seqs"], oriented=True, alignments=want[2], tags=want[3], posteriors=(p[want[4]],))
    host = str(tmp_path / ("host." + fmt))
    if fmt == "sam":
        samfile.write_sam(host, corpus.CHROM_NAMES, corpus.CHROM_LENGTHS, want[0], want[1], **kw)
        assert open(path, "rb").read() == open(host, "rb").read()
        return
    samfile.write_bam(host, corpus.CHROM_NAMES, corpus.CHROM_LENGTHS, want[0], want[1], sort=sort, **kw)
    got = open(path, "rb").read()
    assert gzip.decompress(got) == gzip.decompress(open(host, "rb").read())
    if sort:
        assert open(path + ".bai", "rb").read() == samfile.build_bai(got)
        assert len(samfile.fetch(path, "chr1", 1012, 1015)) >= 8             # the records spliced over j_plus' first intron


# ---- end to end -------------------------------------------------------------------------------------------------------------------

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _records(stream):
    """the records of an inflated BAM stream -> (reference names, [(refID, pos, flag, [(len, op)], seq bytes, the record's bytes)])"""
    from sailfish_amd import samfile
    names, lengths, p, _ = samfile._bam_header(stream)
    refs, out = list(zip(names, lengths)), []
    while p < len(stream):
        size = struct.unpack_from("<i", stream, p)[0]
        ref, pos, l_name, _, _, n_ops, flag, l_seq = struct.unpack_from("<iiBBHHHi", stream, p + 4)
        at = p + 36 + l_name
        ops = [(w >> 4, w & 15) for w in struct.unpack_from("<%dI" % n_ops, stream, at)]
        packed = stream[at + 4 * n_ops:at + 4 * n_ops + (l_seq + 1) // 2]
        seq = bytes(b"=ACMGRSVTWYHKDBN"[(packed[i >> 1] >> (4 if i % 2 == 0 else 0)) & 15] for i in range(l_seq))
        out.append((ref, pos, flag, ops, seq, stream[p:p + 4 + size]))
        p += 4 + size
    return refs, out


def _host_statement(idx, names, r1, r2, batch, weights, placement, chrom_lengths, transcript=False):
    """the sorted file's inflated stream by the host statements over the device's own records, batch by batch"""
    import sailfish_amd as sf
    from sailfish_amd import hits as H, samfile
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)
    body, spliced = [], {1: 0, -1: 0}
    total = dict.fromkeys(H.GENOME_ALN_STATS, 0)
    for a in range(0, len(r1), batch):
        p1, p2 = r1[a:a + batch], r2[a:a + batch]
        h, o = sf.mapper.hits_to_numpy(*idx.map_reads(p1, p2, validate=dict(min_identity=1.0, keep_best=False), tags=True))
        t = tuple(x.cpu().numpy() for x in idx.last_tags)
        tags = (t[0].view(np.uint32), t[1].view(np.uint64), t[2])
        p = H.posteriors_host(h, o, weights)[0]
        qn = [b"r%d" % (a + i) for i in range(len(p1))]
        if transcript:
            head = len(samfile.sam_header(names, ref_len))
            body.append(samfile._sam_text(names, ref_len, h, o, qn, list(zip(p1, p2)), oriented=True, tags=tags, posteriors=(p,))[head:])
            continue
        g_h, g_o, g_aln, g_tags, src, st = H.project_alignments_host(h, o, placement, None, tags)
        for k in total:
            total[k] += st[k]
        for j in range(len(g_h)):                          # the spliced lines by the transcript's strand
            for w in range(2 if g_h[j]["mate_status"] == 3 else 1):
                s = 2 * j + w
                if any(int(x) & 15 == 3 for x in g_aln[3][int(g_aln[2][s]):int(g_aln[2][s + 1])]):
                    spliced[int(placement.strand[h[src[j]]["tid"]])] += 1
        head = len(samfile.sam_header(placement.chrom_names, chrom_lengths))
        body.append(samfile._sam_text(placement.chrom_names, chrom_lengths, g_h, g_o, qn, list(zip(p1, p2)), oriented=True, alignments=g_aln, tags=g_tags,
                                      posteriors=(p[src],))[head:])
    if transcript:
        return samfile.sort_bam_stream(samfile.sam_to_bam(samfile.sam_header(names, ref_len, "coordinate") + b"".join(body)))
    return samfile.sort_bam_stream(samfile.sam_to_bam(samfile.sam_header(placement.chrom_names, chrom_lengths, "coordinate") + b"".join(body))), spliced, total


def test_quantify_reads_writes_the_genome_mappings(gpu, tmp_path):
    """quantify_reads(write_genome_mappings=, genome_annotation=) on the spliced genome, 300 error-free pairs in three batches, as a
    sorted, oriented, tagged BAM with posteriors: every mapped line's SEQ, walked along its CIGAR over the chromosome's own bases,
    matches in every M column; every N is an intron of the GTF; the file is the host statement's; quant.sf, aux/ and the transcript
    mappings file beside it are those of the run without the keywords; and the keywords work without write_mappings"""
    import sailfish_amd as sf
    from sailfish_amd import genes, hits as H, samfile
    names, seqs, r1, r2, gtf_bytes, chroms = corpus.genome()
    gtf = tmp_path / "genome.gtf"
    gtf.write_bytes(gtf_bytes)
    log = []
    sopt = lambda: sf.SailfishOpts(jointLog=lambda lvl, msg: log.append((lvl, msg)))      # noqa: E731
    opts = dict(batch_reads=100, device=gpu, cmd_options={"libType": "IU"}, validate_mappings=True, min_identity=1.0, mappings_format="bam", mappings_sorted=True,
                mappings_oriented=True, mappings_tags=True, mappings_posteriors=True)
    run = lambda tag, **kw: sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / tag), sopt(), **opts, **kw)      # noqa: E731
    rc, exp0 = run("plain", write_mappings=str(tmp_path / "plain.bam"))
    assert rc == 0 and exp0.genome_mappings_stats is None
    del log[:]
    rc, exp = run("both", write_mappings=str(tmp_path / "both.bam"), write_genome_mappings=str(tmp_path / "both.genome.bam"), genome_annotation=str(gtf))
    assert rc == 0
    for ext in ("bam", "bam.bai"):
        assert (tmp_path / ("both." + ext)).read_bytes() == (tmp_path / ("plain." + ext)).read_bytes()
    skip = {"meta_info.json", "cmd_info.json"}
    for d in ("", "aux"):
        a, b = sorted(os.listdir(tmp_path / "both" / d)), sorted(os.listdir(tmp_path / "plain" / d))
        assert a == b
        for x in a:
            if x not in skip and os.path.isfile(tmp_path / "both" / d / x):
                read = gzip.decompress if x.endswith(".gz") else bytes
                assert read((tmp_path / "both" / d / x).read_bytes()) == read((tmp_path / "plain" / d / x).read_bytes()), (d, x)
    # the host statement
    model = genes.ExonModel.from_gtf(str(gtf))
    placement, lengths = model.for_names(names), model.chrom_lengths()
    assert model.chrom_names == [b"chr10", b"chrA", b"chrB"] and placement.status.tolist() == [0] * 18
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    weights = exp.posterior_weights.cpu().numpy()
    want, spliced, total = _host_statement(idx, names, r1, r2, 100, weights, placement, lengths)
    assert spliced[1] >= 20 and spliced[-1] >= 20, spliced                          # the walk below cannot pass vacuously
    got = (tmp_path / "both.genome.bam").read_bytes()
    stream = gzip.decompress(got)
    assert stream == want
    assert (tmp_path / "both.genome.bam.bai").read_bytes() == samfile.build_bai(got)
    assert gzip.decompress((tmp_path / "both.bam").read_bytes()) == _host_statement(idx, names, r1, r2, 100, weights, placement, lengths, transcript=True)
    idx.close()
    st = exp.genome_mappings_stats
    assert {k: st[k] for k in total} == total and st["transcripts"] == st["transcripts_placed"] == 18 and total["records_out"] == total["records_in"] > 300
    line = [m for lvl, m in log if m.startswith("genome mappings:")]
    assert len(line) == 1 and f"{total['lines_spliced']} of them spliced by {total['n_operations']} N operations" in line[0]
    assert not [m for lvl, m in log if lvl == 1 and "write_genome_mappings" in m]
    # the walk over the chromosomes' own bases, and the introns
    introns = set()
    for t in model.transcripts.values():
        blocks = sorted(t[3])
        introns |= {(t[1], a[0] + a[1], b[0]) for a, b in zip(blocks, blocks[1:])}
    refs, records = _records(stream)
    assert [r[0] for r in refs] == ["chr10", "chrA", "chrB"] and [r[1] for r in refs] == lengths
    mapped = n_N = 0
    for ref, pos, flag, ops, seq, _ in records:
        if flag & 4:
            continue
        mapped += 1
        chrom, g, q = chroms[model.chrom_names[ref]], pos, 0
        for n, op in ops:
            if op == 0:
                assert seq[q:q + n] == chrom[g:g + n], (ref, pos, ops)
                q += n; g += n
            elif op == 3:
                assert (ref, g, g + n) in introns, (ref, pos, ops)
                g += n; n_N += 1
            else:
                assert op == 4, (ref, pos, ops)
                q += n
        assert q == len(seq) == 40
    assert mapped == total["lines"] and n_N == total["n_operations"] > 40
    # the genome file alone, into a file object, with a sizes file for the @SQ lengths
    sizes = tmp_path / "chrom.sizes"
    sizes.write_bytes(b"".join(b"%s\t%d\n" % (c, len(s)) for c, s in chroms.items()))
    out = io.BytesIO()
    rc, exp1 = run("alone", write_genome_mappings=out, genome_annotation=str(gtf), genome_sizes=str(sizes))
    assert rc == 0 and exp1.genome_mappings_stats == exp.genome_mappings_stats
    refs1, records1 = _records(gzip.decompress(out.getvalue()))
    assert [r[1] for r in refs1] == [2500, 2500, 3000] and [r[5] for r in records1] == [r[5] for r in records]
    assert (tmp_path / "alone" / "quant.sf").read_bytes() == (tmp_path / "plain" / "quant.sf").read_bytes()
    assert not [x for x in os.listdir(tmp_path) if x.startswith("alone") and os.path.isfile(tmp_path / x)]
    # an annotation that knows other names: every record is dropped, every read written unmapped, the log warns
    other = tmp_path / "other.gtf"
    other.write_bytes(gtf_bytes.replace(b'transcript_id "g', b'transcript_id "G'))
    del log[:]
    rc, exp2 = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "none"), sopt(), batch_reads=100, device=gpu, cmd_options={"libType": "IU"},
                                        write_genome_mappings=str(tmp_path / "none.sam"), genome_annotation=str(other))
    st = exp2.genome_mappings_stats
    assert rc == 0 and st["records_out"] == 0 and st["records_unplaced"] == st["records_in"] > 0 and st["transcripts_placed"] == 0
    flags = [int(ln.split(b"\t")[1]) for ln in (tmp_path / "none.sam").read_bytes().split(b"\n") if ln and not ln.startswith(b"@")]
    assert flags == [77, 141] * 300 and [m for lvl, m in log if lvl == 1 and "places none of the 18" in m]
