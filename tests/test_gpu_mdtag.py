"""The NM / MD tags on the device (csrc/mdtag.hip: sfgpu_hits_md_tags; hits.md_tags) against the Python statement
hits.md_tags_host: array for array and byte for byte over the shared corpus (tests/mdtag_corpus.py), with and without alignments,
and the contract's shapes and errors through the raw entry; the device writers with the tags handed in
(samfile.SamDeviceWriter.write(tags=): "sam", "sam.gz", "bam" and the sorted "bam" with its index) against the host statements
samfile._sam_text(tags=), sam_to_bam, write_bam(sort="coordinate") and build_bai, with a tile edge on every byte of the tag fields;
and mappings_tags= of mapper.quantify_reads / quantify_files end to end."""
import ctypes as C

import numpy as np
import pytest

import mdtag_corpus as corpus
from test_gpu_aligng import _aln_device, _device, _index, _reads

pytestmark = pytest.mark.gpu


def _numpy(nm, md_off, md):
    return nm.cpu().numpy().view(np.uint32), md_off.cpu().numpy().view(np.uint64), md.cpu().numpy()


def _same(got, want, what):
    nm, md_off, md, st = got
    assert np.array_equal(md_off, want[1]), what
    assert np.array_equal(nm, want[0]), what
    assert md.tobytes() == want[2].tobytes(), what
    assert st == want[3], (what, st, want[3])


@pytest.mark.parametrize("name", sorted(n for n in corpus.cases() if n != "no_reads"))
def test_device_equals_the_statement(gpu, name):
    """every case of the corpus: nm, md_off, the MD bytes and the stats are the statement's; once more with every read at an offset
    that is no multiple of 16"""
    from sailfish_amd import hits as H
    case, aln = corpus.cases()[name]
    want = corpus.expected(name)
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    d_aln = None if aln is None else _aln_device(aln, gpu)
    for lead1, lead2 in ((b"", b""), (b"xyz", b"NNNNNNN")):
        r1, r2 = _reads(case, gpu, lead1, lead2)
        nm, md_off, md, st = H.md_tags(idx, d_hits, d_off, r1, r2, d_aln)
        _same((*_numpy(nm, md_off, md), st), want, (name, lead1))
    idx.close()


def _raw(idx, s1, o1, s2, o2, n_reads, d_hits, d_off, a_pos, a_off, a_ops, nm, md_off, md, cap, n_md=True, stats=True, index=True):
    """sfgpu_hits_md_tags itself -> (rc, n_md, stats)"""
    import torch
    from sailfish_amd import _lib
    st = _lib.MdTagStats()
    n = C.c_uint64(12345)
    with torch.cuda.device(idx.device):
        torch.cuda.synchronize()
        rc = _lib.lib().sfgpu_hits_md_tags(idx._h if index else None, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), n_reads, _lib.ptr(d_hits),
                                           _lib.ptr(d_off), _lib.ptr(a_pos), _lib.ptr(a_off), _lib.ptr(a_ops), _lib.ptr(nm), _lib.ptr(md_off), _lib.ptr(md), cap,
                                           C.byref(n) if n_md else None, C.byref(st) if stats else None, _lib.current_stream_ptr())
        torch.cuda.synchronize()
    return rc, n.value, st.as_dict()


def test_shapes_and_errors_of_the_contract(gpu):
    """no records; n_reads == 0; room for one MD byte too few: SFGPU_ERR_RANGE, the need reported exactly, the outputs untouched, and
    md_tags repeats the call once; tid >= M: SFGPU_ERR_RANGE naming the lowest record; null pointers, an alignment given in part and
    mate 2 in a single-end batch: SFGPU_ERR_INVALID, the outputs untouched"""
    import torch
    from sailfish_amd import _lib
    from sailfish_amd import hits as H
    name = "ag_edges_pe_aligned"
    case, aln = corpus.cases()[name]
    want = corpus.expected(name)
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    (s1, o1), (s2, o2) = _reads(case, gpu)
    a_pos, _, a_off, a_ops = _aln_device(aln, gpu)
    R, n = len(case["r1"]), len(case["hits"])
    zero = dict.fromkeys(H.MDTAG_STATS, 0)
    need = len(want[2])
    fresh = lambda: [torch.full((m,), 0x5A, dtype=torch.uint8, device=gpu) for m in (2 * n * 4, (2 * n + 1) * 8, need)]
    untouched = lambda ts: all(bool((t == 0x5A).all().item()) for t in ts)
    # no records at all, and no reads
    none_o = torch.zeros(R + 1, dtype=torch.int32, device=gpu)
    nm, md_off, md, st = H.md_tags(idx, torch.zeros(0, dtype=torch.uint8, device=gpu), none_o, (s1, o1), (s2, o2))
    assert nm.numel() == 0 and md.numel() == 0 and md_off.tolist() == [0] and st == zero
    one = torch.full((1,), 7, dtype=torch.int64, device=gpu)
    rc, n_md, st = _raw(idx, None, None, None, None, 0, None, None, None, None, None, None, one, None, 0)
    assert rc == 0 and n_md == 0 and one.item() == 0 and st == zero
    nm, md_off, md, st = H.md_tags(idx, *_device(corpus.cases()["no_reads"][0], gpu), (torch.zeros(0, dtype=torch.uint8, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu)))
    assert nm.numel() == 0 and md.numel() == 0 and md_off.tolist() == [0] and st == zero
    # the whole thing, raw, with exactly the room it needs
    args = dict(idx=idx, s1=s1, o1=o1, s2=s2, o2=o2, n_reads=R, d_hits=d_hits, d_off=d_off, a_pos=a_pos, a_off=a_off, a_ops=a_ops)
    outs = fresh()
    rc, n_md, st = _raw(**args, nm=outs[0], md_off=outs[1], md=outs[2], cap=need)
    assert rc == 0 and n_md == need and st == want[3]
    got = [t.cpu().numpy().view(dt) for t, dt in zip(outs, (np.uint32, np.uint64, np.uint8))]
    assert all(np.array_equal(g, w) for g, w in zip(got, want[:3]))
    # one byte too few, and none
    for cap in (need - 1, 0):
        outs = fresh()
        rc, n_md, st = _raw(**args, nm=outs[0], md_off=outs[1], md=outs[2] if cap else None, cap=cap)
        assert rc == _lib.ERR_RANGE and n_md == need and untouched(outs), cap
    # md_tags sizes the MD at eight bytes a record and repeats the call once: a batch of mismatches needs more
    heavy, _ = corpus.cases()["heavy_se"]
    hidx = _index(heavy, gpu)
    nm, md_off, md, st = H.md_tags(hidx, heavy["hits"], heavy["off"], heavy["r1"])
    assert md.numel() > 8 * len(heavy["hits"])
    _same((*_numpy(nm, md_off, md), st), corpus.expected("heavy_se"), "retry")
    hidx.close()
    # tid >= M
    bad = case["hits"].copy()
    bad["tid"][[40, 17, 99]] = len(case["seqs"])
    bad_hits = torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).to(gpu)
    outs = fresh()
    rc, _, _ = _raw(**{**args, "d_hits": bad_hits}, nm=outs[0], md_off=outs[1], md=outs[2], cap=need)
    assert rc == _lib.ERR_RANGE and b"record 17 " in _lib.lib().sfgpu_last_error() and untouched(outs)
    with pytest.raises(_lib.SfgpuError, match="record 17 "):
        H.md_tags(idx, bad_hits, d_off, (s1, o1), (s2, o2))
    full = dict(args, nm=outs[0], md_off=outs[1], md=outs[2], cap=need)
    for change in (dict(index=False), dict(n_md=False), dict(stats=False), dict(md_off=None), dict(s1=None), dict(o1=None), dict(o2=None), dict(d_off=None),
                   dict(d_hits=None), dict(nm=None), dict(md=None), dict(a_pos=None), dict(a_off=None), dict(a_ops=None), dict(a_pos=None, a_off=None),
                   dict(a_off=None, a_ops=None), dict(s2=None, o2=None)):          # (the last: records name mate 2)
        rc, _, _ = _raw(**{**full, **change})
        assert rc == _lib.ERR_INVALID, change
    assert b"mate 2" in _lib.lib().sfgpu_last_error() and untouched(outs)
    idx.close()


# ---- the writers take the tags ----------------------------------------------------------------------------------------------------

def _t64(a, gpu, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to(gpu)


def _tags_device(tags, gpu):
    return _t64(tags[0], gpu, np.int32), _t64(tags[1], gpu, np.int64), _t64(tags[2], gpu, np.uint8)


def _written(case, aln, tags, gpu, fmt, sort=None, chunk_bytes=0, cuts=None, read_names=None, say_none=False):
    """the case through an oriented SamDeviceWriter in one batch, or in the batches cut at the reads `cuts` -> (the file's bytes, the
    index's).  say_none: write(tags=None), said aloud"""
    import io
    from sailfish_amd import samfile
    from test_gpu_aligng import corpus as AG
    names, ref_len, _ = AG.sam_inputs(case)
    paired = AG.is_paired(case)
    f, x = io.BytesIO(), io.BytesIO()
    w = samfile.SamDeviceWriter(f, names, ref_len, paired, format=fmt, oriented=True, sort=sort, chunk_bytes=chunk_bytes, index=x if sort else None)
    edges = [0] + list(cuts or []) + [len(case["r1"])]
    for a, b in zip(edges[:-1], edges[1:]):
        h0, h1 = int(case["off"][a]), int(case["off"][b])
        part = dict(seqs=case["seqs"], r1=case["r1"][a:b], r2=None if case["r2"] is None else case["r2"][a:b], hits=case["hits"][h0:h1],
                    off=(case["off"][a:b + 1] - case["off"][a]).astype(np.uint32))
        d_hits, d_off = _device(part, gpu)
        r1, r2 = _reads(part, gpu)
        d_aln, kw = None, (dict(tags=None) if say_none else {})
        if aln is not None:
            pos, nm, op_off, ops = aln[:4]
            w0, w1 = int(op_off[2 * h0]), int(op_off[2 * h1])
            d_aln = _aln_device((pos[2 * h0:2 * h1], nm[2 * h0:2 * h1], op_off[2 * h0:2 * h1 + 1] - op_off[2 * h0], ops[w0:w1]), gpu)
        if tags is not None:
            nm, md_off, md = tags
            m0, m1 = int(md_off[2 * h0]), int(md_off[2 * h1])
            d_tags = _tags_device((nm[2 * h0:2 * h1], md_off[2 * h0:2 * h1 + 1] - md_off[2 * h0], md[m0:m1]), gpu)
            kw = dict(tags=d_tags)
        w.write(d_hits, d_off, seqs=(r1, r2) if paired else r1, alignments=d_aln, read_names=None if read_names is None else read_names[a:b], **kw)
    w.close()
    return f.getvalue(), x.getvalue()


def _host_text(case, aln, tags, read_names=None):
    from sailfish_amd import samfile
    from test_gpu_aligng import corpus as AG
    names, ref_len, seqs = AG.sam_inputs(case)
    return samfile._sam_text(names, ref_len, case["hits"], case["off"], read_names, seqs, oriented=True, alignments=aln, tags=tags)


@pytest.mark.parametrize("name", corpus.WRITABLE)
def test_writers_write_the_tags(gpu, tmp_path, name):
    """"sam", "sam.gz", "bam" and the sorted "bam" with its index: byte-equal (the compressed ones inflated) to _sam_text(tags=),
    sam_to_bam of it and write_bam(sort="coordinate", tags=); the index is build_bai of the device's own file and fetch returns the
    records; a small chunk_bytes and three batches change nothing; with tags=None every file is the one written without the
    argument"""
    import gzip
    from sailfish_amd import samfile
    from test_gpu_aligng import corpus as AG
    case, aln, tags = corpus.writable(name)
    names, ref_len, seqs = AG.sam_inputs(case)
    text = _host_text(case, aln, tags)
    bam = samfile.sam_to_bam(text)
    assert _written(case, aln, tags, gpu, "sam")[0] == text
    assert gzip.decompress(_written(case, aln, tags, gpu, "sam.gz")[0]) == text
    assert gzip.decompress(_written(case, aln, tags, gpu, "bam")[0]) == bam
    path = str(tmp_path / "sorted.bam")
    samfile.write_bam(path, names, ref_len, case["hits"], case["off"], seqs=seqs, oriented=True, sort="coordinate", alignments=aln, tags=tags)
    got, bai = _written(case, aln, tags, gpu, "bam", sort="coordinate")
    assert gzip.decompress(got) == gzip.decompress(open(path, "rb").read())
    assert bai == samfile.build_bai(got) and len(bai) >= 8
    if len(case["hits"]):
        dev_path = str(tmp_path / "device.bam")
        open(dev_path, "wb").write(got); open(dev_path + ".bai", "wb").write(bai)
        tid = int(case["hits"]["tid"][0])
        tname = names[tid].decode() if isinstance(names[tid], bytes) else names[tid]
        found = list(samfile.fetch(dev_path, tname, 0, int(ref_len[tid])))
        assert found and found == list(samfile.fetch(path, tname, 0, int(ref_len[tid]), bai=samfile.build_bai(path)))
    longest = max(len(l) for l in text.split(b"\n")) + 1
    chunk = max(4096, 4 * longest + 64)                               # (a unit fits: the two lines of a pair; a BAM record's QUAL is as long as SEQ)
    R = len(case["r1"])
    for fmt, want in (("sam", text), ("bam", bam)):
        small = _written(case, aln, tags, gpu, fmt, chunk_bytes=chunk, cuts=[R // 3, R // 3 + 1] if R > 3 else None)[0]
        assert (small if fmt == "sam" else gzip.decompress(small)) == want, fmt
    plain = _host_text(case, aln, None)
    for fmt, sort in (("sam", None), ("sam.gz", None), ("bam", None), ("bam", "coordinate")):
        before = _written(case, aln, None, gpu, fmt, sort=sort)
        assert _written(case, aln, None, gpu, fmt, sort=sort, say_none=True) == before, (fmt, sort)
        if sort is None:
            body = before[0] if fmt == "sam" else gzip.decompress(before[0])
            assert body == (samfile.sam_to_bam(plain) if fmt == "bam" else plain), fmt


def test_a_tile_edge_on_every_byte_of_the_tag_fields(gpu):
    """the batch whose first QNAME is 1 .. 64 bytes long, so that the 4 096-byte tile edges move a byte a step through the lines'
    tag fields (tests/test_mdtag_cpu.py shows that they meet every offset): text and BAM records equal the statement for every length"""
    import gzip
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    for n in range(1, 65):
        case, names = corpus.qnames_case(n)
        tags = H.md_tags_host(case["seqs"], case["hits"], case["off"], case["r1"], None)[:3]
        text = _host_text(case, None, tags, names)
        assert _written(case, None, tags, gpu, "sam", read_names=names)[0] == text, n
        assert gzip.decompress(_written(case, None, tags, gpu, "bam", read_names=names)[0]) == samfile.sam_to_bam(text), n


def test_what_the_writer_refuses_with_tags(gpu):
    """an unalignable slot still fails the batch as "no base on the transcript" at the lowest (read, record), in every format, before a
    byte is written; tags without the bases, on a writer that is not oriented, or of another batch: ValueError; the raw entry without
    the mates' offsets, or with a part of the tags: SFGPU_ERR_INVALID"""
    import io
    from sailfish_amd import _lib
    from sailfish_amd import samfile
    from test_gpu_aligng import corpus as AG
    case, aln = corpus.cases()["hand_ops"]
    tags = _tags_device(corpus.expected("hand_ops")[:3], gpu)
    names, ref_len, _ = AG.sam_inputs(case)
    d_hits, d_off = _device(case, gpu)
    r1, _ = _reads(case, gpu)
    for fmt, sort in (("sam", None), ("bam", None), ("bam", "coordinate")):
        f = io.BytesIO()
        w = samfile.SamDeviceWriter(f, names, ref_len, False, format=fmt, sort=sort, index=False, oriented=True)
        with pytest.raises(ValueError, match="read 8, record 0: the read has no base on the transcript"):
            w.write(d_hits, d_off, seqs=r1, alignments=_aln_device(aln, gpu), tags=tags)
        w.close()
        if fmt == "sam":
            assert f.getvalue() == samfile.sam_header(names, ref_len)
    w = samfile.SamDeviceWriter(io.BytesIO(), names, ref_len, False, oriented=True)
    with pytest.raises(ValueError, match="bases"):
        w.write(d_hits, d_off, tags=tags)
    with pytest.raises(ValueError, match="slots"):
        w.write(d_hits, d_off, seqs=r1, tags=_tags_device(corpus.writable("runs_se")[2], gpu))
    # the raw entry
    batch, keep = w._batch_args(d_hits, d_off, None, r1, None, None)
    sink = _lib.TEXT_SINK(lambda addr, nb, user: 0)
    res = _lib.SamWriteResult()
    full = tuple(_lib.ptr(t) for t in tags)

    def call(no_bases, t):
        b = _lib.SamwBatch.from_buffer_copy(batch)
        if no_bases:
            b.seq1, b.seq1_off = None, None
        b.tag_nm, b.tag_md_off, b.tag_md = t
        return _lib.lib().sfgpu_sam_write_text(C.byref(b), w.chunk_bytes, sink, None, C.byref(res), _lib.current_stream_ptr())
    assert call(True, full) == _lib.ERR_INVALID and b"bases" in _lib.lib().sfgpu_last_error()
    for part in ((None, full[1], full[2]), (full[0], None, full[2]), (full[0], full[1], None)):
        assert call(False, part) == _lib.ERR_INVALID and b"tags" in _lib.lib().sfgpu_last_error()
    assert call(True, (None, None, None)) == _lib.OK
    w.close()
    w = samfile.SamDeviceWriter(io.BytesIO(), names, ref_len, False)
    with pytest.raises(ValueError, match="oriented"):
        w.write(d_hits, d_off, seqs=r1, tags=tags)
    w.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def test_quantify_writes_tagged_mappings(gpu, tmp_path):
    """quantify_reads / quantify_files(mappings_tags=True) on a small spliced transcriptome with substitutions and indels: the same
    quant.sf as without the option; the mappings file is write_sam(tags=) of the same records, ungapped and with mappings_gapped, as
    "sam" and as the sorted "bam" with its index; tag_stats is the summed per-batch stats and one log line names them; quantify_sam on
    the tagged file gives the same estimates; map_reads leaves last_tags with and without validation; the ValueError combinations"""
    import gzip
    import os
    import torch
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    from test_gpu_aligng import _spliced_indel_reads
    names, seqs, reads = _spliced_indel_reads(n_reads=300)
    batch = 120
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)
    # map_reads: the tags of what it returns, with and without validation, over the alignment where there is one
    h, o = idx.map_reads(reads, tags=True)
    want = H.md_tags(idx, h, o, reads)
    assert all(torch.equal(a, b) for a, b in zip(idx.last_tags, want[:3])) and idx.last_tag_stats == want[3] and want[3]["sum_nm"] > 100
    h, o = idx.map_reads(reads, validate=dict(max_indel=3, align=True, tags=True))
    want = H.md_tags(idx, h, o, reads, alignments=idx.last_alignments)
    assert all(torch.equal(a, b) for a, b in zip(idx.last_tags, want[:3])) and idx.last_tag_stats == want[3]
    assert torch.equal(idx.last_tags[0], idx.last_alignments[1])                  # nm is the align pass's
    idx.map_reads(reads, validate=dict(max_indel=3))
    assert idx.last_tags is None and idx.last_tag_stats is None
    bodies = {False: [], True: []}
    totals = {False: dict.fromkeys(H.MDTAG_STATS, 0), True: dict.fromkeys(H.MDTAG_STATS, 0)}
    for a in range(0, len(reads), batch):
        part = reads[a:a + batch]
        bh, bo = sf.mapper.hits_to_numpy(*idx.map_reads(part))
        fh, fo, _, _ = H.verify_hits_gapped_host(seqs, bh, bo, part, None, 900, False, 3)
        for gapped in (False, True):
            aln = H.align_hits_host(seqs, fh, fo, part, None, 3) if gapped else None
            tags = H.md_tags_host(seqs, fh, fo, part, None, aln)
            if gapped:
                assert np.array_equal(tags[0], aln[1])
            text = samfile._sam_text(names, ref_len, fh, fo, [b"r%d" % (a + i) for i in range(len(part))], part, oriented=True, alignments=aln, tags=tags[:3])
            bodies[gapped].append(text[len(samfile.sam_header(names, ref_len)):])
            for key, v in tags[3].items():
                totals[gapped][key] = max(totals[gapped][key], v) if key == "max_md_bytes" else totals[gapped][key] + v
    idx.close()
    log = []
    sopt = lambda: sf.SailfishOpts(jointLog=lambda lvl, msg: log.append(msg))
    kw = dict(batch_reads=batch, device=gpu, cmd_options={"libType": "U"}, validate_mappings=True, max_indel=3, mappings_oriented=True)
    rc, exp0 = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "plain"), sopt(), write_mappings=str(tmp_path / "plain.sam"), **kw)
    assert rc == 0 and exp0.tag_stats is None and not [m for m in log if m.startswith("tagged mappings")]
    quant = (tmp_path / "plain" / "quant.sf").read_bytes()
    for gapped in (False, True):
        del log[:]
        out = "tagged%d" % gapped
        rc, exp = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / out), sopt(), write_mappings=str(tmp_path / (out + ".sam")),
                                           mappings_tags=True, mappings_gapped=gapped, **kw)
        assert rc == 0 and exp.tag_stats == totals[gapped] and exp.verify_stats == exp0.verify_stats
        line = [m for m in log if m.startswith("tagged mappings")]
        assert len(line) == 1 and f"on {totals[gapped]['slots']} lines" in line[0] and f"NM sums to {totals[gapped]['sum_nm']}" in line[0]
        want = samfile.sam_header(names, ref_len) + b"".join(bodies[gapped])
        assert (tmp_path / (out + ".sam")).read_bytes() == want
        assert (tmp_path / out / "quant.sf").read_bytes() == quant
    assert totals[True]["sum_nm"] < totals[False]["sum_nm"] and totals[False]["slots_plain"] > 20
    # without validation the tags are those of every record the mapper found
    rc, exp = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "raw"), sopt(), write_mappings=str(tmp_path / "raw.sam"), mappings_tags=True,
                                       mappings_oriented=True, batch_reads=batch, device=gpu, cmd_options={"libType": "U"})
    assert rc == 0 and exp.tag_stats["slots"] == (tmp_path / "raw.sam").read_bytes().count(b"\tNM:i:") > 0
    # from the files on, and the sorted BAM with its index
    (tmp_path / "tx.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    (tmp_path / "reads.fa").write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    rc, expf = sf.mapper.quantify_files(str(tmp_path / "tx.fa"), str(tmp_path / "reads.fa"), None, "U", str(tmp_path / "files"), sopt(),
                                        write_mappings=str(tmp_path / "files.sam"), mappings_tags=True, mappings_gapped=True, **kw)
    assert rc == 0 and expf.tag_stats == totals[True] and (tmp_path / "files.sam").read_bytes() == (tmp_path / "tagged1.sam").read_bytes()
    assert (tmp_path / "files" / "quant.sf").read_bytes() == quant
    rc, _ = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "sorted"), sopt(), write_mappings=str(tmp_path / "tagged.bam"),
                                     mappings_format="bam", mappings_sorted=True, mappings_tags=True, mappings_gapped=True, **kw)
    assert rc == 0
    got = (tmp_path / "tagged.bam").read_bytes()
    assert gzip.decompress(got) == samfile.sort_bam_stream(samfile.sam_to_bam(want))
    assert (tmp_path / "tagged.bam.bai").read_bytes() == samfile.build_bai(got)
    # the tagged file read back: the readers ignore the optional fields, the estimates are those of the untagged file
    for name in ("plain", "tagged0"):
        rc, _ = sf.quant.quantify_sam(str(tmp_path / (name + ".sam")), "U", str(tmp_path / (name + "_back")), sf.SailfishOpts(), device=gpu, cmd_options={"libType": "U"})
        assert rc == 0
    assert (tmp_path / "tagged0_back" / "quant.sf").read_bytes() == (tmp_path / "plain_back" / "quant.sf").read_bytes()
    for bad in (dict(), dict(write_mappings=str(tmp_path / "x.sam")), dict(mappings_oriented=True)):
        with pytest.raises(ValueError, match="mappings_tags"):
            sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "bad"), mappings_tags=True, device=gpu, **bad)
    assert not (tmp_path / "x.sam").exists()
