"""The posterior pass on the device (csrc/posterior.hip: sfgpu_hits_posteriors; hits.posteriors) against the Python statement
hits.posteriors_host: bit for bit over the shared corpus (tests/posterior_corpus.py), and the contract's shapes and errors through the
raw entry; the device writers with the posteriors handed in (samfile.SamDeviceWriter.write(posteriors=): "sam", "sam.gz", "bam" and
the sorted "bam" with its index) against the host statements samfile._sam_text(posteriors=), sam_to_bam and sort_bam_stream, with a
tile edge on every byte of the ZW field; and mappings_posteriors= of mapper.quantify_reads / quantify_files end to end."""
import ctypes as C
import gzip
import io
import re

import numpy as np
import pytest

import posterior_corpus as corpus
from test_gpu_aligng import _aln_device, _device, _reads
from test_gpu_mdtag import _tags_device

pytestmark = pytest.mark.gpu
ZW = re.compile(rb"\tZW:f:([^\t\n]*)")


def _bits(a, dt):
    return np.ascontiguousarray(a).view(dt)


def _bai_shape(bai):
    """what of an index does not depend on the records' bytes: per reference its bins and the length of its linear index, and the
    count of records without a coordinate (the virtual offsets move with the seven bytes a record gains)"""
    from sailfish_amd import samfile
    refs, no_coor = samfile.read_bai(bai)
    return [(sorted(bins), len(linear)) for bins, linear, _ in refs], no_coor


def _post_device(post, gpu):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(post[0], np.float64).copy()).to(gpu), torch.from_numpy(_bits(post[1], np.int32).copy()).to(gpu),
            torch.from_numpy(np.ascontiguousarray(post[2], np.float32).copy()).to(gpu))


def test_device_equals_the_statement(gpu):
    """the corpus's batch -- every size from 0 to 1000 records, interleaved so that a block meets every width class, and the rule's
    special reads: p as uint64 bits, the tokens rendered from rec, f32 as uint32 bits and every counter are the statement's"""
    import torch
    from sailfish_amd import hits as H
    h, o, _, _ = corpus.batch()
    want_p, want_rec, want_f32, want_st = corpus.expected()
    d_hits, d_off = _device(dict(hits=h, off=o), gpu)
    w = torch.from_numpy(corpus.weights().copy()).to(gpu)
    p, rec, f32, st = H.posteriors(d_hits, d_off, w)
    p, rec, f32 = p.cpu().numpy(), rec.cpu().numpy().view(np.uint32), f32.cpu().numpy()
    assert np.array_equal(_bits(p, np.uint64), _bits(want_p, np.uint64))
    assert np.array_equal(rec, want_rec) and [H.posterior_token(v) for v in rec] == corpus.tokens(want_p)
    assert np.array_equal(_bits(f32, np.uint32), _bits(want_f32, np.uint32))
    assert st == want_st
    # host arrays and a weight list go the same way
    again = H.posteriors(h, o, corpus.weights().tolist(), device=gpu)
    assert torch.equal(again[0].cpu(), torch.from_numpy(p)) and again[3] == want_st


def _raw(gpu, d_hits, d_off, n_reads, w, n_refs, p, rec, f32, stats=True):
    """sfgpu_hits_posteriors itself -> (rc, stats)"""
    import torch
    from sailfish_amd import _lib
    st = _lib.PosteriorStats()
    with torch.cuda.device(gpu):
        torch.cuda.synchronize()
        rc = _lib.lib().sfgpu_hits_posteriors(_lib.ptr(d_hits), _lib.ptr(d_off), n_reads, _lib.ptr(w), n_refs, _lib.ptr(p), _lib.ptr(rec), _lib.ptr(f32),
                                              C.byref(st) if stats else None, _lib.current_stream_ptr())
        torch.cuda.synchronize()
    return rc, st.as_dict()


def test_shapes_and_errors_of_the_contract(gpu):
    """n_reads == 0 and a batch without records are valid calls; the lowest record whose tid is no transcript: SFGPU_ERR_RANGE; the
    lowest weight that is negative, NaN, infinite or above 2^960: SFGPU_ERR_INVALID, and before the records; NULL pointers:
    SFGPU_ERR_INVALID; after every error the outputs are untouched"""
    import torch
    from sailfish_amd import _lib
    from sailfish_amd import hits as H
    h, o, _, _ = corpus.batch()
    want = corpus.expected()
    d_hits, d_off = _device(dict(hits=h, off=o), gpu)
    w = torch.from_numpy(corpus.weights().copy()).to(gpu)
    R, n, M = len(o) - 1, len(h), corpus.N_REFS
    zero = dict.fromkeys(H.POSTERIOR_STATS, 0)
    fresh = lambda: [torch.full((n * k,), 0x5A, dtype=torch.uint8, device=gpu) for k in (8, 4, 4)]
    untouched = lambda ts: all(bool((t == 0x5A).all().item()) for t in ts)
    # no reads; reads without a record
    rc, st = _raw(gpu, None, None, 0, w, M, None, None, None)
    assert rc == 0 and st == zero
    rc, st = _raw(gpu, None, None, 0, None, 0, None, None, None)
    assert rc == 0 and st == zero
    none_o = torch.zeros(R + 1, dtype=torch.int32, device=gpu)
    outs = fresh()
    rc, st = _raw(gpu, None, none_o, R, w, M, *outs)
    assert rc == 0 and st == dict(zero, reads=R) and untouched(outs)
    p, rec, f32, st = H.posteriors(torch.zeros(0, dtype=torch.uint8, device=gpu), none_o, w)
    assert p.numel() == rec.numel() == f32.numel() == 0 and st == dict(zero, reads=R)
    # the whole thing, raw
    outs = fresh()
    rc, st = _raw(gpu, d_hits, d_off, R, w, M, *outs)
    assert rc == 0 and st == want[3]
    assert np.array_equal(outs[0].cpu().numpy().view(np.uint64), _bits(want[0], np.uint64)) and np.array_equal(outs[1].cpu().numpy().view(np.uint32), want[1])
    # tid >= n_refs
    bad = h.copy()
    bad["tid"][[900, 77, 5000]] = M
    bad_hits = torch.from_numpy(bad.view(np.uint8).reshape(-1).copy()).to(gpu)
    outs = fresh()
    rc, _ = _raw(gpu, bad_hits, d_off, R, w, M, *outs)
    assert rc == _lib.ERR_RANGE and b"record 77 " in _lib.lib().sfgpu_last_error() and untouched(outs)
    with pytest.raises(_lib.SfgpuError, match="record 77 "):
        H.posteriors(bad_hits, d_off, w)
    rc, _ = _raw(gpu, d_hits, d_off, R, w, 30, *outs)                       # a shorter table: the first record that names 30 or more
    first = int(np.nonzero(h["tid"] >= 30)[0][0])
    assert rc == _lib.ERR_RANGE and b"record %d " % first in _lib.lib().sfgpu_last_error() and untouched(outs)
    # a weight the rule refuses, one kind each: the lowest transcript, and before any record
    for value in (-1.0, float("nan"), float("inf"), 2.0 ** 961):
        wb = corpus.weights().copy()
        wb[[31, 12, 44]] = value
        rc, _ = _raw(gpu, bad_hits, d_off, R, torch.from_numpy(wb).to(gpu), M, *outs)
        assert rc == _lib.ERR_INVALID and b"transcript 12 " in _lib.lib().sfgpu_last_error() and untouched(outs), value
    wb = corpus.weights().copy()
    wb[5] = 2.0 ** 960                                                        # the largest weight the rule takes
    assert _raw(gpu, d_hits, d_off, R, torch.from_numpy(wb).to(gpu), M, *fresh())[0] == 0
    # null pointers
    full = dict(d_hits=d_hits, d_off=d_off, n_reads=R, w=w, n_refs=M, p=outs[0], rec=outs[1], f32=outs[2])
    for change in (dict(stats=False), dict(d_hits=None), dict(d_off=None), dict(w=None), dict(p=None), dict(rec=None), dict(f32=None)):
        rc, _ = _raw(gpu, **{**full, **change})
        assert rc == _lib.ERR_INVALID, change
    assert untouched(outs)


# ---- the writers take the posteriors -----------------------------------------------------------------------------------------------

def _written(case, gpu, fmt, *, aln=None, tags=None, post=None, quals=None, oriented=True, sort=None, read_names=None):
    """the case through a SamDeviceWriter in one batch -> (the file's bytes, the index's)"""
    import torch
    import aligng_corpus as AG
    from sailfish_amd import samfile
    names, ref_len, _ = AG.sam_inputs(case)
    paired = AG.is_paired(case)
    f, x = io.BytesIO(), io.BytesIO()
    w = samfile.SamDeviceWriter(f, names, ref_len, paired, format=fmt, oriented=oriented, sort=sort, index=x if sort else None)
    d_hits, d_off = _device(case, gpu)
    r1, r2 = _reads(case, gpu)
    kw = {}
    if aln is not None:
        kw["alignments"] = _aln_device(aln, gpu)
    if tags is not None:
        kw["tags"] = _tags_device(tags, gpu)
    if post is not None:
        kw["posteriors"] = _post_device(post, gpu)
    if quals is not None:
        flat = [None if q is None else torch.from_numpy(np.frombuffer(b"".join(q), np.uint8).copy()).to(gpu) for q in quals]
        kw["quals"] = tuple(flat) if paired else flat[0]
    w.write(d_hits, d_off, seqs=(r1, r2) if paired else r1, read_names=read_names, **kw)
    w.close()
    return f.getvalue(), x.getvalue()


def _host_text(case, *, aln=None, tags=None, post=None, quals=None, oriented=True, read_names=None):
    import aligng_corpus as AG
    from sailfish_amd import samfile
    names, ref_len, seqs = AG.sam_inputs(case)
    per_read = None
    if quals is not None:
        per_read = list(zip(*quals)) if AG.is_paired(case) else quals[0]
    return samfile._sam_text(names, ref_len, case["hits"], case["off"], read_names, seqs, oriented=oriented, alignments=aln, tags=tags,
                             posteriors=None if post is None else post[:1], quals=per_read)


def _options(name):
    """the option sets a case is written with: nothing else; oriented with qualities and tags; the gapped alignment and tags"""
    import aligng_corpus as AG
    case, aln, tags, post = corpus.writable(name)
    if aln is not None:
        return [dict(aln=aln, tags=tags)]
    q = (corpus.quals(case["r1"]), corpus.quals(case["r2"]) if AG.is_paired(case) else None)
    return [dict(oriented=False), dict(quals=q, tags=tags)]


@pytest.mark.parametrize("name", corpus.WRITER_CASES)
def test_writers_write_the_posteriors(gpu, name):
    """about 40 reads, single-end and paired: "sam", "sam.gz", "bam" and the sorted "bam" with its index are byte-equal (the compressed
    ones inflated) to _sam_text(posteriors=), sam_to_bam of it and sort_bam_stream of that, and the index is build_bai of the device's
    own file, with the bins of the file without the tag -- with no other option, with orientation, qualities and tags, and with a gapped alignment and tags"""
    from sailfish_amd import samfile
    case, _, _, post = corpus.writable(name)
    assert 30 <= len(case["r1"]) <= corpus.WRITER_READS and {len(t) for t in corpus.tokens(post[0])} >= {1, 3, 8, 11}
    for kw in _options(name):
        text = _host_text(case, post=post, **kw)
        assert text.count(b"\tZW:f:") == sum(2 if s == 3 else 1 for s in case["hits"]["mate_status"].tolist()) > 0
        bam = samfile.sam_to_bam(text)
        assert _written(case, gpu, "sam", post=post, **kw)[0] == text, kw.keys()
        assert gzip.decompress(_written(case, gpu, "sam.gz", post=post, **kw)[0]) == text, kw.keys()
        assert gzip.decompress(_written(case, gpu, "bam", post=post, **kw)[0]) == bam, kw.keys()
        got, bai = _written(case, gpu, "bam", post=post, sort="coordinate", **kw)
        assert gzip.decompress(got) == samfile.sort_bam_stream(bam), kw.keys()
        assert bai == samfile.build_bai(got) and _bai_shape(bai) == _bai_shape(_written(case, gpu, "bam", sort="coordinate", **kw)[1])


@pytest.mark.parametrize("token", corpus.TOKENS_AT_THE_EDGE)
def test_a_tile_edge_on_every_byte_of_the_zw_field(gpu, token):
    """the tagged batch whose first QNAME is 1 .. 64 bytes long, so that the 4 096-byte tile edges move a byte a step through the
    lines' ZW fields (tests/test_posterior_cpu.py shows that they meet every offset), with tokens of 1, 8 and 11 bytes: text and BAM
    records equal the statement for every length"""
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    for n in range(1, 65):
        case, names, p = corpus.qnames_case(n, token)
        tags = H.md_tags_host(case["seqs"], case["hits"], case["off"], case["r1"], None)[:3]
        post = (p, np.array([H.posterior_record(v) for v in p], np.uint32), np.array([float(token)] * len(p), np.float32))
        text = _host_text(case, tags=tags, post=post, read_names=names)
        assert _written(case, gpu, "sam", tags=tags, post=post, read_names=names)[0] == text, n
        assert gzip.decompress(_written(case, gpu, "bam", tags=tags, post=post, read_names=names)[0]) == samfile.sam_to_bam(text), n


def test_what_the_writer_refuses_with_posteriors(gpu):
    """posteriors of another batch, or not what hits.posteriors returns: ValueError / TypeError; the raw entry with one of the two
    pointers, and every entry with a NULL batch: SFGPU_ERR_INVALID"""
    import torch
    import aligng_corpus as AG
    from sailfish_amd import _lib, gzfile
    from sailfish_amd import samfile
    case, _, _, post = corpus.writable("runs_se")
    names, ref_len, _ = AG.sam_inputs(case)
    d_hits, d_off = _device(case, gpu)
    r1, _ = _reads(case, gpu)
    d_post = _post_device(post, gpu)
    w = samfile.SamDeviceWriter(io.BytesIO(), names, ref_len, False)
    with pytest.raises(ValueError, match="posteriors of"):
        w.write(d_hits, d_off, seqs=r1, posteriors=tuple(t[:-1] for t in d_post))
    with pytest.raises(TypeError, match="posteriors"):
        w.write(d_hits, d_off, seqs=r1, posteriors=(d_post[0], d_post[0], d_post[2]))
    with pytest.raises(TypeError, match="posteriors"):
        w.write(d_hits, d_off, seqs=r1, posteriors=d_post[:1])
    batch, keep = w._batch_args(d_hits, d_off, None, r1, None, None)
    sink = _lib.TEXT_SINK(lambda addr, nb, user: 0)
    res = _lib.SamWriteResult()
    L = _lib.lib()
    for part in ((_lib.ptr(d_post[1]), None), (None, _lib.ptr(d_post[2]))):
        batch.tag_zw_rec, batch.tag_zw_f32 = part
        rc = L.sfgpu_sam_write_text(C.byref(batch), w.chunk_bytes, sink, None, C.byref(res), _lib.current_stream_ptr())
        assert rc == _lib.ERR_INVALID and b"posteriors" in L.sfgpu_last_error()
    w.close()
    z = gzfile.BgzfDeviceWriter(io.BytesIO())
    z._open(torch.device(gpu))
    assert L.sfgpu_sam_write_bgzf(None, 0, z._h, 1, C.byref(res), _lib.current_stream_ptr()) == _lib.ERR_INVALID and b"batch" in L.sfgpu_last_error()
    z.close()
    b = C.c_void_p()
    _lib.check(L.sfgpu_bamsort_open(C.byref(b)))
    assert L.sfgpu_bamsort_collect(b, None, C.byref(res), _lib.current_stream_ptr()) == _lib.ERR_INVALID and b"batch" in L.sfgpu_last_error()
    _lib.check(L.sfgpu_bamsort_close(b))


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def _lines_of(h):
    return [2 if s == 3 else 1 for s in h["mate_status"].tolist()]


def _sum_stats(total, st):
    for key, v in st.items():
        total[key] = max(total[key], v) if key == "max_records" else total[key] + v


def _statement_over_the_batches(idx, r1, r2, weights, batch, names, ref_len, read_names=None, quals=None, **map_kw):
    """the mappings file's expected body, with and without ZW, from the device's own records batch by batch and the host statements:
    -> (body with posteriors, body without, the tokens in record order, lines per record, summed stats, (p, weights) per read)"""
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    tagged = bool(map_kw.pop("tags", False))
    head = len(samfile.sam_header(names, ref_len))
    with_zw, without, toks, lines, per_read = [], [], [], [], []
    total = dict.fromkeys(H.POSTERIOR_STATS, 0)
    for a in range(0, len(r1), batch):
        p1, p2 = r1[a:a + batch], r2[a:a + batch]
        h, o = sf.mapper.hits_to_numpy(*idx.map_reads(p1, p2, tags=tagged, **map_kw))
        aln = None
        if getattr(idx, "last_alignments", None) is not None and map_kw.get("validate", {}).get("align"):
            aln = tuple(t.cpu().numpy() for t in idx.last_alignments)
            aln = (aln[0], aln[1].view(np.uint32), aln[2].view(np.uint64), aln[3].view(np.uint32))
        tags = None
        if tagged:
            t = tuple(t.cpu().numpy() for t in idx.last_tags)
            tags = (t[0].view(np.uint32), t[1].view(np.uint64), t[2])
        p, _, _, st = H.posteriors_host(h, o, weights)
        _sum_stats(total, st)
        qn = [b"r%d" % (a + i) for i in range(len(p1))] if read_names is None else read_names[a:a + batch]
        kw = dict(oriented=tagged, alignments=aln, tags=tags, quals=None if quals is None else quals[a:a + batch])
        with_zw.append(samfile._sam_text(names, ref_len, h, o, qn, list(zip(p1, p2)), posteriors=(p,), **kw)[head:])
        without.append(samfile._sam_text(names, ref_len, h, o, qn, list(zip(p1, p2)), **kw)[head:])
        toks += corpus.tokens(p); lines += _lines_of(h)
        x = np.asarray(weights)[h["tid"].astype(np.int64)]
        per_read += [(p[o[r]:o[r + 1]], x[o[r]:o[r + 1]]) for r in range(len(o) - 1)]
    return b"".join(with_zw), b"".join(without), toks, lines, total, per_read


def test_quantify_reads_writes_posteriors(gpu, tmp_path):
    """quantify_reads(mappings_posteriors=True), paired, 600 reads over ten genes of four isoforms in three batches that pass twice:
    quant.sf is the one of the run without the option; the mappings file without its ZW fields is that run's file; the tokens in file
    order are posteriors_host over map_reads of the same reads under the weights the experiment holds; the values of a read sum to 1
    within six digits' worth a record; posterior_stats is the statement's and one log line names it.  Once more with rescue,
    validation, gapped alignments, tags and a sorted BAM, as BAM streams."""
    import sailfish_amd as sf
    from sailfish_amd import samfile
    names, seqs, r1, r2 = corpus.end_to_end()
    batch = corpus.E2E_BATCH
    log = []
    sopt = lambda: sf.SailfishOpts(jointLog=lambda lvl, msg: log.append(msg))
    base = dict(batch_reads=batch, device=gpu, cmd_options={"libType": "IU"})
    rc, exp0 = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "plain"), sopt(), write_mappings=str(tmp_path / "plain.sam"), **base)
    assert rc == 0 and exp0.posterior_stats is None and not [m for m in log if m.startswith("posteriors")]
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "post"), sopt(), write_mappings=str(tmp_path / "post.sam"),
                                       mappings_posteriors=True, **base)
    assert rc == 0
    assert (tmp_path / "post" / "quant.sf").read_bytes() == (tmp_path / "plain" / "quant.sf").read_bytes()
    got, plain = (tmp_path / "post.sam").read_bytes(), (tmp_path / "plain.sam").read_bytes()
    assert ZW.sub(b"", got) == plain and got != plain
    weights = exp.posterior_weights.cpu().numpy()
    est, eff = exp.transcripts().estCount.cpu().numpy(), exp.transcripts().EffectiveLength.cpu().numpy()
    ref = np.where(eff > 0, est / np.where(eff > 0, eff, 1.0), 0.0)             # NumReads / EffectiveLength, to the last bits of a division
    assert np.array_equal(weights > 0, ref > 0) and np.allclose(weights, ref, rtol=1e-15, atol=0) and (weights > 0).sum() > 10
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)
    want, want_plain, toks, lines, total, per_read = _statement_over_the_batches(idx, r1, r2, weights, batch, names, ref_len)
    head = samfile.sam_header(names, ref_len)
    assert plain == head + want_plain and got == head + want
    assert [m.decode() for m in ZW.findall(got)] == [t for t, n in zip(toks, lines) for _ in range(n)]
    assert exp.posterior_stats == total and total["reads_multi"] > 300 and total["records"] == len(toks)
    line = [m for m in log if m.startswith("posteriors in the mappings file")]
    assert len(line) == 1 and f"on the {total['records']} records of {total['reads_mapped']} mapped reads, {total['reads_multi']} of them" in line[0]
    # per read the written values sum to 1: six digits' worth a record.  Reads with a flushed record -- a weight above 0 whose value
    # is written as 0 -- are left out, and by the statement those are few (a record whose weight IS 0 loses nothing)
    flushed = {b"r%d" % r for r, (p, x) in enumerate(per_read) if ((p == 0) & (x > 0)).any()}
    assert len(flushed) < 0.05 * len(r1)
    sums = {}
    for l in got[len(head):].split(b"\n")[:-1]:
        f = l.split(b"\t")
        if int(f[1]) & 4 or (int(f[1]) & 0x82) == 0x82:                  # (a pair's second line repeats its record's value)
            continue
        sums.setdefault(f[0], []).append(float(ZW.search(l).group(1)))
    assert len(sums) == total["reads_mapped"] and sum(len(vs) for vs in sums.values()) == total["records"]
    for q, vs in sums.items():
        if q not in flushed:
            assert abs(sum(vs) - 1.0) <= len(vs) * 5e-7, (q, vs)
    # rescue, validation, gapped alignments, tags and a sorted BAM: the streams
    opts = dict(rescue_mates=True, validate_mappings=True, max_indel=3, mappings_gapped=True, mappings_tags=True, mappings_oriented=True, mappings_sorted=True,
                mappings_format="bam")
    del log[:]
    rc, exp0 = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "plain2"), sopt(), write_mappings=str(tmp_path / "plain2.bam"), **opts, **base)
    assert rc == 0
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "post2"), sopt(), write_mappings=str(tmp_path / "post2.bam"),
                                       mappings_posteriors=True, **opts, **base)
    assert rc == 0 and (tmp_path / "post2" / "quant.sf").read_bytes() == (tmp_path / "plain2" / "quant.sf").read_bytes()
    assert exp.rescue_stats == exp0.rescue_stats and exp.verify_stats == exp0.verify_stats and exp.align_stats == exp0.align_stats and exp.tag_stats == exp0.tag_stats
    assert exp.rescue_stats["reads_rescued"] > 0
    weights = exp.posterior_weights.cpu().numpy()
    want, want_plain, toks, lines, total, _ = _statement_over_the_batches(
        idx, r1, r2, weights, batch, names, ref_len, tags=True, validate=dict(min_identity=0.9, keep_best=False, max_indel=3, align=True),
        rescue=dict(min_identity=0.9, window=sf.SailfishOpts().maxFragLen))
    idx.close()
    head = samfile.sam_header(names, ref_len, "coordinate")
    assert gzip.decompress((tmp_path / "plain2.bam").read_bytes()) == samfile.sort_bam_stream(samfile.sam_to_bam(head + want_plain))
    got = (tmp_path / "post2.bam").read_bytes()
    assert gzip.decompress(got) == samfile.sort_bam_stream(samfile.sam_to_bam(head + want))
    assert (tmp_path / "post2.bam.bai").read_bytes() == samfile.build_bai(got)
    assert _bai_shape((tmp_path / "post2.bam.bai").read_bytes()) == _bai_shape((tmp_path / "plain2.bam.bai").read_bytes())
    assert exp.posterior_stats == total and len(ZW.findall(want)) == sum(lines)


def test_quantify_files_writes_posteriors(gpu, tmp_path):
    """quantify_files(mappings_posteriors=True) from FASTQ files, mate 2 gzipped, with the unmapped reads written too: quant.sf and
    the unmapped files are those of the run without the option, the mappings file without its ZW fields is that run's file, and the
    tokens are the statement's over the same reads"""
    import sailfish_amd as sf
    from sailfish_amd import samfile
    names, seqs, r1, r2 = corpus.end_to_end()
    batch = corpus.E2E_BATCH
    junk = [b"ACGT" * 12 + b"TTGACCA" * 2] * 3                               # three pairs that map nowhere
    r1, r2 = list(r1) + junk, list(r2) + junk
    q1, q2 = corpus.quals(r1), corpus.quals(r2)
    (tmp_path / "tx.fa").write_bytes(b"".join(b">%s\n%s\n" % (n.encode(), s) for n, s in zip(names, seqs)))
    (tmp_path / "m1.fq").write_bytes(b"".join(b"@read%d/1\n%s\n+\n%s\n" % (i, r, q) for i, (r, q) in enumerate(zip(r1, q1))))
    (tmp_path / "m2.fq.gz").write_bytes(gzip.compress(b"".join(b"@read%d/2\n%s\n+\n%s\n" % (i, r, q) for i, (r, q) in enumerate(zip(r2, q2)))))
    out = {}
    for key, kw in (("plain", {}), ("post", dict(mappings_posteriors=True))):
        unm = (str(tmp_path / (key + "_u1.fq")), str(tmp_path / (key + "_u2.fq")))
        rc, exp = sf.mapper.quantify_files(str(tmp_path / "tx.fa"), str(tmp_path / "m1.fq"), str(tmp_path / "m2.fq.gz"), "IU", str(tmp_path / key), sf.SailfishOpts(),
                                           write_mappings=str(tmp_path / (key + ".sam")), write_unmapped=unm, check_mate_names=True, batch_reads=batch, device=gpu,
                                           cmd_options={"libType": "IU"}, **kw)
        assert rc == 0
        out[key] = (exp, (tmp_path / key / "quant.sf").read_bytes(), (tmp_path / (key + ".sam")).read_bytes(), [open(u, "rb").read() for u in unm])
    exp, quant, got, unmapped = out["post"]
    assert quant == out["plain"][1] and unmapped == out["plain"][3] and unmapped[0].count(b"\n") >= 12
    assert ZW.sub(b"", got) == out["plain"][2] and exp.unmapped_stats == out["plain"][0].unmapped_stats
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)
    qn = [b"read%d/1" % i for i in range(len(r1))]
    want, _, toks, lines, total, _ = _statement_over_the_batches(idx, r1, r2, exp.posterior_weights.cpu().numpy(), batch, names, ref_len, read_names=qn)
    idx.close()
    assert got == samfile.sam_header(names, ref_len) + want and exp.posterior_stats == total and total["reads"] == len(r1)


def test_no_mappings_file_where_the_quantification_fails(gpu, tmp_path):
    """Gibbs samples and bootstraps both asked for: quantify returns non-zero, the second pass does not run, no mappings file appears
    and the log says so"""
    import sailfish_amd as sf
    names, seqs, r1, r2 = corpus.end_to_end()
    log = []
    sopt = sf.SailfishOpts(numGibbsSamples=2, numBootstraps=2, jointLog=lambda lvl, msg: log.append(msg))
    path = tmp_path / "never.sam"
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1[:50], r2[:50], "IU", str(tmp_path / "out"), sopt, write_mappings=str(path), mappings_posteriors=True,
                                       device=gpu, cmd_options={"libType": "IU"})
    assert rc != 0 and exp is None and not path.exists()
    assert [m for m in log if "no mappings file is written" in m]
