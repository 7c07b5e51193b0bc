"""Qualities and orientation in the device SAM / BAM writer (sfgpu_sam_write_text, sfgpu_sam_write_bgzf;
sailfish_amd/csrc/samtext_write.hip; samfile.SamDeviceWriter(oriented=).write(quals=); mappings_oriented= of mapper.quantify_files /
quantify_reads).  The expected bytes are always the host statement's -- samfile._sam_text(..., quals=, oriented=), sam_to_bam of it
for BAM -- which tests/test_samqual_cpu.py judges on its own; without qualities and orientation they are also what a batch
without those fields writes."""
import ctypes as C
import gzip
import io
import os

import numpy as np
import pytest
import torch

import bamwrite_corpus as bw
import samqual_corpus as corpus
import samwrite_corpus as sw
from test_gpu_samwrite import _batches, _device_seqs, _first_difference, _greedy_chunks, _sample, _t, _unit_lengths

pytestmark = pytest.mark.gpu


def _call(case, gpu, quals, oriented, *, fmt=None, old=False, chunk_bytes=0, base=0, null_sink=False):
    """one C call over the case's arrays -> (status, result dict, chunks, inflated bytes or None).  fmt None: the text entry with a
    sink that keeps every chunk; "sam.gz" / "bam": the BGZF entry into an encoder of its own.  old: the batch without its quality
    fields (quals and oriented must then be off)."""
    from sailfish_amd import _lib, gzfile
    L = _lib.lib()
    d = {k: _t(v, gpu) for k, v in corpus.arrays(case).items()}
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    batch = _lib.SamwBatch(p(d["hits"]), _lib.ptr(d["offsets"]), d["offsets"].numel() - 1, int(case["paired"]), p(d["ref"]), _lib.ptr(d["ref_off"]),
                           len(case["names"]), p(d["q"]), p(d["q_off"]), p(d["s1"]), p(d["s1_off"]), p(d["s2"]), p(d["s2_off"]), base)
    assert not (old and (quals or oriented))
    if not old:
        batch.qual1, batch.qual2, batch.oriented = p(d["k1"]) if quals else None, p(d["k2"]) if quals else None, int(oriented)
    chunks = []

    def sink(addr, n, _user):
        chunks.append(C.string_at(addr, n))
        return 0

    res = _lib.SamWriteResult()
    with torch.cuda.device(gpu):
        if fmt is None:
            rc = L.sfgpu_sam_write_text(C.byref(batch), chunk_bytes, _lib.TEXT_SINK(0) if null_sink else _lib.TEXT_SINK(sink), None, C.byref(res),
                                        _lib.current_stream_ptr())
            return rc, res.as_dict(), chunks, None
        out = io.BytesIO()
        z = gzfile.BgzfDeviceWriter(out)
        z._open(torch.device(gpu))
        rc = L.sfgpu_sam_write_bgzf(C.byref(batch), chunk_bytes, z._h, 1 if fmt == "bam" else 0, C.byref(res), _lib.current_stream_ptr())
        z.close()
    return rc, res.as_dict(), chunks, gzip.decompress(out.getvalue())


def _records(case, text_with_header):
    """sam_to_bam of the text, from the first record on"""
    from sailfish_amd import samfile
    head = samfile.sam_to_bam(samfile.sam_header(case["names"], case["ref_len"]))
    data = samfile.sam_to_bam(text_with_header)
    assert data.startswith(head)
    return data[len(head):]


@pytest.fixture(scope="module")
def text_corpora():
    """per library: [(name, case, base, {mode: expected lines})], computed once"""
    out = {}
    for paired in (True, False):
        cases = [("corner", corpus.dress(sw.corner(paired), 1), 4_294_967_000), ("runs", corpus.reversed_runs(paired), 0)]
        if paired:
            cases += [("mate1", corpus.only(cases[1][1], 0), 0), ("mate2", corpus.only(cases[1][1], 1), 0)]
        out[paired] = [(name, dict(c, read_names=None) if base else c, base, {m: corpus.expected(dict(c, read_names=None) if base else c, *m, base) for m in corpus.MODES})
                       for name, c, base in cases]
    return out


@pytest.fixture(scope="module")
def bam_corpora():
    out = {}
    names, ref_len = bw._transcripts()
    for paired in (True, False):
        cases = [("corner", corpus.dress(bw.corner(paired, (9000, 5000)), 4)), ("runs", corpus.reversed_runs(paired, names, ref_len))]
        if paired:
            cases += [("mate2", corpus.only(cases[1][1], 1))]
        out[paired] = [(name, c, {m: corpus.expected(c, *m, header=True) for m in corpus.MODES}) for name, c in cases]
    return out


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_text_is_the_host_statement_at_every_chunk_size(gpu, text_corpora, paired):
    for name, case, base, wants in text_corpora[paired]:
        assert len(set(wants.values())) == 4
        for (quals, oriented), want in wants.items():
            unit_len = _unit_lengths(case, want)
            longest = int(unit_len.max())
            for chunk_bytes in (0, max(longest, len(want) // 6), longest + 1):
                rc, res, chunks, _ = _call(case, gpu, quals, oriented, chunk_bytes=chunk_bytes, base=base)
                got = b"".join(chunks)
                assert rc == 0 and got == want, (name, quals, oriented, chunk_bytes, _first_difference(got, want))
                assert (res["n_bytes"], res["n_lines"], res["max_unit_bytes"]) == (len(want), want.count(b"\n"), longest)
                assert res["n_chunks"] == len(chunks) == _greedy_chunks(unit_len, chunk_bytes or (32 << 20))
        # neither: the bytes of the entry without the arguments
        rc, _, chunks, _ = _call(case, gpu, False, False, old=True, base=base)
        assert rc == 0 and b"".join(chunks) == wants[(False, False)]


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_bgzf_text_and_bam_inflate_to_the_host_statement(gpu, text_corpora, bam_corpora, paired):
    for name, case, base, wants in text_corpora[paired]:
        if name not in ("corner", "runs"):
            continue
        for (quals, oriented), want in wants.items():
            longest = int(_unit_lengths(case, want).max())
            for chunk_bytes in (0, max(longest, len(want) // 6), longest + 1):
                rc, res, _, got = _call(case, gpu, quals, oriented, fmt="sam.gz", chunk_bytes=chunk_bytes, base=base)
                assert rc == 0 and got == want, (name, quals, oriented, chunk_bytes, _first_difference(got, want))
        rc, _, _, got = _call(case, gpu, False, False, fmt="sam.gz", old=True, base=base)
        assert rc == 0 and got == wants[(False, False)]
    for name, case, texts in bam_corpora[paired]:
        wants = {m: _records(case, t) for m, t in texts.items()}
        assert len(set(wants.values())) == 4
        for (quals, oriented), want in wants.items():
            rc, res, _, got = _call(case, gpu, quals, oriented, fmt="bam", null_sink=True)
            assert rc == 0
            longest = res["max_unit_bytes"]
            for chunk_bytes in (0, max(longest, len(want) // 6), longest + 1):
                rc, res, _, got = _call(case, gpu, quals, oriented, fmt="bam", chunk_bytes=chunk_bytes)
                assert rc == 0 and got == want, (name, quals, oriented, chunk_bytes, _first_difference(got, want))
                assert res["n_bytes"] == len(want) and res["n_lines"] == texts[(quals, oriented)].count(b"\n") - texts[(quals, oriented)].count(b"\n@") - 1
        rc, _, _, got = _call(case, gpu, False, False, fmt="bam", old=True)
        assert rc == 0 and got == wants[(False, False)]


def _dense(piece, n_bases, tid):
    """64 single-end reads, each with a name of `piece` bytes, n_bases bases and qualities and one record on the reverse strand of
    transcript tid (whose name has `piece` bytes too)"""
    rng = np.random.default_rng(piece)
    assert len(sw.NAMES[tid]) == piece
    reads = [((b"dense%02d" % i).ljust(piece, b"q"), corpus._bases(rng, n_bases), [sw.rec(tid, 3, 0, 0, n_bases, 0, 0, 0, 0)]) for i in range(64)]
    case = dict(sw._case(False, reads), names=sw.NAMES, ref_len=sw.REF_LEN)
    return dict(case, quals=[corpus._quals(rng, n_bases) for _ in reads])


def test_the_job_queue_at_its_densest(gpu):
    """Every run of every line is one byte longer than what a lane copies itself (49 = kShortCopy + 1), so every name, SEQ and QUAL is
    queued: four jobs per line of about 225 bytes in the text, as many per tile as the line grammar allows; a job that was dropped
    would leave zeros in the tile.  In BAM 97 bases pack into 49 bytes.  With 48-byte pieces nothing is queued at all."""
    text, packed, short = _dense(49, 49, 4), _dense(49, 97, 4), _dense(48, 48, 3)
    for oriented in (False, True):
        want = corpus.expected(text, True, oriented)
        assert 3 * 4096 < len(want) <= 4 * 4096 and want.count(b"\n") == 64
        rc, res, chunks, _ = _call(text, gpu, True, oriented)
        got = b"".join(chunks)
        assert rc == 0 and got == want, (oriented, _first_difference(got, want))
        want = _records(packed, corpus.expected(packed, True, oriented, header=True))
        rc, res, _, got = _call(packed, gpu, True, oriented, fmt="bam")
        assert rc == 0 and got == want, (oriented, _first_difference(got, want))
        want = corpus.expected(short, True, oriented)
        rc, res, chunks, _ = _call(short, gpu, True, oriented)
        got = b"".join(chunks)
        assert rc == 0 and got == want, (oriented, _first_difference(got, want))
    assert corpus.expected(text, True, True) != corpus.expected(text, True, False)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_quality_bytes_that_cannot_be_written(gpu, paired):
    from sailfish_amd import _lib, samfile
    for case, read, record, kind in corpus.failing(paired):
        for fmt in (None, "sam.gz", "bam"):
            for null_sink in ((False, True) if fmt is None else (False,)):
                rc, res, chunks, got = _call(case, gpu, True, True, fmt=fmt, null_sink=null_sink)
                assert rc == _lib.ERR_INVALID and not chunks and not got
                assert (res["error_kind"], res["error_read"], res["error_record"]) == (kind, read, record)
    # qualities of a mate whose bases are not given
    case = corpus.reversed_runs(paired)
    d = {k: _t(v, gpu) for k, v in corpus.arrays(case).items()}
    res = _lib.SamWriteResult()
    with torch.cuda.device(gpu):
        batch = _lib.SamwBatch(_lib.ptr(d["hits"]), _lib.ptr(d["offsets"]), d["offsets"].numel() - 1, int(paired), _lib.ptr(d["ref"]),
                               _lib.ptr(d["ref_off"]), len(case["names"]), qual1=_lib.ptr(d["k1"]), oriented=1)
        rc = _lib.lib().sfgpu_sam_write_text(C.byref(batch), 0, _lib.TEXT_SINK(0), None, C.byref(res), _lib.current_stream_ptr())
    assert rc == _lib.ERR_INVALID
    # the writer names the read counted over the batches
    bad, read, record, kind = corpus.failing(paired)[0]
    assert kind == 6
    w = samfile.SamDeviceWriter(io.BytesIO(), bad["names"], bad["ref_len"], paired, oriented=True)
    ok = corpus.dress(sw.random_case(3, paired, n_reads=20), 6)
    for c, raises in ((ok, False), (bad, True)):
        h, o, q, s = next(_batches(c, [0, len(c["offsets"]) - 1]))
        args, kw = (_t(h.view(np.uint8).reshape(-1), gpu), _t(o, gpu)), dict(read_names=q, seqs=_device_seqs(s, paired, gpu), quals=_device_quals(c, gpu))
        if raises:
            with pytest.raises(ValueError) as e:
                w.write(*args, **kw)
            assert str(e.value) == f"read {20 + read}, record {record}: {samfile.QUAL_WRITE_KINDS[6]}"
        else:
            w.write(*args, **kw)
    w.close()


def _device_quals(case, gpu):
    a = corpus.arrays(case)
    return (_t(a["k1"], gpu), _t(a["k2"], gpu)) if case["paired"] else _t(a["k1"], gpu)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_writer_files_read_back(gpu, tmp_path, paired):
    """SamDeviceWriter(oriented=True).write(quals=) in three batches, all three formats: the file is the host statement's, and read
    back through samfile.SamFile it gives the batch's hit records -- orientation does not change what is quantified"""
    from sailfish_amd import samfile
    names, ref_len = bw._transcripts()
    names = [n.decode() for n in names]
    case = corpus.dress(bw.case(paired, n_reads=300, seed=3), 8)
    n = len(case["offsets"]) - 1
    text = samfile._sam_text(names, ref_len, case["hits"], case["offsets"], case["read_names"], case["seqs"], quals=case["quals"], oriented=True)
    plain = samfile._sam_text(names, ref_len, case["hits"], case["offsets"], case["read_names"], case["seqs"])
    assert text != plain
    want_hits, want_off = samfile.read_sam_host(plain, names, paired)
    for fmt in samfile.WRITE_FORMATS:
        path = tmp_path / f"out.{fmt}"
        with samfile.SamDeviceWriter(str(path), names, ref_len, paired, chunk_bytes=50000, format=fmt, oriented=True) as w:
            for a, b in ((0, 97), (97, 98), (98, n)):
                sub = dict(case, hits=case["hits"][case["offsets"][a]:case["offsets"][b]], offsets=(case["offsets"][a:b + 1] - case["offsets"][a]).astype(np.uint32),
                           read_names=case["read_names"][a:b], seqs=case["seqs"][a:b], quals=case["quals"][a:b])
                w.write(_t(sub["hits"].view(np.uint8).reshape(-1), gpu), _t(sub["offsets"], gpu), read_names=sub["read_names"],
                        seqs=_device_seqs(sub["seqs"], paired, gpu), quals=_device_quals(sub, gpu))
        got = path.read_bytes() if fmt == "sam" else gzip.decompress(path.read_bytes())
        want = samfile.sam_to_bam(text) if fmt == "bam" else text
        assert got == want, (fmt, _first_difference(got, want))
        got_hits, got_off = [], [np.zeros(1, np.int64)]
        with samfile.SamFile(str(path), gpu, paired=paired, names=names, block_bytes=1 << 16) as f:
            for h, o in f:
                got_hits.append(h.cpu().numpy())
                got_off.append(o.cpu().numpy().view(np.uint32)[1:].astype(np.int64) + got_off[-1][-1])
        assert np.concatenate(got_hits).tobytes() == want_hits.tobytes() and np.array_equal(np.concatenate(got_off), want_off)


def _fastq(path, reads, quals, mate):
    path.write_bytes(b"".join(b"@frag.%d mate=%d\n" % (i, mate) + r + b"\n+\n" + q + b"\n" for i, (r, q) in enumerate(zip(reads, quals))))


@pytest.mark.parametrize("fmt", ["sam", "bam"])
def test_quantify_files_writes_oriented_mappings(gpu, tmp_path, fmt):
    """quant.sf does not depend on the option; undoing the orientation of the 0x10 lines recovers the FASTQ records"""
    import sailfish_amd as sf
    from sailfish_amd import samfile
    names, seqs, r1, r2 = _sample()
    n = 600
    rng = np.random.default_rng(5)
    quals = [[rng.choice(corpus.QUALS, len(r)).tobytes() for r in reads[:n]] for reads in (r1, r2)]
    fa = tmp_path / "transcripts.fasta"
    fa.write_bytes(b"".join(b">" + nm.encode() + b"\n" + s + b"\n" for nm, s in zip(names, seqs)))
    paths = [tmp_path / "reads_1.fastq", tmp_path / "reads_2.fastq"]
    for m, p in enumerate(paths):
        _fastq(p, (r1, r2)[m][:n], quals[m], m + 1)
    fopts = dict(batch_reads=250, cmd_options={"libType": "IU"}, device=gpu)
    rc, _ = sf.mapper.quantify_files(fa, *paths, "IU", str(tmp_path / "plain"), sf.SailfishOpts(numFragSamples=5000), **fopts)
    assert rc == 0
    out = tmp_path / f"mappings.{fmt}"
    rc, _ = sf.mapper.quantify_files(fa, *paths, "IU", str(tmp_path / "kept"), sf.SailfishOpts(numFragSamples=5000), write_mappings=str(out),
                                     mappings_format=fmt, mappings_oriented=True, **fopts)
    assert rc == 0 and (tmp_path / "kept" / "quant.sf").read_bytes() == (tmp_path / "plain" / "quant.sf").read_bytes()
    text = out.read_bytes() if fmt == "sam" else samfile.bam_to_sam(gzip.decompress(out.read_bytes()))
    lines = [l.split(b"\t") for l in text.splitlines() if not l.startswith(b"@")]
    primary = [f for f in lines if not int(f[1]) & 0x100]
    assert len(primary) >= n and any(int(f[1]) & 0x10 for f in primary) and any(not int(f[1]) & 0x10 for f in primary)
    seen = set()
    for f in primary:
        flag, i = int(f[1]), int(f[0][5:])
        m = 1 if flag & 0x80 else 0
        seq, qual = (f[9].translate(corpus.COMP)[::-1], f[10][::-1]) if flag & 0x10 else (f[9], f[10])
        assert (seq, qual) == ((r1, r2)[m][i], quals[m][i]), (i, m, flag)
        seen.add((i, m))
    assert {i for i, _ in seen} == set(range(n)) and len(seen) > n


def test_quantify_reads_takes_qualities(gpu, tmp_path):
    import sailfish_amd as sf
    from sailfish_amd import samfile
    names, seqs, r1, r2 = _sample()
    n = 500
    r1, r2 = r1[:n], r2[:n]
    rng = np.random.default_rng(6)
    q1, q2 = ([rng.choice(corpus.QUALS, len(r)).tobytes() for r in reads] for reads in (r1, r2))
    opts = dict(batch_reads=200, cmd_options={"libType": "IU"}, device=gpu)
    sam = tmp_path / "mappings.sam"
    rc, _ = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "kept"), sf.SailfishOpts(numFragSamples=5000), write_mappings=str(sam),
                                     quals1=q1, quals2=q2, mappings_oriented=True, **opts)
    assert rc == 0
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    hits, off = [], [np.zeros(1, np.int64)]
    for a in range(0, n, 200):
        h, o = sf.mapper.hits_to_numpy(*idx.map_reads(r1[a:a + 200], r2[a:a + 200]))
        hits.append(h)
        off.append(o[1:].astype(np.int64) + off[-1][-1])
    want = samfile._sam_text(names, idx.ref_len.cpu().numpy(), np.concatenate(hits), np.concatenate(off).astype(np.uint32), None, list(zip(r1, r2)),
                             quals=list(zip(q1, q2)), oriented=True)
    idx.close()
    got = sam.read_bytes()
    assert got == want, _first_difference(got, want)
