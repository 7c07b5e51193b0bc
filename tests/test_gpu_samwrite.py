"""The mapper's alignments written as SAM from the device (sfgpu_sam_write_text, sailfish_amd/csrc/samtext_write.hip with the
rules of csrc/samwfmt.h; samfile.SamDeviceWriter; write_mappings= of mapper.quantify_reads / quantify_files).  The expected bytes
are always samfile._sam_text's -- the per-record host loop -- over the host copy of the same batch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import samwrite_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
LONG = (9000, 5000)                                        # a line that spans three 4 KB tiles, one that spans two


def _t(a, gpu):
    if a is None:
        return None
    if a.dtype in (np.uint32, np.uint64):
        a = a.view(np.int32 if a.dtype == np.uint32 else np.int64)
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(gpu)


def _collect(case, gpu, chunk_bytes=0, base=0, refuse_at=None, null_sink=False, n_refs=None):
    """the C entry over the case's arrays with a sink that keeps every chunk -> (status, result dict, chunks)"""
    from sailfish_amd import _lib
    d = {k: _t(v, gpu) for k, v in corpus.arrays(case).items()}
    p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
    chunks = []

    def sink(addr, n, _user):
        chunks.append(C.string_at(addr, n))
        return 1 if refuse_at is not None and len(chunks) == refuse_at else 0

    res = _lib.SamWriteResult()
    batch = _lib.SamwBatch(p(d["hits"]), _lib.ptr(d["offsets"]), d["offsets"].numel() - 1, int(case["paired"]), p(d["ref"]), _lib.ptr(d["ref_off"]),
                           len(case["names"]) if n_refs is None else n_refs, p(d["q"]), p(d["q_off"]), p(d["s1"]), p(d["s1_off"]), p(d["s2"]),
                           p(d["s2_off"]), base)
    with torch.cuda.device(gpu):
        rc = _lib.lib().sfgpu_sam_write_text(C.byref(batch), chunk_bytes, _lib.TEXT_SINK(0) if null_sink else _lib.TEXT_SINK(sink), None, C.byref(res),
                                             _lib.current_stream_ptr())
    return rc, res.as_dict(), chunks


def _unit_lengths(case, text):
    """bytes of every unit of the text: a pair record and a record-less paired read own two lines, everything else one"""
    line_len = np.diff(np.concatenate([[0], np.flatnonzero(np.frombuffer(text, np.uint8) == ord("\n")) + 1]))
    per_read = np.diff(case["offsets"].astype(np.int64))
    lines = []
    for r, k in enumerate(per_read):
        st = case["hits"]["mate_status"][case["offsets"][r]:case["offsets"][r + 1]]
        lines += [2 if s == 3 else 1 for s in st] if k else [2 if case["paired"] else 1]
    assert sum(lines) == len(line_len)
    ends = np.cumsum(lines)
    return np.add.reduceat(line_len, np.concatenate([[0], ends[:-1]])) if len(lines) else np.zeros(0, np.int64)


def _greedy_chunks(unit_len, chunk_bytes):
    n, cur = 0, 0
    for L in unit_len:
        if cur and cur + L > chunk_bytes:
            n, cur = n + 1, 0
        cur += int(L)
    return n + (1 if cur else 0)


def _first_difference(got, want):
    n = min(len(got), len(want))
    d = np.flatnonzero(np.frombuffer(got, np.uint8, n) != np.frombuffer(want, np.uint8, n))
    i = int(d[0]) if len(d) else n
    lo = want.rfind(b"\n", 0, i) + 1
    return f"lengths {len(got)} / {len(want)}, first difference at byte {i}: got {got[lo:i + 60]!r}, want {want[lo:i + 60]!r}"


@pytest.fixture(scope="module")
def corpora():
    """per library: [(variant, base, expected text, unit lengths)] over the corner and the random corpus, computed once"""
    out = {}
    for paired in (True, False):
        rows = []
        for case, base in ((corpus.corner(paired, LONG), 0), (corpus.random_case(0, paired, long_seqs=LONG), 4_294_967_000)):
            for v in corpus.variants(case):
                want = corpus.expected(v, base)
                rows.append((v, base, want, _unit_lengths(v, want)))
        out[paired] = rows
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_text_is_sam_text_at_every_chunk_size(gpu, corpora, paired):
    for v, base, want, unit_len in corpora[paired]:
        longest = int(unit_len.max())
        if v["seqs"] is not None:
            assert longest > 9000
        ends = set(np.cumsum(unit_len).tolist())
        for chunk_bytes in (0, max(longest, len(want) // 6), longest + 1):
            rc, res, chunks = _collect(v, gpu, chunk_bytes, base)
            assert rc == 0
            got = b"".join(chunks)
            assert got == want, _first_difference(got, want)
            assert (res["n_bytes"], res["n_lines"], res["max_unit_bytes"]) == (len(want), want.count(b"\n"), longest)
            assert res["n_chunks"] == len(chunks) == _greedy_chunks(unit_len, chunk_bytes or (32 << 20))
            assert all(c.endswith(b"\n") and len(c) <= (chunk_bytes or (32 << 20)) for c in chunks)
            assert set(np.cumsum([len(c) for c in chunks]).tolist()) <= ends          # chunks end between units: no pair is split
            if chunk_bytes == max(longest, len(want) // 6):
                assert len(chunks) >= 4


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_contract(gpu, corpora, paired):
    from sailfish_amd import _lib
    v, base, want, unit_len = corpora[paired][0]
    longest = int(unit_len.max())
    # sizing only
    rc, res, chunks = _collect(v, gpu, 0, base, null_sink=True)
    assert rc == 0 and not chunks and (res["n_bytes"], res["n_chunks"], res["max_unit_bytes"]) == (len(want), 0, longest)
    # no reads
    none = dict(v, hits=np.zeros(0, corpus.HIT_DTYPE), offsets=np.zeros(1, np.uint32), read_names=[], seqs=[])
    rc, res, chunks = _collect(none, gpu)
    assert rc == 0 and not chunks and res["n_bytes"] == 0 and res["n_lines"] == 0
    # reads without any record
    n = 700
    unmapped = dict(v, hits=np.zeros(0, corpus.HIT_DTYPE), offsets=np.zeros(n + 1, np.uint32), read_names=[b"u%d" % i for i in range(n)],
                    seqs=[(b"ACGT" * (i % 40), b"T" * (i % 3)) if paired else b"ACGT" * (i % 40) for i in range(n)])
    for u in corpus.variants(unmapped):
        rc, res, chunks = _collect(u, gpu, 4096, 5)
        assert rc == 0 and b"".join(chunks) == corpus.expected(u, 5) and res["n_lines"] == n * (2 if paired else 1) and len(chunks) > 2
    # a unit longer than chunk_bytes
    rc, res, chunks = _collect(v, gpu, longest - 1, base)
    assert rc == _lib.ERR_RANGE and not chunks and res["max_unit_bytes"] == longest and res["n_bytes"] == len(want)
    # a sink that refuses the second chunk
    rc, res, chunks = _collect(v, gpu, longest + 1, base, refuse_at=2)
    assert rc == _lib.ERR_IO and len(chunks) == 2 and b"sink" in _lib.lib().sfgpu_last_error()
    assert b"".join(chunks) == want[:len(chunks[0]) + len(chunks[1])]
    # records that cannot be written: the lowest offender, before any sink call
    for case, read, record, kind in corpus.failing(paired):
        for null_sink in (False, True):
            rc, res, chunks = _collect(case, gpu, null_sink=null_sink)
            assert rc == _lib.ERR_INVALID and not chunks
            assert (res["error_kind"], res["error_read"], res["error_record"]) == (kind, read, record)
    # the same through n_refs: every tid of the batch at or above it is an offender
    tids = v["hits"]["tid"]
    first = int(np.flatnonzero(tids >= 3)[0])
    read = int(np.searchsorted(v["offsets"], first, side="right")) - 1
    rc, res, chunks = _collect(v, gpu, 0, base, n_refs=3)
    assert rc == _lib.ERR_INVALID and not chunks and (res["error_kind"], res["error_read"], res["error_record"]) == (2, read, first - int(v["offsets"][read]))
    # arguments
    assert _collect(v, gpu, 15)[0] == _lib.ERR_INVALID and _collect(v, gpu, (1 << 30) + 1)[0] == _lib.ERR_INVALID
    down = v["offsets"].copy()
    down[3] = down[2] - 1
    for off in (np.concatenate([[1], v["offsets"][1:]]).astype(np.uint32), down):
        rc, _, chunks = _collect(dict(v, offsets=off), gpu)
        assert rc == _lib.ERR_INVALID and not chunks


def _batches(case, cuts):
    """the case cut into batches of reads [cuts[i], cuts[i + 1]): (hits, offsets, read_names, seqs) with offsets from 0"""
    off = case["offsets"].astype(np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        yield (case["hits"][off[a]:off[b]], (off[a:b + 1] - off[a]).astype(np.uint32), None if case["read_names"] is None else case["read_names"][a:b],
               None if case["seqs"] is None else case["seqs"][a:b])


def _device_seqs(seqs, paired, gpu):
    if seqs is None:
        return None
    mates = [[s[m] for s in seqs] for m in (0, 1)] if paired else [seqs]
    pairs = [tuple(_t(x, gpu) for x in corpus.blob(m, np.int64)) for m in mates]
    return tuple(pairs) if paired else pairs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_writer_over_three_batches(gpu, tmp_path, paired):
    """default names: the running read index carries over the batches; then the file read back on the device"""
    from sailfish_amd import samfile
    names = ["t%d" % i for i in range(len(corpus.NAMES))]
    case = dict(corpus.random_case(1, paired, long_seqs=LONG), names=[n.encode() for n in names], read_names=None)
    n = len(case["offsets"]) - 1
    for with_seqs in (True, False):
        v = dict(case, seqs=case["seqs"] if with_seqs else None)
        path = tmp_path / f"out{int(with_seqs)}.sam"
        with samfile.SamDeviceWriter(str(path), names, corpus.REF_LEN, paired, chunk_bytes=20000) as w:
            for h, o, _, s in _batches(v, [0, 97, 98, n]):
                w.write(_t(h.view(np.uint8).reshape(-1), gpu), _t(o, gpu), seqs=_device_seqs(s, paired, gpu))
            stats = w.stats
        seqs = v["seqs"] if with_seqs or not paired else [(b"*", b"*")] * n
        want = samfile._sam_text(names, corpus.REF_LEN, v["hits"], v["offsets"], None, seqs)
        got = path.read_bytes()
        assert got == want, _first_difference(got, want)
        assert (stats["reads"], stats["hits"], stats["batches"]) == (n, len(v["hits"]), 3) and stats["header_bytes"] + stats["bytes"] == len(want)
        chunks = 0                                         # every batch is chunked on its own
        for a, (h, o, _, sq) in zip((0, 97, 98), _batches(v, [0, 97, 98, n])):
            sub = dict(v, hits=h, offsets=o, seqs=sq)
            chunks += _greedy_chunks(_unit_lengths(sub, corpus.expected(sub, a)), 20000)
        assert stats["chunks"] == chunks >= 3 and w.n_reads == n
    # SEQ '*': every line is one the reader takes (a SEQ of another length than the CIGAR's is BAD_LENGTH there)
    hits, off = samfile.read_sam_host(got, names, paired)
    got_hits, got_off = [], [np.zeros(1, np.int64)]
    with samfile.SamFile(str(path), gpu, paired=paired, names=names, block_bytes=1 << 16) as f:
        for h, o in f:
            got_hits.append(h.cpu().numpy())
            got_off.append(o.cpu().numpy().view(np.uint32)[1:].astype(np.int64) + got_off[-1][-1])
    assert np.concatenate(got_hits).tobytes() == hits.tobytes() and np.array_equal(np.concatenate(got_off), off)
    assert len(off) - 1 == n
    # a list of names, a file object, and a record SAM cannot express in the second batch
    bad, read, record, _ = corpus.failing(paired)[0]
    f = open(tmp_path / "bad.sam", "wb")
    w = samfile.SamDeviceWriter(f, names, corpus.REF_LEN, paired)
    ok = list(_batches(case, [0, 5]))[0]
    w.write(_t(ok[0].view(np.uint8).reshape(-1), gpu), _t(ok[1], gpu), read_names=[b"a b", "c", b"", b"d" * 100, b"e"])
    with pytest.raises(ValueError, match=rf"^read {5 + read}, record {record}: "):
        w.write(_t(bad["hits"].view(np.uint8).reshape(-1), gpu), _t(bad["offsets"], gpu))
    w.close()
    assert not f.closed
    f.close()
    want = samfile._sam_text(names, corpus.REF_LEN, ok[0], ok[1], [b"a b", b"c", b"", b"d" * 100, b"e"], [(b"*", b"*")] * 5 if paired else None)
    assert (tmp_path / "bad.sam").read_bytes() == want


def _sample():
    d = np.load(os.path.join(GOLD, "sample_data_reads.npz"))
    n, L = len(d["truth"]), int(d["read_len"])

    def unpack2(p):
        b = np.unpackbits(p).reshape(-1, 2)
        return np.frombuffer(b"ACGT", np.uint8)[(b[:, 0] * 2 + b[:, 1])[: n * L]].reshape(n, L)
    seqs = [bytes(d["seq"][d["seq_off"][t]:d["seq_off"][t + 1]]) for t in range(len(d["names"]))]
    return [str(x) for x in d["names"]], seqs, [bytes(r) for r in unpack2(d["mate1_2bit"])], [bytes(r) for r in unpack2(d["mate2_2bit"])]


def _mapped(idx, r1, r2, batch):
    """the batches QuasiIndex.map_reads returns for the reads, concatenated on the host"""
    import sailfish_amd as sf
    hits, off = [], [np.zeros(1, np.int64)]
    for a in range(0, len(r1), batch):
        h, o = sf.mapper.hits_to_numpy(*idx.map_reads(r1[a:a + batch], r2[a:a + batch]))
        hits.append(h)
        off.append(o[1:].astype(np.int64) + off[-1][-1])
    return np.concatenate(hits), np.concatenate(off).astype(np.uint32)


@pytest.mark.gpu
def test_quantify_reads_and_files_write_their_mappings(gpu, tmp_path):
    import sailfish_amd as sf
    from sailfish_amd import samfile
    names, seqs, r1, r2 = _sample()
    opts = dict(batch_reads=3000, cmd_options={"libType": "IU"}, device=gpu)
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "plain"), sf.SailfishOpts(numFragSamples=5000), **opts)
    assert rc == 0 and exp.numMappedFragments() == 10000
    sam = tmp_path / "mappings.sam"
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "kept"), sf.SailfishOpts(numFragSamples=5000),
                                       write_mappings=str(sam), **opts)
    assert rc == 0 and exp.numMappedFragments() == 10000
    assert (tmp_path / "kept" / "quant.sf").read_bytes() == (tmp_path / "plain" / "quant.sf").read_bytes()
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ref_len = idx.ref_len.cpu().numpy()
    hits, off = _mapped(idx, r1, r2, 3000)
    assert len(off) - 1 == 10000 and (hits["mate_status"] == 3).any()
    want = samfile._sam_text(names, ref_len, hits, off, None, list(zip(r1, r2)))
    got = sam.read_bytes()
    assert got == want, _first_difference(got, want)

    # from files: names with a comment behind a space or a tab; QNAME ends at the first of them
    n = 600
    fa = tmp_path / "transcripts.fasta"
    fa.write_bytes(b"".join(b">" + nm.encode() + b"\n" + s + b"\n" for nm, s in zip(names, seqs)))
    paths = []
    for mate, reads in ((1, r1), (2, r2)):
        p = tmp_path / f"reads_{mate}.fastq"
        p.write_bytes(b"".join(b"@frag.%d%slane=3 mate=%d\n" % (i, b"\t" if i % 3 == 0 else b" ", mate) + r + b"\n+\n" + b"I" * len(r) + b"\n"
                               for i, r in enumerate(reads[:n])))
        paths.append(p)
    out = [tmp_path / "f_plain", tmp_path / "f_kept"]
    fopts = dict(batch_reads=250, cmd_options={"libType": "IU"}, device=gpu)
    rc, _ = sf.mapper.quantify_files(fa, *paths, "IU", str(out[0]), sf.SailfishOpts(numFragSamples=5000), **fopts)
    assert rc == 0
    fsam = tmp_path / "from_files.sam"
    rc, _ = sf.mapper.quantify_files(fa, *paths, "IU", str(out[1]), sf.SailfishOpts(numFragSamples=5000), write_mappings=str(fsam), **fopts)
    assert rc == 0 and (out[1] / "quant.sf").read_bytes() == (out[0] / "quant.sf").read_bytes()
    hits, off = _mapped(idx, r1[:n], r2[:n], 250)
    want = samfile._sam_text(names, ref_len, hits, off, [b"frag.%d" % i for i in range(n)], list(zip(r1[:n], r2[:n])))
    got = fsam.read_bytes()
    assert got == want, _first_difference(got, want)
    assert got.count(b"frag.7\t") >= 2 and b"lane" not in got
    idx.close()
