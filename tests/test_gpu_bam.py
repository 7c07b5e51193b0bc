"""The device BAM reader (csrc/bamtext.hip behind samfile.SamFile) against the contract, samfile.read_bam_host: records byte for
byte, offsets, counts and error messages, over the corpora of bam_corpus.py and the SAM corpora converted by sam_to_bam, at member
and block sizes that cut records, groups and the header anywhere, through both carriers; then quant.quantify_sam on a BAM file
against the SAM text of the same records."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import bam_corpus as bam
import sam_corpus as corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = [n.decode("utf-8", "surrogateescape") for n in corpus.NAMES]
BOTH = pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])


def device_read(path, gpu, paired, **kw):
    """-> (HIT_DTYPE array, uint32 offsets, stats): the batches of a SamFile joined, offsets rebased"""
    from sailfish_amd.hits import HIT_DTYPE
    from sailfish_amd.samfile import SamFile
    f = SamFile(str(path), gpu, paired, **kw)
    assert f.format == "bam"
    hits, off = [np.zeros(0, HIT_DTYPE)], [np.zeros(1, np.uint32)]
    for h, o in f:
        o = o.cpu().numpy().view(np.uint32)
        assert o[0] == 0 and h.numel() == 24 * int(o[-1])
        hits.append(h.cpu().numpy().view(HIT_DTYPE)); off.append(o[1:] + off[-1][-1])
    return np.concatenate(hits), np.concatenate(off), f.stats


_STREAMS, _HOST = {}, {}


def stream_of(key, paired):
    """the corpus streams, built once"""
    from sailfish_amd.samfile import sam_to_bam
    if (key, paired) not in _STREAMS:
        _STREAMS[key, paired] = {"corner": lambda: sam_to_bam(corpus.corner(paired)[:-2]),      # (without its ill-formed last field, "\tb")
                                 "random2": lambda: sam_to_bam(corpus.random_sam(2, paired)), "random3": lambda: sam_to_bam(corpus.random_sam(3, paired)),
                                 "spans": lambda: bam.spans(paired), "decoy": lambda: bam.decoy(paired)}[key]()
    return _STREAMS[key, paired]


def host_read(key, stream, paired, names=corpus.NAMES):
    """read_bam_host once per stream"""
    from sailfish_amd.samfile import read_bam_host
    if (key, paired) not in _HOST:
        counts = {}
        _HOST[key, paired] = read_bam_host(stream, names, paired, counts=counts) + (counts,)
    return _HOST[key, paired]


def same(got, want):
    hits, off, stats = got
    w_hits, w_off, counts = want
    assert np.array_equal(off, w_off) and hits.tobytes() == w_hits.tobytes()
    assert (stats["lines"], stats["header_lines"], stats["reads"], stats["hits"], stats["pairs"]) == \
        (counts["lines"], 0, counts["reads"], counts["hits"], counts["pairs"])


def write(path, stream, member_bytes=65280):
    from sailfish_amd import gzfile
    gzfile.write_bgzf(str(path), stream, member_bytes=member_bytes)
    return path


@BOTH
@pytest.mark.parametrize("member,block", [(300, 256), (4096, 4096), (65280, 32 << 20)])
def test_corpora_inflated_on_the_device(gpu, tmp_path, paired, member, block):
    for key in ("corner", "random2", "random3", "spans", "decoy"):
        stream = stream_of(key, paired)
        p = write(tmp_path / f"{key}.bam", stream, member)
        got = device_read(p, gpu, paired, names=NAMES, inflate="device", block_bytes=block)
        same(got, host_read(key, stream, paired))
        assert got[2]["members"] >= len(stream) // member and got[2]["blocks"] > 0, key
    assert len(stream_of("spans", paired)) > 3 * bam.SUPER


@BOTH
@pytest.mark.parametrize("block", [256, 4096, 32 << 20])
def test_corpora_inflated_on_the_host(gpu, tmp_path, paired, block):
    for key in ("corner", "random2", "random3", "spans", "decoy"):
        stream = stream_of(key, paired)
        p = write(tmp_path / f"{key}.bam", stream)
        got = device_read(p, gpu, paired, names=NAMES, inflate="host", block_bytes=block)
        same(got, host_read(key, stream, paired))
        assert got[2]["members"] == 0, key
    # a gzip file that is no BGZF goes through the host carrier whatever is asked for; "auto" on BGZF is the device
    stream = stream_of("decoy", paired)
    z = tmp_path / "decoy.gz.bam"
    z.write_bytes(gzip.compress(stream))
    got = device_read(z, gpu, paired, names=NAMES, inflate="device", block_bytes=block)
    same(got, host_read("decoy", stream, paired))
    assert got[2]["members"] == 0
    assert device_read(tmp_path / "decoy.bam", gpu, paired, names=NAMES, block_bytes=block)[2]["members"] > 0


def test_a_block_boundary_at_every_byte_of_a_group(gpu, tmp_path):
    """the first block ends k bytes into the chosen group of three records, for every k: in its block_size words, its fixed fields,
    its names, CIGAR words and tags, and at both of its edges"""
    R = lambda *a, **k: bam.record(True, *a, **k)
    front = bam.header() + bam.good_group(True, b"a") + bam.good_group(True, b"ab", 1)
    chosen = R(b"ab.", 99, 2, 5, [(3, bam.S), (7, bam.M)]) + R(b"ab.", 147, 2, 40, [(10, bam.M)], tags=b"NHC\x02") + \
        R(b"ab.", 73 | 0x100, 6, 1, l_seq=4)
    stream = front + chosen + bam.good_group(True, b"ab", 3) + R(b"z", 77) + R(b"z", 141)
    want = host_read("cut", stream, True)
    assert len(want[1]) - 1 == 5
    p = tmp_path / "cut.bam"
    p.write_bytes(gzip.compress(stream))
    for k in range(len(chosen) + 1):
        same(device_read(p, gpu, True, names=NAMES, inflate="host", block_bytes=len(front) + k), want)


def test_header_only_and_header_longer_than_a_block(gpu, tmp_path):
    from sailfish_amd.samfile import read_header
    head = bam.header()
    one = bam.good_group(True, b"only")
    refs = [b"r%04d" % i for i in range(3000)] + corpus.NAMES
    long_head = bam.header(refs, [5] * 3000 + corpus.REF_LEN)
    long_body = bam.good_group(True, b"a", 3000) + bam.good_group(True, b"b", 3001) + bam.good_group(True, b"c", 3006)
    for key, stream, reads, kw in (("header", head, 0, {}), ("one", head + one, 1, {}), ("long", long_head + long_body, 3, dict(block_bytes=4096))):
        p = write(tmp_path / f"{key}.bam", stream, 3000)
        for inflate in ("device", "host"):
            for block in (kw.get("block_bytes", 64), 32 << 20):
                got = device_read(p, gpu, True, names=NAMES, inflate=inflate, block_bytes=block)
                same(got, host_read(key, stream, True))
                assert len(got[1]) - 1 == reads and len(got[0]) == reads
    assert len(long_head) > 8 * 4096 and read_header(str(tmp_path / "long.bam"))[0][-1] == NAMES[-1]
    assert host_read("long", None, True)[0]["tid"].tolist() == [0, 1, 6]


@BOTH
def test_malformed_streams(gpu, tmp_path, paired):
    from sailfish_amd.samfile import SamFile, read_bam_host
    for name, stream, kind, record in bam.malformed(paired):
        p = write(tmp_path / f"{name}.bam", stream, 3000)
        with pytest.raises(ValueError) as want:
            read_bam_host(stream, corpus.NAMES, paired, path=str(p))
        assert f"record {record} " in str(want.value) and f"(kind {kind})" in str(want.value)
        for inflate, block in (("device", 256), ("device", 32 << 20), ("host", 256), ("host", 32 << 20)):
            batches = []
            with pytest.raises(ValueError) as got:
                for b in SamFile(str(p), gpu, paired, names=NAMES, inflate=inflate, block_bytes=block):
                    batches.append(b)
            assert str(got.value) == str(want.value), (name, inflate, block)
            # nothing of the batch that holds the record: what came out is whole groups in front of it
            n_reads = sum(int(o.numel()) - 1 for _, o in batches)
            assert n_reads <= 3 and (block == 256 or not batches), (name, inflate, block)


def test_direct_calls(gpu):
    """sfgpu_bam_parse_device: SFGPU_ERR_CAPACITY with the exact sizes and then success; a misaligned or slack-less text"""
    import torch
    from sailfish_amd import _lib
    from sailfish_amd.hits import HIT_DTYPE
    from sailfish_amd.samfile import _bam_header
    L = _lib.lib()
    stream = stream_of("random3", True)
    w_hits, w_off, counts = host_read("random3", stream, True)
    refs, _, header_bytes, _ = _bam_header(stream)

    def on_device(items):
        blob = np.frombuffer(b"".join(items), np.uint8).copy()
        off = np.concatenate([[0], np.cumsum([len(n) for n in items])]).astype(np.int64)
        return torch.from_numpy(blob).to(gpu), torch.from_numpy(off).to(gpu)

    d_blob, d_off = on_device(corpus.NAMES)
    d_rblob, d_roff = on_device([r.encode() for r in refs])
    n = len(stream)
    cap_text = ((n + 1 + 15) & ~15) + 16
    text = torch.zeros(cap_text + 16, dtype=torch.uint8, device=gpu)
    text[:n] = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(gpu)
    h = C.c_void_p()
    _lib.check(L.sfgpu_bam_open(C.byref(h), _lib.ptr(d_blob), _lib.ptr(d_off), len(corpus.NAMES), _lib.ptr(d_rblob), _lib.ptr(d_roff), len(refs),
                                header_bytes, 1, None))
    try:
        n_hits, n_reads = counts["hits"], counts["reads"]
        hits = torch.zeros(n_hits * 24, dtype=torch.uint8, device=gpu)
        offs = torch.full((n_reads + 1,), -1, dtype=torch.int32, device=gpu)
        res = _lib.SamResult()
        call = lambda ch, cr, t=text, cap=cap_text: L.sfgpu_bam_parse_device(h, _lib.ptr(t), n, cap, 1, _lib.ptr(hits), ch, _lib.ptr(offs), cr,
                                                                             C.byref(res), None)
        assert call(n_hits, n_reads, text[1:], cap_text) == _lib.ERR_INVALID and b"aligned" in L.sfgpu_last_error()
        assert call(n_hits, n_reads, text, cap_text - 1) == _lib.ERR_INVALID and b"cap_text" in L.sfgpu_last_error()
        assert call(n_hits - 1, n_reads) == _lib.ERR_CAPACITY and (res.need_hits, res.need_reads) == (n_hits, n_reads)
        assert res.n_hits == 0 and res.consumed == 0 and not hits.any()
        assert call(n_hits, n_reads - 1) == _lib.ERR_CAPACITY and (res.need_hits, res.need_reads) == (n_hits, n_reads)
        assert call(int(res.need_hits), int(res.need_reads)) == _lib.OK
        assert (res.n_lines, res.n_header, res.n_hits, res.n_reads, res.n_pairs, res.consumed) == (counts["lines"], 0, n_hits, n_reads, counts["pairs"], n)
        assert hits.cpu().numpy().view(HIT_DTYPE).tobytes() == w_hits.tobytes() and np.array_equal(offs.cpu().numpy().view(np.uint32), w_off)
    finally:
        L.sfgpu_bam_close(h)


def test_names_in_another_order_and_a_reference_that_is_none(gpu, tmp_path):
    """names= in another order than the header's, one header reference missing from them: records on it are RNAME, a file that
    never uses it reads clean with the tids of the given order"""
    from sailfish_amd.samfile import read_bam_host
    names = [NAMES[6], NAMES[0], NAMES[3], NAMES[2], NAMES[1], NAMES[5]]              # without NAMES[4]
    clean = bam.header() + bam.good_group(True, b"g1", 0) + bam.good_group(True, b"g2", 6) + bam.good_group(True, b"g3", 3)
    p = write(tmp_path / "clean.bam", clean)
    want = read_bam_host(clean, names, True)
    assert want[0]["tid"].tolist() == [1, 0, 2]
    got = device_read(p, gpu, True, names=names)
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    uses = clean + bam.good_group(True, b"g4", 4)
    p = write(tmp_path / "uses.bam", uses)
    with pytest.raises(ValueError) as w:
        read_bam_host(uses, names, True, path=str(p))
    assert "record 7 " in str(w.value) and "(kind 8)" in str(w.value)
    with pytest.raises(ValueError) as g:
        device_read(p, gpu, True, names=names)
    assert str(g.value) == str(w.value)


# ---- end to end ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lib", ["IU", "U"])
def test_quantify_sam_on_bam_writes_what_it_writes_on_sam(gpu, tmp_path, lib):
    import sailfish_amd as sf
    from sailfish_amd import samfile
    from sailfish_amd.hits import HIT_DTYPE
    gold = np.load(os.path.join(GOLD, "sample_data_hits_scan.npz"))
    hits, off = gold["hits"].view(HIT_DTYPE).copy(), gold["offsets"]
    if lib == "U":                                   # the left mates alone, as single-end records
        for k in ("mate_pos", "frag_len", "mate_len", "mate_fwd", "mate_status"):
            hits[k] = 0
    names, ref_len = [str(x) for x in gold["names"]], gold["ref_len"]
    sam_path, bam_path = tmp_path / "hits.sam", tmp_path / "hits.bam"
    samfile.write_sam(str(sam_path), names, ref_len, hits, off)
    samfile.write_bam(str(bam_path), names, ref_len, hits, off)
    opts = lambda: sf.SailfishOpts(numFragSamples=5000, dumpEq=True)
    rc, exp = sf.quant.quantify_sam(str(sam_path), lib, str(tmp_path / "sam"), opts(), device=gpu, block_bytes=1 << 18)
    assert rc == 0 and exp.numMappedFragments() == 10000
    rc, exp2 = sf.quant.quantify_sam(str(bam_path), lib, str(tmp_path / "bam"), opts(), device=gpu, block_bytes=1 << 16)
    assert rc == 0 and exp2.numMappedFragments() == exp.numMappedFragments() and exp2.numObservedFragments() == exp.numObservedFragments()
    for f in ("quant.sf", os.path.join("aux", "eq_classes.txt")):
        assert (tmp_path / "bam" / f).read_bytes() == (tmp_path / "sam" / f).read_bytes(), f
