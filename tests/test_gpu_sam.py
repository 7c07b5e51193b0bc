"""The device SAM reader (csrc/samtext.hip behind samfile.SamFile) against the contract, samfile.read_sam_host: records byte for
byte, offsets, counts and error messages, over the corpus of sam_corpus.py, at block sizes that cut lines and groups anywhere,
through every carrier; then quant.quantify_sam against quant.quantify on the same records."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

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
    hits, off = [np.zeros(0, HIT_DTYPE)], [np.zeros(1, np.uint32)]
    for h, o in f:
        o = o.cpu().numpy().view(np.uint32)
        assert o[0] == 0 and h.numel() == 24 * int(o[-1])
        hits.append(h.cpu().numpy().view(HIT_DTYPE)); off.append(o[1:] + off[-1][-1])
    return np.concatenate(hits), np.concatenate(off), f.stats


_HOST = {}


def host_read(key, text, paired):
    """read_sam_host once per text of the corpus"""
    from sailfish_amd.samfile import read_sam_host
    if (key, paired) not in _HOST:
        counts = {}
        _HOST[key, paired] = read_sam_host(text, corpus.NAMES, paired, counts=counts) + (counts,)
    return _HOST[key, paired]


def same(got, want):
    hits, off, stats = got
    w_hits, w_off, counts = want
    assert np.array_equal(off, w_off) and hits.tobytes() == w_hits.tobytes()
    assert (stats["lines"], stats["header_lines"], stats["reads"], stats["hits"], stats["pairs"]) == \
        (counts["lines"], counts["header"], counts["reads"], counts["hits"], counts["pairs"])


@BOTH
@pytest.mark.parametrize("block", [256, 4096, 32 << 20])
def test_corner_and_random_corpus(gpu, tmp_path, paired, block):
    for key, text in (("corner", corpus.corner(paired)), ("random2", corpus.random_sam(2, paired)), ("random3", corpus.random_sam(3, paired))):
        p = tmp_path / f"{key}.sam"
        p.write_bytes(text)
        got = device_read(p, gpu, paired, block_bytes=block)      # names: the @SQ lines
        same(got, host_read(key, text, paired))
        assert got[2]["blocks"] > (10 if block == 256 else 0)


def test_a_block_boundary_at_every_byte_of_a_group(gpu, tmp_path):
    """the first block ends k bytes into the chosen group, for every k: in its names, its numbers, its line ends, and at both of
    its edges (k = 0: the group in front may not be emitted yet, its name might go on)"""
    L = lambda *a, **k: corpus.line(True, *a, **k)
    front = corpus.good_group(True, b"a") + corpus.good_group(True, b"ab", 1)
    chosen = L(b"ab.", 99, 2, 5, b"3S7M") + L(b"ab.", 147, 2, 40, b"10M", eol=b"\r\n") + L(b"ab.", 73 | 0x100, 6, 1, b"*", seq=b"ACGT")
    text = front + chosen + corpus.good_group(True, b"ab", 3) + L(b"z", 77) + L(b"z", 141, eol=b"")
    want = host_read("cut", text, True)
    assert len(want[1]) - 1 == 5
    p = tmp_path / "cut.sam"
    p.write_bytes(text)
    for k in range(len(chosen) + 1):
        same(device_read(p, gpu, True, names=NAMES, block_bytes=len(front) + k), want)


def test_one_group_empty_and_header_only_files(gpu, tmp_path):
    one = b"".join(corpus.line(True, b"only", 99 | (0x100 if i else 0), i % 5, 1 + i, b"50M") +
                   corpus.line(True, b"only", 147 | (0x100 if i else 0), i % 5, 90 + i, b"50M") for i in range(40))
    for key, text, reads in (("one", one, 1), ("one_headed", corpus.header() + one, 1), ("empty", b"", 0), ("header", corpus.header(), 0),
                             ("header_no_nl", corpus.header()[:-1], 0)):
        p = tmp_path / f"{key}.sam"
        p.write_bytes(text)
        for block in (64, 32 << 20):
            got = device_read(p, gpu, True, names=NAMES, block_bytes=block)
            same(got, host_read(key, text, True))
            assert len(got[1]) - 1 == reads and len(got[0]) == 40 * reads


@BOTH
def test_malformed_files(gpu, tmp_path, paired):
    from sailfish_amd.samfile import SamFile, read_sam_host
    for name, text, kind, line in corpus.malformed(paired):
        p = tmp_path / f"{name}.sam"
        p.write_bytes(text)
        with pytest.raises(ValueError) as want:
            read_sam_host(text, corpus.NAMES, paired, path=str(p))
        assert f"line {line} " in str(want.value) and f"(kind {kind})" in str(want.value)
        for block in (256, 32 << 20):
            batches = []
            with pytest.raises(ValueError) as got:
                for b in SamFile(str(p), gpu, paired, names=NAMES, block_bytes=block):
                    batches.append(b)
            assert str(got.value) == str(want.value), (name, block)
            # nothing of the batch that holds the line: what came out is whole groups in front of it
            n_reads = sum(int(o.numel()) - 1 for _, o in batches)
            assert n_reads <= 2 and (block == 256 or not batches), (name, block)


@BOTH
def test_carriers_give_the_same_batches(gpu, tmp_path, paired):
    from sailfish_amd import gzfile
    text = corpus.corner(paired)
    want = host_read("corner", text, paired)
    b, z = tmp_path / "corner.sam.bgzf", tmp_path / "corner.sam.gz"
    gzfile.write_bgzf(str(b), text, member_bytes=3000)
    z.write_bytes(gzip.compress(text))
    for path, kw, where in ((b, dict(block_bytes=8192), "device"), (b, {}, "device"), (z, dict(inflate="device", block_bytes=8192), "device"),
                            (z, dict(inflate="device"), "device"), (z, dict(inflate="host", block_bytes=8192), "host"), (z, {}, "host")):
        got = device_read(path, gpu, paired, **kw)
        same(got, want)
        assert (got[2]["members"] > 0) == (where == "device")


def test_capacity_is_reported_exactly(gpu):
    import torch
    from sailfish_amd import _lib
    from sailfish_amd.hits import HIT_DTYPE
    L = _lib.lib()
    text = np.frombuffer(corpus.random_sam(5, True), np.uint8).copy()
    w_hits, w_off, counts = host_read("random5", text.tobytes(), True)
    blob = np.frombuffer(b"".join(corpus.NAMES), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(n) for n in corpus.NAMES])]).astype(np.int64)
    h = C.c_void_p()
    d_blob, d_off = torch.from_numpy(blob).to(gpu), torch.from_numpy(off).to(gpu)
    _lib.check(L.sfgpu_sam_open(C.byref(h), _lib.ptr(d_blob), _lib.ptr(d_off), len(corpus.NAMES), 1, None))
    try:
        n_hits, n_reads = counts["hits"], counts["reads"]
        hits = torch.zeros(n_hits * 24, dtype=torch.uint8, device=gpu)
        offs = torch.full((n_reads + 1,), -1, dtype=torch.int32, device=gpu)
        res = _lib.SamResult()
        call = lambda ch, cr: L.sfgpu_sam_parse_host(h, _lib.ptr(text), text.size, 1, _lib.ptr(hits), ch, _lib.ptr(offs), cr, C.byref(res), None)
        assert call(n_hits - 1, n_reads) == _lib.ERR_CAPACITY and (res.need_hits, res.need_reads) == (n_hits, n_reads)
        assert res.n_hits == 0 and res.consumed == 0 and not hits.any()
        assert call(n_hits, n_reads - 1) == _lib.ERR_CAPACITY and (res.need_hits, res.need_reads) == (n_hits, n_reads)
        assert call(int(res.need_hits), int(res.need_reads)) == _lib.OK
        assert (res.n_hits, res.n_reads, res.n_pairs, res.consumed) == (n_hits, n_reads, counts["pairs"], text.size)
        assert hits.cpu().numpy().view(HIT_DTYPE).tobytes() == w_hits.tobytes() and np.array_equal(offs.cpu().numpy().view(np.uint32), w_off)
        # a name that occurs twice is refused when the handle is opened
        twice = torch.from_numpy(np.frombuffer(b"tAtBtA", np.uint8).copy()).to(gpu)
        twice_off = torch.tensor([0, 2, 4, 6], dtype=torch.int64, device=gpu)
        h2 = C.c_void_p()
        assert L.sfgpu_sam_open(C.byref(h2), _lib.ptr(twice), _lib.ptr(twice_off), 3, 1, None) == _lib.ERR_INVALID
        assert b"occurs twice" in L.sfgpu_last_error()
    finally:
        L.sfgpu_sam_close(h)


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def _fixture(single):
    from sailfish_amd.hits import HIT_DTYPE
    gold = np.load(os.path.join(GOLD, "sample_data_hits_scan.npz"))
    hits, off = gold["hits"].view(HIT_DTYPE).copy(), gold["offsets"]
    if single:                                       # the left mates alone, as single-end records
        for k in ("mate_pos", "frag_len", "mate_len", "mate_fwd", "mate_status"):
            hits[k] = 0
    return [str(x) for x in gold["names"]], gold["ref_len"], hits, off


@pytest.mark.parametrize("lib", ["IU", "U"])
def test_quantify_sam_writes_what_quantify_writes(gpu, tmp_path, lib):
    import sailfish_amd as sf
    from sailfish_amd import samfile
    names, ref_len, hits, off = _fixture(lib == "U")
    sam = tmp_path / "hits.sam"
    samfile.write_sam(str(sam), names, ref_len, hits, off)
    opts = lambda: sf.SailfishOpts(numFragSamples=5000, dumpEq=True)
    rc, exp = sf.quant.quantify(names, ref_len, [(hits, off)], lib, str(tmp_path / "mem"), opts(), device=gpu)
    assert rc == 0 and exp.numMappedFragments() == 10000
    rc, exp2 = sf.quant.quantify_sam(str(sam), lib, str(tmp_path / "sam"), opts(), device=gpu, block_bytes=1 << 18)
    assert rc == 0 and exp2.numMappedFragments() == 10000 and exp2.numObservedFragments() == exp.numObservedFragments()
    for f in ("quant.sf", os.path.join("aux", "eq_classes.txt")):
        assert (tmp_path / "sam" / f).read_bytes() == (tmp_path / "mem" / f).read_bytes(), f


def test_quantify_sam_with_bias_correction(gpu, tmp_path):
    import sailfish_amd as sf
    from sailfish_amd import samfile
    names, ref_len, hits, off = _fixture(False)
    d = np.load(os.path.join(GOLD, "sample_data_reads.npz"))
    seqs = [bytes(d["seq"][d["seq_off"][t]:d["seq_off"][t + 1]]) for t in range(len(names))]
    assert [str(x) for x in d["names"]] == names
    fa, sam = tmp_path / "transcripts.fasta", tmp_path / "hits.sam.gz"
    fa.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in zip(names, seqs)))
    samfile.write_sam(str(sam), names, ref_len, hits, off, bgzf=True)
    opts = lambda: sf.SailfishOpts(numFragSamples=5000, biasCorrect=True)
    s, o = sf.mapper.pack_sequences([x + b"$" for x in seqs])
    rc, exp = sf.quant.quantify(names, ref_len, [(hits, off)], "IU", str(tmp_path / "mem"), opts(), device=gpu, seq=bytes(s.numpy().tobytes()),
                                seq_off=o[:-1].numpy())
    assert rc == 0
    rc, exp2 = sf.quant.quantify_sam(str(sam), "IU", str(tmp_path / "sam"), opts(), transcripts_path=str(fa), device=gpu, block_bytes=1 << 16)
    assert rc == 0 and exp2.readBias().sum() > 0 and np.array_equal(exp2.readBias(), exp.readBias())
    assert (tmp_path / "sam" / "quant.sf").read_bytes() == (tmp_path / "mem" / "quant.sf").read_bytes()
    stored = [gzip.open(tmp_path / d / "aux" / "observed_bias.gz").read() for d in ("sam", "mem")]
    assert stored[0] == stored[1] == exp.readBias().astype(np.int32).tobytes()
    with pytest.raises(ValueError, match="transcripts_path"):
        sf.quant.quantify_sam(str(sam), "IU", str(tmp_path / "none"), opts(), device=gpu)
    fa.write_bytes(b"".join(b">" + n.encode() + b"\n" + s + b"\n" for n, s in zip(names[::-1], seqs[::-1])))
    with pytest.raises(ValueError, match="@SQ"):
        sf.quant.quantify_sam(str(sam), "IU", str(tmp_path / "swapped"), opts(), transcripts_path=str(fa), device=gpu)
