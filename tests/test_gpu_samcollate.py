"""The collated device reader (csrc/samcollate.hip behind samfile.SamFile(collate=True)) against the contract,
samfile.read_sam_collated_host / read_bam_collated_host: records byte for byte, offsets, counts and error messages, over the corpus
of samcollate_corpus.py, at block sizes that take many collect calls, through every carrier and as BAM; the raw C interface; then
quant.quantify_sam on a name-grouped file against quantify_sam(collate=True) on its position-sorted SAM and BAM forms."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import samcollate_corpus as corpus

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = [n.decode("utf-8", "surrogateescape") for n in corpus.NAMES]
BOTH = pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])


def device_read(path, gpu, paired, **kw):
    """-> (HIT_DTYPE array, uint32 offsets, stats, batches): the batches of a collated SamFile joined, offsets rebased"""
    from sailfish_amd.hits import HIT_DTYPE
    from sailfish_amd.samfile import SamFile
    f = SamFile(str(path), gpu, paired, collate=kw.pop("collate", True), **kw)
    hits, off, batches = [np.zeros(0, HIT_DTYPE)], [np.zeros(1, np.uint32)], 0
    for h, o in f:
        o = o.cpu().numpy().view(np.uint32)
        assert o[0] == 0 and h.numel() == 24 * int(o[-1])
        hits.append(h.cpu().numpy().view(HIT_DTYPE)); off.append(o[1:] + off[-1][-1]); batches += 1
    return np.concatenate(hits), np.concatenate(off), f.stats, batches


_HOST = {}


def host_read(key, data, paired, bam=False):
    """the host statement once per file of the corpus"""
    from sailfish_amd.samfile import read_bam_collated_host, read_sam_collated_host
    if (key, paired, bam) not in _HOST:
        counts = {}
        _HOST[key, paired, bam] = (read_bam_collated_host if bam else read_sam_collated_host)(data, corpus.NAMES, paired, counts=counts) + (counts,)
    return _HOST[key, paired, bam]


def same(got, want):
    hits, off, stats, _ = got
    w_hits, w_off, counts = want
    assert np.array_equal(off, w_off) and hits.tobytes() == w_hits.tobytes()
    assert (stats["lines"], stats["header_lines"], stats["reads"], stats["hits"], stats["pairs"], stats["fragments"]) == \
        (counts["lines"], counts["header"], counts["reads"], counts["hits"], counts["pairs"], counts["reads"])


@BOTH
@pytest.mark.parametrize("block", [256, 32 << 20])
def test_corpus_plain(gpu, tmp_path, paired, block):
    """every file of the corpus; 256-byte blocks: hundreds of collect calls, and lines longer than a block ("present more")"""
    for key, text in corpus.files(paired):
        p = tmp_path / f"{key}.sam"
        p.write_bytes(text)
        got = device_read(p, gpu, paired, names=NAMES, block_bytes=block)
        same(got, host_read(key, text, paired))
        assert got[2]["calls"] >= (len(text) // 512 if block == 256 else 1 if text else 0) and got[2]["state_bytes"] >= 32 * (got[2]["lines"] - got[2]["header_lines"])
        rounds = got[2]["sort_rounds"]                  # (length byte + name) / 8, rounded up, of the longest name that needs telling apart
        assert rounds == 32 if key == "names" else 1 <= rounds <= 4 if got[2]["reads"] else rounds == 0, key


@BOTH
def test_carriers_give_the_same_records(gpu, tmp_path, paired):
    from sailfish_amd import gzfile
    for key in ("names", "pairing", "random1_sorted"):
        text = dict(corpus.files(paired))[key]
        want = host_read(key, text, paired)
        b, z = tmp_path / f"{key}.sam.bgzf", tmp_path / f"{key}.sam.gz"
        gzfile.write_bgzf(str(b), text, member_bytes=700)
        z.write_bytes(gzip.compress(text))
        for path, kw, where in ((b, dict(block_bytes=1024), "device"), (b, {}, "device"), (z, dict(inflate="device", block_bytes=8192), "device"),
                                (z, dict(inflate="host", block_bytes=256), "host"), (z, {}, "host")):
            got = device_read(path, gpu, paired, names=NAMES, **kw)
            same(got, want)
            assert (got[2]["members"] > 0) == (where == "device")
            if kw.get("block_bytes", 1 << 20) <= 1024:
                assert got[2]["calls"] >= len(text) // 4096


@BOTH
def test_corpus_as_bam(gpu, tmp_path, paired):
    """BGZF members of a few hundred bytes (records straddle members, and collect calls), the whole file in one block, and gzip on
    the host in 256-byte blocks"""
    from sailfish_amd import gzfile
    for key, text, bam in corpus.bam_files(paired):
        want = host_read(key, bam, paired, bam=True)
        assert want[0].tobytes() == host_read(key, text, paired)[0].tobytes()
        b, z = tmp_path / f"{key}.bam", tmp_path / f"{key}.bam.gz"
        gzfile.write_bgzf(str(b), bam, member_bytes=400)
        z.write_bytes(gzip.compress(bam))
        small = key != "scattered"                      # (the one large file: members of 400 bytes, blocks of 64 KiB)
        for path, kw in ((b, dict(block_bytes=1024 if small else 1 << 16)), (b, {}), (z, dict(block_bytes=256 if small else 1 << 16))):
            got = device_read(path, gpu, paired, names=NAMES, **kw)
            same(got, want)
            if small and kw:
                assert got[2]["calls"] >= len(bam) // 4096


@BOTH
@pytest.mark.parametrize("key", ["pairing", "random2_shuffled"])
def test_batch_reads(gpu, tmp_path, paired, key):
    text = dict(corpus.files(paired))[key]
    want = host_read(key, text, paired)
    p = tmp_path / f"{key}.sam"
    p.write_bytes(text)
    reads = len(want[1]) - 1
    for batch, n in ((1, reads), (7, -(-reads // 7)), (1_000_000, 1)):
        got = device_read(p, gpu, paired, names=NAMES, batch_reads=batch)
        same(got, want)
        assert got[3] == n


def _open(gpu, paired):
    import torch
    from sailfish_amd import _lib
    L = _lib.lib()
    blob = np.frombuffer(b"".join(corpus.NAMES), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum([len(n) for n in corpus.NAMES])]).astype(np.int64)
    h = C.c_void_p()
    d_blob, d_off = torch.from_numpy(blob).to(gpu), torch.from_numpy(off).to(gpu)
    _lib.check(L.sfgpu_sam_open(C.byref(h), _lib.ptr(d_blob), _lib.ptr(d_off), len(corpus.NAMES), int(paired), None))
    return L, h


def test_raw_interface(gpu):
    """capacity reported exactly with nothing written; call order; a `paired` mismatch; a slice beyond the collection"""
    import torch
    from sailfish_amd import _lib
    from sailfish_amd.hits import HIT_DTYPE
    text = np.frombuffer(dict(corpus.files(True))["random1_sorted"], np.uint8).copy()
    w_hits, w_off, counts = host_read("random1_sorted", text.tobytes(), True)
    L, h = _open(gpu, True)
    _, h_single = _open(gpu, False)
    c, c_single = C.c_void_p(), C.c_void_p()
    _lib.check(L.sfgpu_samc_open(C.byref(c), 1, None))
    _lib.check(L.sfgpu_samc_open(C.byref(c_single), 0, None))
    try:
        res, info = _lib.SamResult(), _lib.SamcInfo()
        n_hits, n_reads = counts["hits"], counts["reads"]
        hits = torch.zeros(n_hits * 24, dtype=torch.uint8, device=gpu)
        offs = torch.full((n_reads + 1,), -1, dtype=torch.int32, device=gpu)
        emit = lambda first, n, cap: L.sfgpu_samc_emit(c, first, n, _lib.ptr(hits), cap, _lib.ptr(offs), C.byref(res), None)
        collect = lambda handle, into, final=1: L.sfgpu_sam_collect_host(handle, into, _lib.ptr(text), text.size, final, C.byref(res), None)
        assert collect(h, c_single) == _lib.ERR_INVALID and collect(h_single, c) == _lib.ERR_INVALID
        assert emit(0, 0, n_hits) == _lib.ERR_STATE                                   # emit before finish
        ends = np.flatnonzero(text == 10)
        half = int(ends[len(ends) // 2]) + 8                                          # a block that ends inside a line
        assert L.sfgpu_sam_collect_host(h, c, _lib.ptr(text), half, 0, C.byref(res), None) == _lib.OK
        used = int(res.consumed)
        assert 0 < used <= half and text[used - 1] == 10 and (res.n_reads, res.n_hits) == (0, 0) and res.n_lines == int((text[:used] == 10).sum())
        rest = text[used:].copy()
        assert L.sfgpu_sam_collect_host(h, c, _lib.ptr(rest), rest.size, 1, C.byref(res), None) == _lib.OK and res.consumed == rest.size
        assert L.sfgpu_samc_finish(c, C.byref(info), None) == _lib.OK
        assert (info.n_lines, info.n_reads, info.n_hits, info.n_pairs) == (counts["lines"] - counts["header"], n_reads, n_hits, counts["pairs"])
        assert 1 <= info.sort_rounds <= 32 and info.state_bytes >= 32 * info.n_lines
        assert collect(h, c) == _lib.ERR_STATE and L.sfgpu_samc_finish(c, C.byref(info), None) == _lib.ERR_STATE      # collect after finish
        assert emit(0, n_reads, n_hits - 1) == _lib.ERR_CAPACITY and res.need_hits == n_hits
        assert res.n_hits == 0 and not hits.any() and (offs == -1).all()               # nothing written
        assert emit(1, n_reads, n_hits) == _lib.ERR_RANGE
        assert emit(0, n_reads, n_hits) == _lib.OK and (res.n_reads, res.n_hits, res.n_pairs) == (n_reads, n_hits, counts["pairs"])
        assert hits.cpu().numpy().view(HIT_DTYPE).tobytes() == w_hits.tobytes() and np.array_equal(offs.cpu().numpy().view(np.uint32), w_off)
        first = n_reads // 3                                                          # a slice in the middle: d_off[0] = 0
        assert emit(first, 5, n_hits) == _lib.OK
        o = offs.cpu().numpy().view(np.uint32)[:6]
        assert o[0] == 0 and np.array_equal(o, w_off[first:first + 6] - w_off[first])
        assert hits.cpu().numpy().view(HIT_DTYPE)[:o[5]].tobytes() == w_hits[w_off[first]:w_off[first + 5]].tobytes()
    finally:
        L.sfgpu_samc_close(c); L.sfgpu_samc_close(c_single)
        L.sfgpu_sam_close(h); L.sfgpu_sam_close(h_single)


@BOTH
def test_malformed_files(gpu, tmp_path, paired):
    """the line stands in a late block; the message is the host statement's, with the file-wide line number; nothing is emitted"""
    from sailfish_amd.samfile import SamFile, read_sam_collated_host
    for name, text, kind, line in corpus.malformed(paired):
        if not kind:
            continue
        p = tmp_path / f"{name}.sam"
        p.write_bytes(text)
        with pytest.raises(ValueError) as want:
            read_sam_collated_host(text, corpus.NAMES, paired, path=str(p))
        assert f"line {line} " in str(want.value) and f"(kind {kind})" in str(want.value)
        for block in (256, 32 << 20):
            batches = []
            f = SamFile(str(p), gpu, paired, names=NAMES, block_bytes=block, collate=True)
            with pytest.raises(ValueError) as got:
                for b in f:
                    batches.append(b)
            assert str(got.value) == str(want.value), (name, block)
            assert not batches and (block != 256 or line < 20 or f.stats["calls"] > 5), (name, block)


def test_malformed_bam_record_in_a_late_block(gpu, tmp_path):
    from sailfish_amd import gzfile
    from sailfish_amd.samfile import SamFile, read_bam_collated_host
    bam = dict((k, b) for k, _, b in corpus.bam_files(True))["random1_sorted"][:-7]      # the stream ends inside the last record
    p = tmp_path / "cut.bam"
    gzfile.write_bgzf(str(p), bam, member_bytes=400)
    with pytest.raises(ValueError) as want:
        read_bam_collated_host(bam, corpus.NAMES, True, path=str(p))
    assert "record 1647 " in str(want.value) and "(kind 1)" in str(want.value)
    for block in (1024, 32 << 20):
        with pytest.raises(ValueError) as got:
            list(SamFile(str(p), gpu, True, names=NAMES, block_bytes=block, collate=True))
        assert str(got.value) == str(want.value)


def test_collate_auto(gpu, tmp_path):
    """auto collates iff the header says SO:coordinate"""
    from sailfish_amd.samfile import SamFile, read_sam_host
    _, by_pos, _ = corpus.random_forms(1, True)
    want = host_read("random1_sorted", by_pos, True)
    for key, text, collated in (("coordinate", by_pos, True), ("unsorted", by_pos.replace(b"SO:coordinate", b"SO:unsorted"), False),
                                ("no_hd", by_pos[by_pos.index(b"@SQ"):], False)):
        p = tmp_path / f"{key}.sam"
        p.write_bytes(text)
        f = SamFile(str(p), gpu, True, collate="auto")
        assert f.collated == collated
        f.close()
        got = device_read(p, gpu, True, collate="auto")
        if collated:
            same(got, want)
        else:                                            # read as the name-grouped file it says it is
            w_hits, w_off = read_sam_host(text, corpus.NAMES, True)
            assert np.array_equal(got[1], w_off) and got[0].tobytes() == w_hits.tobytes() and "fragments" not in got[2]
    with pytest.raises(ValueError, match="collate"):
        SamFile(str(p), gpu, True, collate="yes")


def test_quantify_sam_from_position_sorted_files(gpu, tmp_path):
    """quantify_sam on the name-grouped file, and with collate=True on its position-sorted SAM and BAM forms: the same quant.sf and
    eq_classes.txt.  The library holds fewer fragments than numFragSamples, so the fragment-length sample is the same set."""
    import sailfish_amd as sf
    from sailfish_amd import gzfile, samfile
    from sailfish_amd.hits import HIT_DTYPE
    gold = np.load(os.path.join(GOLD, "sample_data_hits_scan.npz"))
    hits, off = gold["hits"].view(HIT_DTYPE).copy(), gold["offsets"]
    names, ref_len = [str(x) for x in gold["names"]], gold["ref_len"]
    grouped = samfile._sam_text(names, ref_len, hits, off, None, None)
    lines = grouped.split(b"\n")[:-1]
    head = [l.replace(b"SO:unsorted\tGO:query", b"SO:coordinate") + b"\n" for l in lines if l.startswith(b"@")]
    tid_of = {n.encode(): i for i, n in enumerate(names)}
    body = sorted((l + b"\n" for l in lines if not l.startswith(b"@")), key=lambda l: (tid_of[l.split(b"\t")[2]], int(l.split(b"\t")[3])))
    by_pos = b"".join(head + body)
    g, s, b = tmp_path / "grouped.sam", tmp_path / "sorted.sam", tmp_path / "sorted.bam"
    g.write_bytes(grouped); s.write_bytes(by_pos)
    gzfile.write_bgzf(str(b), samfile.sam_to_bam(by_pos))
    assert samfile.header_sort_order(str(s)) == samfile.header_sort_order(str(b)) == "coordinate"
    opts = lambda: sf.SailfishOpts(numFragSamples=20000, dumpEq=True)
    n_frags = len(off) - 1
    assert n_frags < 20000
    rc, exp = sf.quant.quantify_sam(str(g), "IU", str(tmp_path / "grouped"), opts(), device=gpu)
    assert rc == 0 and exp.numObservedFragments() == n_frags
    for path, out, collate in ((s, "sorted_sam", True), (b, "sorted_bam", "auto")):
        rc, exp2 = sf.quant.quantify_sam(str(path), "IU", str(tmp_path / out), opts(), device=gpu, collate=collate, block_bytes=1 << 18)
        assert rc == 0 and exp2.numMappedFragments() == exp.numMappedFragments() and exp2.numObservedFragments() == n_frags
        for f in ("quant.sf", os.path.join("aux", "eq_classes.txt")):
            assert (tmp_path / out / f).read_bytes() == (tmp_path / "grouped" / f).read_bytes(), (out, f)
