"""The rules of a mapper's BAM stream as csrc/bamfmt.h states them (the functions bamtext.hip runs inside its kernels), compiled as
plain C++ with g++ -Wall -Wextra -Werror (tests/bam_harness.cpp) and judged by the host reader that is the contract:
samfile.read_bam_host, which in turn must say what read_sam_host says about the SAM text of the same alignments.  Records byte
for byte, offsets, counts, the (kind, record) of every malformed stream, and the record starts the tile functions find against a
plain walk of the chain.  No GPU."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import bam_corpus as bam
import sam_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "bam_harness.cpp")
GOLD = os.path.join(ROOT, "tests", "golden")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
BLOCKS = (0, 1, 7, 64, 4096)
NAME_BLOB = b"".join(n + b"\n" for n in corpus.NAMES)
BOTH = pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])


def sam_texts(paired):
    """the well-formed SAM corpora; the corner's last line loses its ill-formed optional fields (`b` is no TAG:TYPE:VALUE)"""
    corner = corpus.corner(paired)
    assert corner.endswith(b"\tNH:i:1\tXS:Z:a\tb")
    return [("corner", corner[:-len(b"\tb")]), ("random2", corpus.random_sam(2, paired)), ("random3", corpus.random_sam(3, paired))]


class Harness:
    def __init__(self, so):
        L = self.L = C.CDLL(so)
        L.bam_harness_new.restype = C.c_void_p
        L.bam_harness_new.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
        L.bam_harness_free.argtypes = [C.c_void_p]
        L.bam_harness_read.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.bam_harness_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.bam_harness_chain.restype = C.c_uint32
        L.bam_harness_chain.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64]

    def read(self, text, paired, block_bytes=0):
        """-> dict(bad, bad_record (0-based), hits, offsets, records, pairs, header_bytes)"""
        from sailfish_amd.hits import HIT_DTYPE
        text = bytes(text)
        h = self.L.bam_harness_new(int(paired), NAME_BLOB, len(NAME_BLOB), text, len(text))
        assert h
        try:
            out = np.zeros(7, np.uint64)
            self.L.bam_harness_read(h, text, len(text), block_bytes, out.ctypes.data)
            bad, bad_record, reads, n_hits, records, pairs, header_bytes = (int(x) for x in out)
            hits = np.zeros(n_hits, HIT_DTYPE); off = np.zeros(reads + 1, np.uint32)
            self.L.bam_harness_export(h, hits.ctypes.data, off.ctypes.data)
        finally:
            self.L.bam_harness_free(h)
        return dict(bad=bad, bad_record=bad_record, hits=hits, offsets=off, records=records, pairs=pairs, header_bytes=header_bytes)

    def chain(self, text, skip, n=None):
        return self.L.bam_harness_chain(bytes(text), skip, len(text) if n is None else n)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("bamh")), "libbam_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    return Harness(so)


def same_as_host(harness, stream, paired, blocks=BLOCKS):
    from sailfish_amd.samfile import read_bam_host, read_bam_header  # noqa: F401
    counts = {}
    hits, off = read_bam_host(stream, corpus.NAMES, paired, counts=counts)
    for block in blocks:
        got = harness.read(stream, paired, block)
        assert got["bad"] == 0, block
        assert got["hits"].tobytes() == hits.tobytes() and np.array_equal(got["offsets"], off), block
        assert (got["records"], len(got["offsets"]) - 1, len(got["hits"]), got["pairs"]) == \
            (counts["lines"], counts["reads"], counts["hits"], counts["pairs"]), block
    return hits, off, counts


@BOTH
def test_bam_says_what_the_sam_text_says(harness, paired):
    """read_bam_host(sam_to_bam(text)) = read_sam_host(text) = read_sam_host(bam_to_sam(sam_to_bam(text))), and BamSerial agrees"""
    from sailfish_amd.samfile import bam_to_sam, read_sam_host, sam_to_bam
    for key, text in sam_texts(paired):
        want_counts = {}
        want, want_off = read_sam_host(text, corpus.NAMES, paired, counts=want_counts)
        stream = sam_to_bam(text)
        hits, off, counts = same_as_host(harness, stream, paired)
        assert hits.tobytes() == want.tobytes() and np.array_equal(off, want_off), key
        assert all(counts[k] == want_counts[k] for k in ("reads", "hits", "pairs")), key
        assert counts["lines"] == want_counts["lines"] - want_counts["header"] and counts["header"] == 0
        back_counts = {}
        back, back_off = read_sam_host(bam_to_sam(stream), corpus.NAMES, paired, counts=back_counts)
        assert back.tobytes() == want.tobytes() and np.array_equal(back_off, want_off), key
        assert all(back_counts[k] == want_counts[k] for k in ("reads", "hits", "pairs")), key
        assert sam_to_bam(bam_to_sam(stream)) == stream, key
        assert len(off) > 20 and len(hits) > 50


def test_sam_to_bam_fields_and_refusals():
    from sailfish_amd.samfile import bam_to_sam, sam_to_bam
    head = b"@HD\tVN:1.6\n@SQ\tSN:tA\tLN:1000\n@SQ\tSN:tB\tLN:70000000\n"
    line = b"q\t99\ttB\t65537\t7\t3S10M2D5M\t=\t70000\t20\tACGTNACGTNACGTNACG\t" + bytes(range(33, 51)) + b"\tNH:i:-3\tXA:A:c\tXF:f:1.5\tXZ:Z:a b\tXI:i:70000\n"
    stream = sam_to_bam(head + line)
    p = stream.index(b"tB\0") + 3 + 4
    block_size, ref, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, nref, npos, tlen = np.frombuffer(stream[p:p + 36], "<i4,<i4,<i4,u1,u1,<u2,<u2,<u2,<u4,<i4,<i4,<i4")[0]
    assert (block_size, ref, pos, l_name, mapq, n_cigar, flag, l_seq, nref, npos, tlen) == (len(stream) - p - 4, 1, 65536, 2, 7, 4, 99, 18, 1, 69999, 20)
    assert bin_ == 4681 + (65536 >> 14)                            # reg2bin(65536, 65553): both ends in one 16 kb bin
    assert stream[p + 36:p + 38] == b"q\0" and stream[p + 38 + 16:p + 38 + 16 + 9] == bytes([0x12, 0x48, 0xf1, 0x24, 0x8f, 0x12, 0x48, 0xf1, 0x24])
    assert b"NHc\xfd" in stream and b"XAAc" in stream and b"XZZa b\0" in stream and b"XIi" + (70000).to_bytes(4, "little") in stream
    assert bam_to_sam(stream) == head + line
    star = sam_to_bam(head + b"q\t4\t*\t0\t0\t*\t*\t0\t0\tACG\t*\n")
    assert star.endswith(b"\x12\x40\xff\xff\xff") and bam_to_sam(star).endswith(b"\tACG\t*\n")
    for bad, what in ((b"q\t0\ttA\t1\t0\t1M\t*\t0\t0\tA\t*\tXB:B:c,1\n", "optional field"), (b"q\t0\ttA\t1\t0\t1M\t*\t0\t0\tA\t*\tb\n", "optional field"),
                      (b"q" * 255 + b"\t0\ttA\t1\t0\t1M\t*\t0\t0\tA\t*\n", "QNAME"), (b"q\t0\ttA\t0\t0\t1M\t*\t0\t0\tA\t*\n", "kind 2"),
                      (b"q\t0\ttC\t1\t0\t1M\t*\t0\t0\tA\t*\n", "kind 8"), (b"q\t0\ttA\t1\t0\t1M\t*\t0\t0\n", "kind 1"),
                      (b"q\t0\ttA\t1\t0\t2M\t*\t0\t0\tA\t*\n", "kind 32")):
        with pytest.raises(ValueError, match=what):
            sam_to_bam(head + bad)


@pytest.mark.parametrize("fixture", ["sample_data_hits.npz", "sample_data_hits_scan.npz"])
def test_write_bam_and_header(tmp_path, fixture):
    """write_bam then gzip.open gives sam_to_bam of write_sam's text; the header comes back, and the records through read_bam_host"""
    from sailfish_amd.hits import HIT_DTYPE
    from sailfish_amd.samfile import is_bam, read_bam_header, read_bam_host, read_header, sam_to_bam, write_bam, write_sam
    gold = np.load(os.path.join(GOLD, fixture))
    hits, off = gold["hits"].view(HIT_DTYPE).copy(), gold["offsets"]
    names = [str(x) for x in gold["names"]]
    sam_path, bam_path = tmp_path / "out.sam", tmp_path / "out.bam"
    write_sam(str(sam_path), names, gold["ref_len"], hits, off)
    write_bam(str(bam_path), names, gold["ref_len"], hits, off, member_bytes=3000)
    stream = gzip.open(bam_path).read()
    assert stream == sam_to_bam(sam_path.read_bytes())
    assert bam_path.read_bytes().endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))      # the EOF member
    assert is_bam(str(bam_path)) and not is_bam(str(sam_path))
    h_names, h_lens, header_bytes, text = read_bam_header(str(bam_path))
    assert (h_names, h_lens) == (names, gold["ref_len"].tolist()) == read_header(str(bam_path))
    assert text == b"".join(l + b"\n" for l in sam_path.read_bytes().split(b"\n") if l.startswith(b"@"))
    assert header_bytes == 12 + len(text) + sum(9 + len(n.encode()) for n in names)
    assert stream[header_bytes + 36:].startswith(b"r0\0")
    got, got_off = read_bam_host(stream, names, True)
    assert np.array_equal(got_off, off) and got.tobytes() == hits.tobytes()


def test_header_longer_than_the_first_members(tmp_path):
    from sailfish_amd import gzfile
    from sailfish_amd.samfile import read_bam_header
    refs = [b"ref%05d" % i for i in range(3000)]
    stream = bam.header(refs, list(range(1, 3001)), text=b"@CO\t" + b"x" * 200000 + b"\n")
    p = tmp_path / "long.bam"
    gzfile.write_bgzf(str(p), stream + bam.good_group(True, b"g"), member_bytes=500)
    names, lens, header_bytes, text = read_bam_header(str(p))
    assert names == [r.decode() for r in refs] and lens == list(range(1, 3001)) and header_bytes == len(stream) and len(text) == 200005
    gzfile.write_bgzf(str(p), stream[:-3], member_bytes=500)
    with pytest.raises(ValueError, match="ends inside the BAM header"):
        read_bam_header(str(p))


@BOTH
def test_raw_corpora(harness, paired):
    """the decoy and the spans stream: the fakes in the tags yield nothing, and blocks cut the long records anywhere"""
    decoy = bam.decoy(paired)
    hits, off, counts = same_as_host(harness, decoy, paired)
    assert counts["lines"] == 240 and counts["reads"] == 120 and len(hits) == (120 if paired else 240) and (hits["pos"] < 400).all()
    assert decoy.count(b"fake1\0") == 240
    spans = bam.spans(paired)
    hits, off, counts = same_as_host(harness, spans, paired, blocks=(0, 4096))
    assert len(spans) > 3 * bam.SUPER and counts["lines"] > 9096 and int(np.diff(off.astype(np.int64)).max()) == (2500 if paired else 5000)
    assert (hits["tid"] == 6).sum() >= 2                            # the two long records, among others


@BOTH
def test_malformed_streams(harness, paired):
    from sailfish_amd.samfile import BAM_KINDS, read_bam_host
    cases = bam.malformed(paired)
    assert {c[2] for c in cases} == set(BAM_KINDS)
    for name, stream, kind, record in cases:
        with pytest.raises(ValueError) as e:
            read_bam_host(stream, corpus.NAMES, paired, path="f.bam")
        assert re.match(rf"f\.bam: record {record} is malformed: .* \(kind {kind}\)$", str(e.value), re.S), (name, str(e.value))
        for block in BLOCKS:
            got = harness.read(stream, paired, block)
            assert (got["bad"], got["bad_record"] + 1) == (kind, record), (name, block)
            assert block or len(got["hits"]) == 0, name                # (the call that meets the record emits nothing; earlier calls have)


def test_header_only_and_header_cut_by_blocks(harness):
    long_head = bam.header([b"r%04d" % i for i in range(3000)] + corpus.NAMES, [5] * 3000 + corpus.REF_LEN)
    for head, body, records, reads in ((bam.header(), b"", 0, 0), (bam.header(), bam.good_group(True, b"only"), 2, 1),
                                       (long_head, bam.good_group(True, b"a", 3000) + bam.good_group(True, b"b", 3001), 4, 2)):
        for block in BLOCKS:
            got = harness.read(head + body, True, block)
            assert (got["bad"], got["records"], len(got["offsets"]) - 1, len(got["hits"]), got["header_bytes"]) == (0, records, reads, reads, len(head))
    assert len(long_head) > 4096 * 8


@BOTH
def test_tile_functions_give_the_plain_walk(harness, paired):
    """nxt, pointer doubling, supertile links, tile entries and the per-tile enumeration at T = 64, 256 and the production T against
    a plain walk: on the spans and decoy streams, and on streams that end broken or incomplete at every one of the last 40 bytes"""
    skip = len(bam.header())
    for stream in (bam.spans(paired), bam.decoy(paired), bam.header() + bam.good_group(paired, b"g"), bam.header()):
        assert harness.chain(stream, skip) == 0
    stream = bam.decoy(paired, 12)
    for cut in range(1, 41):
        assert harness.chain(stream, skip, len(stream) - cut) == 0, cut                        # incomplete at the end
        broken = bytearray(stream)
        tail = len(stream) - cut
        broken[tail:tail + 4] = (31).to_bytes(4, "little")                                     # whatever chain passes here breaks
        assert harness.chain(bytes(broken), skip) == 0, cut
    last = p = skip
    while p < len(stream):
        last, p = p, p + 4 + int.from_bytes(stream[p:p + 4], "little")
    assert p == len(stream)
    for bs in (31, 0, -1, 32, 2 ** 31 - 1):                                                    # the last real record's block_size
        broken = bytearray(stream)
        broken[last:last + 4] = (bs & 0xffffffff).to_bytes(4, "little")
        assert harness.chain(bytes(broken), skip) == 0, bs


def test_sanitized_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer and UBSan, over the corpus files (host code only)"""
    from sailfish_amd.samfile import sam_to_bam
    exe = str(tmp_path / "bam_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBAM_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    names = tmp_path / "names.txt"
    names.write_bytes(NAME_BLOB)
    for paired in (True, False):
        files = []
        for name, stream in [(k, sam_to_bam(t)) for k, t in sam_texts(paired)[:2]] + [("decoy", bam.decoy(paired)), ("spans", bam.spans(paired)),
                                                                                     ("header", bam.header())] + [(c[0], c[1]) for c in bam.malformed(paired)]:
            p = tmp_path / f"{name}.{'pe' if paired else 'se'}.bam"; p.write_bytes(stream); files.append(str(p))
        r = subprocess.run([exe, "paired" if paired else "single", str(names)] + files, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert re.search(r"corner\.\w+\.bam bad=0 ", r.stdout) and r.stdout.count("\n") == len(files)
        for name, _, kind, record in bam.malformed(paired):
            assert re.search(rf"/{name}\.\w+\.bam bad={kind} record={record - 1} ", r.stdout), name
