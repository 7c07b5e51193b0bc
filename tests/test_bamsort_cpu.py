"""The coordinate-sorted BAM file and its BAI index without a GPU: csrc/baifmt.h alone (tests/bamsort_harness.cpp, g++ -Wall -Wextra
-Werror) against the host statements samfile.write_bam(sort="coordinate") and samfile.build_bai, byte for byte over the corpus; a
hand-computed index; samfile.fetch through the index against a brute-force overlap scan; what stays as it was."""
import ctypes as C
import gzip
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import bamsort_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "bamsort_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("bais")), "libbamsort_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.bais_hd_line.restype = C.c_char_p
    L.bais_sort.restype = C.c_int64
    L.bais_sort.argtypes = [_P, C.c_uint64, _P]
    L.bais_index.restype = C.c_int64
    L.bais_index.argtypes = [_P, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.c_uint64, _P, C.c_uint64]
    L.bais_key.restype = C.c_uint64
    L.bais_key.argtypes = [C.c_int32, C.c_int32]
    L.bais_reg2bin.restype = C.c_uint32
    L.bais_reg2bin.argtypes = [C.c_uint32, C.c_uint32]
    return L


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """per case: (case, path of write_bam(sort="coordinate") in members of 32 768 bytes, its inflated stream, its records)"""
    d = tmp_path_factory.mktemp("sorted")
    out = {}
    for name, case in corpus.cases().items():
        path = str(d / f"{name}.bam")
        corpus.write_host(case, path, member_bytes=32768)
        stream = gzip.decompress(open(path, "rb").read())
        out[name] = (case, path, stream, corpus.records(stream))
    return out


def _serial_index(L, stream, p, n_ref, sizes, first_member):
    rec = np.frombuffer(stream[p:], np.uint8)
    sz = np.asarray(sizes, np.uint32)
    need = L.bais_index(rec.ctypes.data if len(rec) else None, len(rec), n_ref, sz.ctypes.data, len(sz), first_member, None, 0)
    assert need >= 0, need
    out = np.zeros(need, np.uint8)
    assert L.bais_index(rec.ctypes.data if len(rec) else None, len(rec), n_ref, sz.ctypes.data, len(sz), first_member, out.ctypes.data, need) == need
    return out.tobytes()


def test_baifmt_serial_equals_the_host_statements(harness, files):
    """the harness sorts the records of the unsorted stream and indexes the result from the member sizes alone: both equal
    write_bam(sort="coordinate") inflated and build_bai of that file, byte for byte, over the whole corpus"""
    from sailfish_amd import samfile
    assert harness.bais_hd_line() == samfile._HD_COORDINATE
    for name, (case, path, stream, recs) in files.items():
        want = corpus.sorted_stream(case)
        assert stream == want, name
        assert samfile.header_sort_order(path) == "coordinate"
        head = samfile.sam_to_bam(samfile.sam_header(case["names"], case["ref_len"], "coordinate"))
        assert stream.startswith(head)
        unsorted = corpus.unsorted_stream(case)
        p = samfile._bam_header(unsorted)[2]
        src, dst = np.frombuffer(unsorted[p:], np.uint8), np.zeros(len(unsorted) - p, np.uint8)
        assert harness.bais_sort(src.ctypes.data if len(src) else None, len(src), dst.ctypes.data if len(dst) else None) == len(recs), name
        assert dst.tobytes() == stream[len(head):], name
        members, _, _ = samfile._bgzf_members(open(path, "rb").read())
        sizes = [b[0] - a[0] for a, b in zip(members[:-1], members[1:])]      # the EOF member is the last and not among them
        first = -(-len(head) // 32768)
        assert [m[2] for m in members[first:-1]] == [32768] * (len(members) - first - 2) + [len(stream) - len(head) - 32768 * (len(members) - first - 2)] \
            or len(stream) == len(head), name
        assert _serial_index(harness, stream, len(head), len(case["names"]), sizes, first) == samfile.build_bai(path), name


def test_corpus_covers_its_rules(harness, files):
    """the shapes the corpus promises: ties, a level-5 bin edge, a recurring bin, an untouched window, straddling records, a long header"""
    from sailfish_amd import samfile
    case, path, stream, recs = files["edges"]
    keys = [harness.bais_key(r[0], r[1]) for r in recs]
    assert keys == sorted(keys) and len(keys) - len(set(keys)) >= 8 and recs[-1][0] == -1
    ties = [r[3] for r in recs if r[0] == 0 and r[1] == 100]
    assert [t[36:t.index(b"\0", 36)] for t in ties] == [b"tie%d.%d" % (b, i) for b in range(3) for i in range(3)]      # write order, across batches
    refs, no_coor = samfile.read_bai(samfile.build_bai(path))
    assert no_coor == sum(r[0] < 0 for r in recs) == 4
    bins, lin, pseudo = refs[0]
    assert len(bins[4681]) == 2 and 585 in bins and 4682 in bins and lin[2] == lin[3] == lin[4] and lin[1] < lin[2] and len(lin) == 7
    assert refs[1] == ({}, [], None) and pseudo[1] == (sum(r[0] == 0 for r in recs), 0)
    assert harness.bais_reg2bin(16383, 16384) == 4681 and harness.bais_reg2bin(16383, 16385) == 585 and harness.bais_reg2bin(16384, 16385) == 4682
    case, path, stream, recs = files["big"]
    head = samfile._bam_header(stream)[2]
    assert len(stream) - head > 3 * 32768 and any((sum(len(r[3]) for r in recs[:k]) % 32768) + len(recs[k][3]) > 32768 for k in range(len(recs)))
    assert samfile._bam_header(files["many_refs"][2])[2] > 32768 and len(files["single"][3]) == 1 and files["nothing"][3] == []
    assert samfile.build_bai(files["nothing"][1]) == b"BAI\1" + struct.pack("<I", 4) + bytes(8 * 4) + bytes(8)


def test_hand_computed_bai():
    """one record at pos 0 of length 10 on reference 0 of two: bin 4681 with one chunk, the pseudo-bin, one window, an empty
    reference 1, n_no_coor 0 -- the expected bytes written out from the specification"""
    from sailfish_amd import gzfile, samfile
    head = samfile.sam_to_bam(b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:a\tLN:100\n@SQ\tSN:b\tLN:100\n")
    body = struct.pack("<iiBBHHHIiii", 0, 0, 2, 255, 4681, 1, 0, 10, -1, -1, 0) + b"q\0" + struct.pack("<I", 10 << 4) + bytes([0x11] * 5) + b"\xff" * 10
    rec = struct.pack("<i", len(body)) + body
    m0, m1 = gzfile.bgzf_member(head), gzfile.bgzf_member(rec)
    blob = m0 + m1 + gzfile.BGZF_EOF
    vbeg, vend = len(m0) << 16, (len(m0) + len(m1)) << 16
    want = (b"BAI\1" + struct.pack("<I", 2)
            + struct.pack("<I", 2)                                          # reference 0: two bins
            + struct.pack("<II", 4681, 1) + struct.pack("<QQ", vbeg, vend)
            + struct.pack("<II", 37450, 2) + struct.pack("<QQ", vbeg, vend) + struct.pack("<QQ", 1, 0)
            + struct.pack("<I", 1) + struct.pack("<Q", vbeg)                # one window
            + struct.pack("<I", 0) + struct.pack("<I", 0)                   # reference 1: no bin, no window
            + struct.pack("<Q", 0))
    assert samfile.build_bai(blob) == want


def test_fetch_equals_brute_force(files, tmp_path):
    """for every corpus file and a grid of regions -- ending and beginning at multiples of 16 384, empty references, empty regions --
    fetch through build_bai returns exactly the records a brute-force overlap scan returns, in file order; by number and by name"""
    from sailfish_amd import samfile
    checked = found = 0
    for name, (case, path, stream, recs) in files.items():
        bai = samfile.build_bai(path)
        for tid, beg, end in corpus.regions(case):
            got = samfile.fetch(path, tid, beg, end, bai=bai)
            assert got == corpus.brute_force(recs, tid, beg, end), (name, tid, beg, end)
            checked += 1
            found += len(got)
    assert checked > 500 and found > 2000
    case, path, stream, recs = files["edges"]
    open(path + ".bai", "wb").write(samfile.build_bai(path))
    assert samfile.fetch(path, "chrB", 0, 60000) == corpus.brute_force(recs, 2, 0, 60000) != []
    assert samfile.fetch(path, "empty", 0, 500) == []


def test_build_bai_raises_on_an_unsorted_file(tmp_path):
    from sailfish_amd import gzfile, samfile
    case = corpus.edges()
    path = tmp_path / "unsorted.bam"
    gzfile.write_bgzf(str(path), corpus.unsorted_stream(case))
    with pytest.raises(ValueError, match="not coordinate-sorted"):
        samfile.build_bai(str(path))


def test_unsorted_write_bam_is_what_it_was(tmp_path):
    """write_bam(sort=None), the default, writes write_bgzf of sam_to_bam of the text, byte for byte; the options are checked"""
    from sailfish_amd import gzfile, mapper, samfile
    case = corpus.pairs()
    m = corpus.merged(case)
    kw = dict(read_names=m["read_names"], seqs=m["seqs"], quals=m["quals"], oriented=True)
    want = io.BytesIO()
    gzfile.write_bgzf(want, samfile.sam_to_bam(samfile._sam_text(case["names"], case["ref_len"], m["hits"], m["offsets"], m["read_names"], m["seqs"],
                                                                  quals=m["quals"], oriented=True)))
    for extra in ({}, {"sort": None}):
        path = tmp_path / "plain.bam"
        samfile.write_bam(str(path), case["names"], case["ref_len"], m["hits"], m["offsets"], **kw, **extra)
        assert path.read_bytes() == want.getvalue()
        assert samfile.header_sort_order(str(path)) == "unsorted"
    with pytest.raises(ValueError, match="sort"):
        samfile.write_bam(str(tmp_path / "x.bam"), case["names"], case["ref_len"], m["hits"], m["offsets"], sort="queryname")
    for fmt in ("sam", "sam.gz"):
        with pytest.raises(ValueError, match="coordinate"):
            samfile.SamDeviceWriter(io.BytesIO(), case["names"], case["ref_len"], True, format=fmt, sort="coordinate")
        with pytest.raises(ValueError, match="mappings_sorted"):
            mapper.quantify_files("t.fa", "r1.fq", None, "U", str(tmp_path / "o"), mappings_format=fmt, mappings_sorted=True, write_mappings=str(tmp_path / "m"))
    with pytest.raises(ValueError, match="sort"):
        samfile.SamDeviceWriter(io.BytesIO(), case["names"], case["ref_len"], True, format="bam", sort="queryname")
    assert samfile.sam_header([b"a"], [5]) == b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@SQ\tSN:a\tLN:5\n"
