"""The rules of a mapper's SAM text as csrc/samfmt.h states them (the functions samtext.hip runs inside its kernels), compiled as
plain C++ with g++ -Wall -Wextra -Werror (tests/sam_harness.cpp) and judged by the host reader that is the contract:
samfile.read_sam_host.  Records byte for byte, offsets, counts, and the (kind, line) of every malformed file.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sam_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "sam_harness.cpp")
GOLD = os.path.join(ROOT, "tests", "golden")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
BLOCKS = (0, 1, 7, 64, 4096)
NAME_BLOB = b"".join(n + b"\n" for n in corpus.NAMES)


class Harness:
    def __init__(self, so):
        L = self.L = C.CDLL(so)
        L.sam_harness_new.restype = C.c_void_p
        L.sam_harness_new.argtypes = [C.c_int, C.c_char_p, C.c_uint64]
        L.sam_harness_free.argtypes = [C.c_void_p]
        L.sam_harness_read.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.sam_harness_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]

    def read(self, text, paired, block_bytes=0):
        """-> dict(bad, bad_line (0-based), hits, offsets, lines, header, pairs)"""
        from sailfish_amd.hits import HIT_DTYPE
        h = self.L.sam_harness_new(int(paired), NAME_BLOB, len(NAME_BLOB))
        try:
            out = np.zeros(7, np.uint64)
            self.L.sam_harness_read(h, bytes(text), len(text), block_bytes, out.ctypes.data)
            bad, bad_line, reads, n_hits, lines, header, pairs = (int(x) for x in out)
            hits = np.zeros(n_hits, HIT_DTYPE); off = np.zeros(reads + 1, np.uint32)
            self.L.sam_harness_export(h, hits.ctypes.data, off.ctypes.data)
        finally:
            self.L.sam_harness_free(h)
        return dict(bad=bad, bad_line=bad_line, hits=hits, offsets=off, lines=lines, header=header, pairs=pairs)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("samh")), "libsam_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    return Harness(so)


def same_as_host(harness, text, paired):
    from sailfish_amd.samfile import read_sam_host
    counts = {}
    hits, off = read_sam_host(text, corpus.NAMES, paired, counts=counts)
    for block in BLOCKS:
        got = harness.read(text, paired, block)
        assert got["bad"] == 0, block
        assert got["hits"].tobytes() == hits.tobytes() and np.array_equal(got["offsets"], off), block
        assert (got["lines"], got["header"], len(got["offsets"]) - 1, len(got["hits"]), got["pairs"]) == \
            (counts["lines"], counts["header"], counts["reads"], counts["hits"], counts["pairs"]), block
    return hits, off


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_corner_file(harness, paired):
    from sailfish_amd import hits as H
    text = corpus.corner(paired)
    hits, off = same_as_host(harness, text, paired)
    n = lambda q: [l.split(b"\t")[0] for l in text.split(b"\n") if not l.startswith(b"@")].index(q)      # first line of q among the records
    groups = []
    for l in text.split(b"\n"):
        if not l.startswith(b"@") and (not groups or groups[-1] != l.split(b"\t")[0]):
            groups.append(l.split(b"\t")[0])
    assert len(groups) == len(off) - 1 and groups.count(b"q1") == 2
    of = lambda q: hits[off[groups.index(q)]:off[groups.index(q) + 1]]
    assert len(of(b"u1")) == 0 and len(of(b"none")) == 0 and n(b"big") > 0
    if paired:
        assert of(b"mix")["mate_status"].tolist() == [H.PAIRED_END_PAIRED] and of(b"mix")["frag_len"].tolist() == [343]
        assert of(b"rev")["mate_status"].tolist() == [H.PAIRED_END_LEFT, H.PAIRED_END_RIGHT] and of(b"rev")["pos"].tolist() == [199, 399]
        assert of(b"split")["mate_status"].tolist() == [H.PAIRED_END_LEFT, H.PAIRED_END_RIGHT]
        assert of(b"same")["fwd"].tolist() == [1] and of(b"same")["mate_fwd"].tolist() == [1]
        assert of(b"in")["frag_len"].tolist() == [100]
        assert of(b"clip")["pos"].tolist() == [96] and of(b"clip")["mate_pos"].tolist() == [296] and of(b"clip")["read_len"].tolist() == [50]
        assert of(b"hsh")["pos"].tolist() == [94] and of(b"hsh")["read_len"].tolist() == [48]
        assert of(b"star")["read_len"].tolist() == [60] and of(b"star")["mate_len"].tolist() == [33] and of(b"star0")["read_len"].tolist() == [0]
        assert of(b"neg")["pos"].tolist() == [-5] and of(b"neg")["frag_len"].tolist() == [74]
        assert of(b"multi")["tid"].tolist() == [0, 2, 6, 6] and of(b"multi")["pos"].tolist() == [9, 9, 9, 19]
        assert of(b"orph")["mate_status"].tolist() == [1, 1, 1, 2, 2, 2] and of(b"orph")["tid"].tolist() == [1, 4, 4, 2, 2, 6]
        assert of(b"orph")["pos"].tolist() == [3, 2, 5, 1, 4, 0]
        big = of(b"big")
        assert len(big) == 2500 and (np.diff(big["tid"].astype(np.int64)) >= 0).all() and (big["mate_status"] == 3).all()
        assert all((np.diff(big["pos"][big["tid"] == t]) > 0).all() for t in range(7))                # ties keep file order
        assert of(b"edge")["pos"].tolist() == [2 ** 31 - 2, 0] and of(b"edge")["read_len"].tolist() == [65535, 1]
    else:
        assert (hits["mate_status"] == 0).all() and (hits["mate_len"] == 0).all() and (hits["frag_len"] == 0).all()
        assert of(b"mix")["tid"].tolist() == [0, 0, 4, 6] and of(b"orph")["tid"].tolist() == [1, 2, 2, 4, 4, 6]
        assert len(of(b"big")) == 5000
    assert 5 not in hits["tid"]                                 # "unused"
    assert of(b"zeros")["tid"].tolist() == [3] and of(b"last")["pos"].tolist() == [76]


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
@pytest.mark.parametrize("seed", range(8))
def test_random_files(harness, seed, paired):
    hits, off = same_as_host(harness, corpus.random_sam(seed, paired), paired)
    assert len(off) > 100 and len(hits) > 100


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_malformed_files(harness, paired):
    from sailfish_amd.samfile import KINDS, read_sam_host
    cases = corpus.malformed(paired)
    assert {c[2] for c in cases} == set(KINDS)
    for name, text, kind, line in cases:
        with pytest.raises(ValueError) as e:
            read_sam_host(text, corpus.NAMES, paired, path="f.sam")
        assert re.match(rf"f\.sam: line {line} is malformed: .* \(kind {kind}\)$", str(e.value)), (name, str(e.value))
        for block in BLOCKS:
            got = harness.read(text, paired, block)
            assert (got["bad"], got["bad_line"] + 1) == (kind, line), (name, block)
            assert block or len(got["hits"]) == 0, name                # (the call that meets the line emits nothing; earlier calls have)


def test_empty_and_header_only(harness):
    for text, lines in ((b"", 0), (corpus.header(), 9), (corpus.header()[:-1], 9), (b"@CO\tx", 1)):
        for block in BLOCKS:
            got = harness.read(text, True, block)
            assert (got["bad"], len(got["hits"]), got["offsets"].tolist(), got["lines"], got["header"]) == (0, 0, [0], lines, lines)


@pytest.mark.parametrize("fixture", ["sample_data_hits.npz", "sample_data_hits_scan.npz"])
def test_write_sam_round_trip(tmp_path, fixture):
    """write_sam then read_sam_host returns the mapper fixture's records byte for byte.  One field is masked: mate_len of the
    orphan records (status 1 / 2), which SAM does not carry -- the mate of an orphan has no line."""
    from sailfish_amd.hits import HIT_DTYPE
    from sailfish_amd.samfile import read_header, read_sam_host, write_sam
    gold = np.load(os.path.join(GOLD, fixture))
    hits, off = gold["hits"].view(HIT_DTYPE).copy(), gold["offsets"]
    names = [str(x) for x in gold["names"]]
    path = tmp_path / "out.sam"
    write_sam(str(path), names, gold["ref_len"], hits, off)
    assert read_header(str(path)) == (names, gold["ref_len"].tolist())
    got, got_off = read_sam_host(path.read_bytes(), names, True)
    orphan = (hits["mate_status"] == 1) | (hits["mate_status"] == 2)
    assert (hits["mate_status"] == 3).any()
    hits["mate_len"][orphan] = 0                                # (the committed fixtures hold pair records only: nothing is masked today)
    assert np.array_equal(got_off, off) and got.tobytes() == hits.tobytes()


def test_write_sam_single_end_and_negative_positions(tmp_path):
    from sailfish_amd.hits import HIT_DTYPE
    from sailfish_amd.samfile import read_sam_host, write_sam
    recs = np.array([(0, -7, 0, 0, 50, 0, 1, 0, 0, 0), (3, 12, 0, 0, 50, 0, 0, 0, 0, 0), (6, 0, 0, 0, 1, 0, 1, 0, 0, 0)], HIT_DTYPE)
    off = np.array([0, 2, 2, 3], np.uint32)
    names = [n.decode("utf-8") for n in corpus.NAMES]
    path = tmp_path / "se.sam"
    write_sam(str(path), names, corpus.REF_LEN, recs, off, read_names=["a b", "c", "d"], seqs=[b"A" * 50, b"C" * 9, b"G"])
    got, got_off = read_sam_host(path.read_bytes(), names, False)
    assert np.array_equal(got_off, off) and got.tobytes() == recs.tobytes()
    assert b"\n" + b"\t".join([b"c", b"4", b"*", b"0", b"255", b"*", b"*", b"0", b"0", b"C" * 9, b"*"]) + b"\n" in path.read_bytes()
    with pytest.raises(ValueError):
        write_sam(str(path), names, corpus.REF_LEN, np.array([(0, -50, 0, 0, 50, 0, 1, 0, 0, 0)], HIT_DTYPE), np.array([0, 1], np.uint32))


def test_sanitized_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer and UBSan, over the corpus files (host code only)"""
    exe = str(tmp_path / "sam_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSAM_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    names = tmp_path / "names.txt"
    names.write_bytes(NAME_BLOB)
    for paired in (True, False):
        files = []
        for name, text in [("corner", corpus.corner(paired)), ("random", corpus.random_sam(1, paired)), ("empty", b""), ("header", corpus.header())] + \
                [(c[0], c[1]) for c in corpus.malformed(paired)]:
            p = tmp_path / f"{name}.{'pe' if paired else 'se'}.sam"; p.write_bytes(text); files.append(str(p))
        r = subprocess.run([exe, "paired" if paired else "single", str(names)] + files, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert re.search(r"corner\.\w+\.sam bad=0 ", r.stdout) and r.stdout.count("\n") == len(files)
        for name, _, kind, line in corpus.malformed(paired):
            assert re.search(rf"/{name}\.\w+\.sam bad={kind} line={line - 1} ", r.stdout), name
