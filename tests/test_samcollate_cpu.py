"""The collated reading of a SAM text as csrc/samcfmt.h states it (the functions samcollate.hip runs inside its kernels), compiled
as plain C++ with g++ -Wall -Wextra -Werror (tests/samcollate_harness.cpp) and judged by the host reader that is the contract:
samfile.read_sam_collated_host.  Records byte for byte, offsets, counts, and the (kind, line) of every malformed file; the contract
itself is checked against what the corpus says a file must yield, against read_sam_host on name-grouped forms, and against the BAM
statement.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import samcollate_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "samcollate_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
BLOCKS = (0, 1, 7, 64, 4096)
NAME_BLOB = b"".join(n + b"\n" for n in corpus.NAMES)
PAIRED = pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])


class Harness:
    def __init__(self, so):
        L = self.L = C.CDLL(so)
        L.samc_harness_new.restype = C.c_void_p
        L.samc_harness_new.argtypes = [C.c_int, C.c_char_p, C.c_uint64]
        L.samc_harness_free.argtypes = [C.c_void_p]
        L.samc_harness_read.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.samc_harness_export.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]

    def read(self, text, paired, block_bytes=0):
        """-> dict(bad, bad_line (0-based), hits, offsets, lines, header, pairs)"""
        from sailfish_amd.hits import HIT_DTYPE
        h = self.L.samc_harness_new(int(paired), NAME_BLOB, len(NAME_BLOB))
        try:
            out = np.zeros(7, np.uint64)
            self.L.samc_harness_read(h, bytes(text), len(text), block_bytes, out.ctypes.data)
            bad, bad_line, reads, n_hits, lines, header, pairs = (int(x) for x in out)
            hits = np.zeros(n_hits, HIT_DTYPE); off = np.zeros(reads + 1, np.uint32)
            self.L.samc_harness_export(h, hits.ctypes.data, off.ctypes.data)
        finally:
            self.L.samc_harness_free(h)
        return dict(bad=bad, bad_line=bad_line, hits=hits, offsets=off, lines=lines, header=header, pairs=pairs)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("samch")), "libsamc_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    return Harness(so)


def same_as_host(harness, text, paired, blocks=BLOCKS):
    from sailfish_amd.samfile import read_sam_collated_host
    counts = {}
    hits, off = read_sam_collated_host(text, corpus.NAMES, paired, counts=counts)
    for block in blocks:
        got = harness.read(text, paired, block)
        assert got["bad"] == 0, block
        assert got["hits"].tobytes() == hits.tobytes() and np.array_equal(got["offsets"], off), block
        assert (got["lines"], got["header"], len(got["offsets"]) - 1, len(got["hits"]), got["pairs"]) == \
            (counts["lines"], counts["header"], counts["reads"], counts["hits"], counts["pairs"]), block
    return hits, off


def records(text, hits, off):
    from sailfish_amd.hits import HIT_DTYPE
    return {q: np.frombuffer(b, HIT_DTYPE) for q, b in corpus.by_name(text, hits, off).items()}


@PAIRED
def test_names(harness, paired):
    """every name is a fragment of its own, however it resembles another: one pair (two single-end records) each"""
    text = corpus.names_file(paired)
    hits, off = same_as_host(harness, text, paired)
    names = corpus.tricky_names()
    assert {len(n) for n in names} >= {1, 7, 8, 9, 16, 17, 254} and len(off) - 1 == len(names)
    got = records(text, hits, off)
    for i, q in enumerate(names):
        assert got[q]["tid"].tolist() == [i % 5] * (1 if paired else 2), q
        assert sorted(got[q]["pos"].tolist()) == ([9 + i] if paired else [9 + i, 199 + i]), q      # (single end: in the shuffled file order)


@PAIRED
def test_scattered_fragments(harness, paired):
    text = corpus.scattered(paired)
    hits, off = same_as_host(harness, text, paired, blocks=(0, 7, 4096))
    got = records(text, hits, off)
    assert len(off) - 1 == 3002 and list(got)[:2] == [b"wide", b"big"]            # numbered by their first lines
    big = got[b"big"]
    if paired:
        assert got[b"wide"]["mate_status"].tolist() == [3] and got[b"wide"]["mate_pos"].tolist() == [899]
        assert len(big) == 1500 and (big["mate_status"] == 3).all() and (np.diff(big["tid"].astype(np.int64)) >= 0).all()
        assert all((np.diff(big["pos"][big["tid"] == t]) > 0).all() for t in range(7))              # ties keep file order
        assert (big["mate_pos"] == big["pos"] + 500).all()
    else:
        assert len(big) == 3000 and len(got[b"wide"]) == 3
    assert all(len(got[b"one%d" % i]) == 1 for i in (0, 1, 2999))


def test_pairing_by_mate_fields(harness):
    text, want = corpus.pairing(True)
    hits, off = same_as_host(harness, text, True)
    got = records(text, hits, off)
    assert list(got) == list(want)
    for q, w in want.items():
        assert [(int(x["mate_status"]), int(x["tid"]), int(x["pos"]), int(x["mate_pos"])) for x in got[q]] == w, q
    assert got[b"twice"]["read_len"].tolist() == [30, 40] and got[b"twice"]["mate_len"].tolist() == [31, 41]      # the i-th with the i-th
    assert got[b"clip"]["frag_len"].tolist() == [171]
    same_as_host(harness, corpus.pairing(False)[0], False)


@PAIRED
def test_malformed_files(harness, paired):
    from sailfish_amd.samfile import COLLATED_KINDS, read_sam_collated_host
    cases = corpus.malformed(paired)
    assert {c[2] for c in cases} - {0} == set(COLLATED_KINDS)
    for name, text, kind, line in cases:
        if not kind:                                       # the same line is fine in this call
            same_as_host(harness, text, paired, blocks=(0, 64))
            continue
        with pytest.raises(ValueError) as e:
            read_sam_collated_host(text, corpus.NAMES, paired, path="f.sam")
        assert re.match(rf"f\.sam: line {line} is malformed: .* \(kind {kind}\)$", str(e.value)), (name, str(e.value))
        for block in BLOCKS:
            got = harness.read(text, paired, block)
            assert (got["bad"], got["bad_line"] + 1) == (kind, line), (name, block)
            assert len(got["hits"]) == 0 and got["offsets"].tolist() == [0], name      # nothing is emitted


def test_name_grouped_readers_never_raise_bad_qname():
    from sailfish_amd.samfile import read_sam_host
    text, _, _ = corpus.long_qname(True)
    hits, off = read_sam_host(text, corpus.NAMES, True)
    assert len(off) - 1 == 3


@PAIRED
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_files_sorted_and_shuffled(harness, seed, paired):
    """the collated reading of the position-sorted and of the shuffled form equals read_sam_host of the grouped text, fragment by
    fragment (by name: the fragments are numbered by their first lines, which the orders move)"""
    from sailfish_amd.samfile import read_sam_host
    grouped, by_pos, shuffled = corpus.random_forms(seed, paired)
    want = corpus.by_name(grouped, *read_sam_host(grouped, corpus.NAMES, paired))
    assert sum(1 for v in want.values() if not v) > 10 and len(want) == 400
    for text in (grouped, by_pos, shuffled):
        hits, off = same_as_host(harness, text, paired, blocks=(0, 64))
        assert corpus.by_name(text, hits, off) == want
    wrong = read_sam_host(by_pos, corpus.NAMES, paired)[1]
    assert len(wrong) - 1 > 2 * len(want)                    # what the name-grouped reader makes of the sorted file: every line a fragment


@PAIRED
def test_bam_statement(paired):
    from sailfish_amd.samfile import read_bam_collated_host, read_sam_collated_host
    files = corpus.bam_files(paired)
    assert len(files) >= 11 and {"names", "scattered", "pairing", "random1_sorted", "header_only"} <= {f[0] for f in files}
    for name, text, bam in files:
        c1, c2 = {}, {}
        hits, off = read_sam_collated_host(text, corpus.NAMES, paired, counts=c1)
        got, got_off = read_bam_collated_host(bam, corpus.NAMES, paired, counts=c2)
        assert got.tobytes() == hits.tobytes() and np.array_equal(got_off, off), name
        assert (c2["lines"], c2["reads"], c2["hits"], c2["pairs"]) == (c1["lines"] - c1["header"], c1["reads"], c1["hits"], c1["pairs"]), name


def test_empty_and_header_only(harness):
    for text, lines in ((b"", 0), (corpus.header(), 9), (corpus.header()[:-1], 9), (b"@CO\tx", 1)):
        for block in BLOCKS:
            got = harness.read(text, True, block)
            assert (got["bad"], len(got["hits"]), got["offsets"].tolist(), got["lines"], got["header"]) == (0, 0, [0], lines, lines)


def test_header_sort_order(tmp_path):
    from sailfish_amd import gzfile, samfile
    for text, want in ((corpus.header(), "coordinate"), (corpus.header(b"unsorted"), "unsorted"), (b"@SQ\tSN:tA\tLN:1000\n", None),
                       (b"@HD\tVN:1.6\n@SQ\tSN:tA\tLN:1000\n", None), (b"", None)):
        p = tmp_path / "h.sam"
        p.write_bytes(text + b"".join(corpus.mates(True, b"q", 0, 5, 105)))
        assert samfile.header_sort_order(str(p)) == want
        gzfile.write_bgzf(str(tmp_path / "h.sam.gz"), p.read_bytes())
        assert samfile.header_sort_order(str(tmp_path / "h.sam.gz")) == want
        if b"@SQ" in text:
            gzfile.write_bgzf(str(tmp_path / "h.bam"), samfile.sam_to_bam(p.read_bytes()))
            assert samfile.is_bam(str(tmp_path / "h.bam")) and samfile.header_sort_order(str(tmp_path / "h.bam")) == want


def test_sanitized_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer and UBSan, over the corpus files (host code only)"""
    exe = str(tmp_path / "samc_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSAMC_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    names = tmp_path / "names.txt"
    names.write_bytes(NAME_BLOB)
    for paired in (True, False):
        files = []
        bad = [c for c in corpus.malformed(paired) if c[2]]
        for name, text in [f for f in corpus.files(paired) if f[0] != "scattered"] + [(c[0], c[1]) for c in bad]:
            p = tmp_path / f"{name}.{'pe' if paired else 'se'}.sam"; p.write_bytes(text); files.append(str(p))
        r = subprocess.run([exe, "paired" if paired else "single", str(names)] + files, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert re.search(r"pairing\.\w+\.sam bad=0 ", r.stdout) and r.stdout.count("\n") == len(files)
        for name, _, kind, line in bad:
            assert re.search(rf"/{name}\.\w+\.sam bad={kind} line={line - 1} ", r.stdout), name
