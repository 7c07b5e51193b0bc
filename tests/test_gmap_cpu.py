"""The rules of a --geneMap file as csrc/gtffmt.h states them (the functions genemap.hip runs inside its kernels), compiled as plain
C++ with g++ -Wall -Wextra -Werror (tests/gmap_harness.cpp) and judged by the host readers that are the contract:
genes.TranscriptGeneMap.from_gtf and .from_file.  Exact list equality of transcript_names, t2g and gene_names.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gmap_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "gmap_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]


class Harness:
    def __init__(self, so):
        L = self.L = C.CDLL(so)
        L.gmap_harness_new.restype = C.c_void_p
        L.gmap_harness_new.argtypes = [C.c_int, C.c_char_p, C.c_uint32]
        L.gmap_harness_free.argtypes = [C.c_void_p]
        L.gmap_harness_map.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.gmap_harness_export.argtypes = [C.c_void_p] + [C.c_void_p] * 5

    def map(self, is_gtf, key, text, block_bytes=0):
        """-> dict(flags, transcript_names, t2g, gene_names, n_lines, n_records); names as str"""
        key = key.encode("ascii")
        h = self.L.gmap_harness_new(int(is_gtf), key, len(key))
        try:
            out = np.zeros(7, np.uint64)
            self.L.gmap_harness_map(h, bytes(text), len(text), block_bytes, out.ctypes.data)
            flags, T, G, tb, gb, n_lines, n_records = (int(x) for x in out)
            tn = np.zeros(tb + 1, np.uint8); to = np.zeros(T + 1, np.uint64); t2g = np.zeros(T + 1, np.uint32)
            gn = np.zeros(gb + 1, np.uint8); go = np.zeros(G + 1, np.uint64)
            self.L.gmap_harness_export(h, tn.ctypes.data, to.ctypes.data, t2g.ctypes.data, gn.ctypes.data, go.ctypes.data)
        finally:
            self.L.gmap_harness_free(h)
        cut = lambda blob, off, n: [bytes(blob[int(off[i]):int(off[i + 1])]).decode("ascii") for i in range(n)]
        return dict(flags=flags, transcript_names=cut(tn, to, T), t2g=[int(x) for x in t2g[:T]], gene_names=cut(gn, go, G),
                    n_lines=n_lines, n_records=n_records)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("gmh")), "libgmap_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    return Harness(so)


def host_map(tmp_path, is_gtf, key, text):
    from sailfish_amd.genes import TranscriptGeneMap
    p = tmp_path / ("m.gtf" if is_gtf else "m.tsv")
    p.write_bytes(text)
    m = TranscriptGeneMap.from_gtf(str(p), key) if is_gtf else TranscriptGeneMap.from_file(str(p))
    return dict(transcript_names=m.transcript_names, t2g=m.t2g, gene_names=m.gene_names)


def same(got, want):
    assert got["flags"] == 0
    for k in ("transcript_names", "t2g", "gene_names"):
        assert got[k] == want[k], k


@pytest.mark.parametrize("key", corpus.KEYS + ("exon_number", "gene_id\x0b", "", "a;b"))
def test_corner_gtf(harness, tmp_path, key):
    text = corpus.corner_gtf()
    want = host_map(tmp_path, True, key, text)
    assert len(want["transcript_names"]) > 40 and (key not in corpus.KEYS or len(want["gene_names"]) > 10)
    same(harness.map(True, key, text), want)


def test_corner_tsv(harness, tmp_path):
    text = corpus.corner_tsv()
    want = host_map(tmp_path, False, "gene_id", text)
    assert "odd_one_out" not in want["transcript_names"] and want["transcript_names"].count("t1") == 3
    same(harness.map(False, "gene_id", text), want)


@pytest.mark.parametrize("seed", range(20))
def test_random_files(harness, tmp_path, seed):
    text = corpus.random_gtf(seed)
    key = corpus.KEYS[seed % 4]
    same(harness.map(True, key, text), host_map(tmp_path, True, key, text))
    text = corpus.random_tsv(seed)
    same(harness.map(False, key, text), host_map(tmp_path, False, key, text))


def test_key_at_every_alignment(harness, tmp_path):
    """the pad in column 2 moves the attribute column through all 16 positions of a 16-byte group"""
    text = "".join(corpus.gtf_line(f'gene_id "g{i % 3}"; transcript_id "t{i:02d}"; gene_name "n{i % 5}";', pad="p" * i) for i in range(32)).encode()
    starts = {text.split(b"\n")[i].index(b"gene_id") % 16 for i in range(32)}
    assert starts == set(range(16))
    for key in ("gene_id", "gene_name"):
        same(harness.map(True, key, text), host_map(tmp_path, True, key, text))


@pytest.mark.parametrize("name,is_gtf,text,flag", corpus.flagged(), ids=[f[0] for f in corpus.flagged()])
def test_host_only_inputs_are_flagged(harness, name, is_gtf, text, flag):
    got = harness.map(is_gtf, "gene_id", text)
    assert got["flags"] & flag and got["transcript_names"] == []
    assert harness.map(is_gtf, "gene_id", text, block_bytes=5)["flags"] & flag


def test_name_at_the_cap_is_not_flagged(harness):
    t = "L" * corpus.NAME_CAP
    assert harness.map(True, "gene_id", corpus.gtf_line(f'transcript_id "{t}"; gene_id "{t}";').encode())["flags"] == 0
    assert harness.map(False, "gene_id", f"{t} {t}\n".encode())["flags"] == 0


@pytest.mark.parametrize("block", [1, 2, 3, 7, 16, 61, 64, 1000])
def test_blocks_that_cut_lines_names_and_crlf(harness, block):
    """fed in blocks (the caller carries the unconsumed tail) the map is the one-block map, line and record counts included"""
    for is_gtf, text in ((True, corpus.corner_gtf()), (False, corpus.corner_tsv()), (True, corpus.random_gtf(3)), (False, corpus.random_tsv(3))):
        assert harness.map(is_gtf, "gene_id", text, block_bytes=block) == harness.map(is_gtf, "gene_id", text)


def test_sanitized_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer and UBSan, over the corner corpus (host code only)"""
    exe = str(tmp_path / "gmap_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGMAP_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    gtf, tsv, rnd = tmp_path / "corner.gtf", tmp_path / "corner.tsv", tmp_path / "random.gtf"
    gtf.write_bytes(corpus.corner_gtf()); tsv.write_bytes(corpus.corner_tsv()); rnd.write_bytes(corpus.random_gtf(1))
    flagged = []
    for name, is_gtf, text, _ in corpus.flagged():
        p = tmp_path / (name + (".gtf" if is_gtf else ".tsv")); p.write_bytes(text); flagged.append((is_gtf, str(p)))
    for key in corpus.KEYS:
        r = subprocess.run([exe, "gtf", key, str(gtf), str(rnd)] + [p for g, p in flagged if g], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "corner.gtf flags=0" in r.stdout
    r = subprocess.run([exe, "tsv", "gene_id", str(tsv)] + [p for g, p in flagged if not g], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "corner.tsv flags=0" in r.stdout
