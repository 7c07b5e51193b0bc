"""csrc/bamwfmt.h alone (tests/bamwrite_harness.cpp, g++ -Wall -Wextra -Werror): the serial BAM record writer must give the records of
samfile.sam_to_bam(samfile._sam_text(...)) byte for byte, over every SamwLine branch and every rule of the header at its edges, and
name the lowest (read, record) of a batch BAM cannot say.  No GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bamwrite_corpus as corpus
from samwrite_corpus import arrays, variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "bamwrite_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p
_ARGS = [_P, _P, C.c_uint32, C.c_int, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, C.c_uint64, _P]


def _ptr(a):
    return None if a is None else a.ctypes.data


class Harness:
    def __init__(self, so):
        self.L = C.CDLL(so)
        self.L.bamw_harness_size.argtypes = _ARGS
        self.L.bamw_harness_format.argtypes = _ARGS
        self.L.bamw_harness_reg2bin.argtypes = [C.c_uint32, C.c_uint32]
        self.L.bamw_harness_reg2bin.restype = C.c_uint32

    def _call(self, fn, case, base, last):
        a = arrays(case)
        return fn(_ptr(a["hits"]), _ptr(a["offsets"]), len(a["offsets"]) - 1, int(case["paired"]), _ptr(a["ref"]), _ptr(a["ref_off"]),
                  len(case["names"]), _ptr(a["q"]), _ptr(a["q_off"]), _ptr(a["s1"]), _ptr(a["s1_off"]), _ptr(a["s2"]), _ptr(a["s2_off"]), base, last)

    def size(self, case, base=0):
        out = np.zeros(8, np.uint64)
        self._call(self.L.bamw_harness_size, case, base, out.ctypes.data)
        assert out[7] == 0, "bamw_unit_len and bamw_serial disagree"
        return dict(zip(("n_bytes", "n_lines", "n_units", "max_unit_bytes", "kind", "read", "record"), (int(x) for x in out[:7])))

    def records(self, case, base=0):
        res = self.size(case, base)
        assert res["kind"] == 0, res
        buf = np.full(res["n_bytes"] + 16, 0xAB, np.uint8)
        assert self._call(self.L.bamw_harness_format, case, base, buf.ctypes.data) == 0
        assert (buf[res["n_bytes"]:] == 0xAB).all()
        return buf[:res["n_bytes"]].tobytes(), res


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("bamw")), "libbamwrite_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    return Harness(so)


def sam_text(case, first_read=0):
    """the text of the case with case['paired'] in force, default names counted from first_read"""
    from sailfish_amd import samfile
    n = len(case["offsets"]) - 1
    seqs, names = case["seqs"], case["read_names"]
    if seqs is None and case["paired"]:
        seqs = [(b"*", b"*")] * n
    if names is None and first_read:
        names = [b"r%d" % (first_read + r) for r in range(n)]
    return samfile._sam_text(case["names"], case["ref_len"], case["hits"], case["offsets"], names, seqs)


def head_len(case):
    from sailfish_amd import samfile
    return len(samfile.sam_to_bam(samfile.sam_header(case["names"], case["ref_len"])))


def same_as_host(harness, case, base=0, back=True):
    """the statement against sam_to_bam for the case with and without names and bases; `back`: bam_to_sam leads back to the text
    (where the bases are upper-case IUPAC letters: BAM keeps neither case nor other bytes)"""
    from sailfish_amd import samfile
    skip = head_len(case)
    for v in variants(case):
        text = sam_text(v, base)
        want = samfile.sam_to_bam(text)
        got, res = harness.records(v, base)
        assert got == want[skip:]
        assert res["n_lines"] == text.count(b"\n") - text.count(b"\n@") - 1
        assert not back or samfile.bam_to_sam(want[:skip] + got) == text
    return got


def _records(data):
    out, p = [], 0
    while p < len(data):
        size = struct.unpack_from("<i", data, p)[0]
        out.append(data[p + 4:p + 4 + size]); p += 4 + size
    assert p == len(data)
    return out


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_corner_batch(harness, paired):
    from sailfish_amd import samfile
    case = corpus.corner(paired)
    hits, off = case["hits"], case["offsets"]
    assert {0, 1, 3} <= set(np.diff(off.astype(np.int64)).tolist())
    assert set(hits["mate_status"].tolist()) == ({1, 2, 3} if paired else {0}) and set(hits["fwd"].tolist()) == {0, 1}
    assert {0, -1, 2 ** 29 - 2 ** 16, 2 ** 29 - 50} <= set(hits["pos"].tolist()) and (hits["pos"] == -65534).any()
    assert not paired or {(f, m) for f, m in zip(hits["fwd"][hits["mate_status"] == 3], hits["mate_fwd"][hits["mate_status"] == 3])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {1, 254} <= {len(q) for q in case["read_names"]}
    assert {0, 1, 48, 49, 223, 9000, 65535} <= {len(s) for sq in case["seqs"] for s in (sq if paired else (sq,))}
    got = same_as_host(harness, case, back=False)          # (the variant without names and without bases comes last)
    assert struct.unpack_from("<I", got, 20)[0] == 0 and got[36:39] == b"r0\0"
    same_as_host(harness, case, base=999_999_999_990, back=False)
    # what the first variant's records say: a bin at every level and bin 0, 4680 and pos -1 when unmapped, both nibble orders
    recs = _records(harness.records(case)[0])
    fields = [struct.unpack_from("<iiBBHHHIiii", r) for r in recs]
    bins = {f[4] for f in fields}
    assert {4680, 0} <= bins and all(any(lo <= b < hi for b in bins) for lo, hi in ((1, 9), (9, 73), (73, 585), (585, 4681), (4681, 37450)))
    assert all((f[1] == -1) == (f[0] == -1) == (f[4] == 4680 and f[5] == 0) for f in fields) and {0, 1, 2} == {f[5] for f in fields}
    assert all(f[3] == 255 for f in fields)
    odd = next(r for r, f in zip(recs, fields) if f[7] == 223)
    q = 32 + odd[8] + 4 * struct.unpack_from("<H", odd, 12)[0]
    packed = odd[q:q + 112]
    want = bytes(samfile._BASE_CODE.get(c, 15) for c in corpus.ODD_BASES.upper())
    assert [b >> 4 for b in packed] == list(want[0::2]) and [b & 15 for b in packed[:-1]] == list(want[1::2]) and packed[-1] & 15 == 0
    assert set(want) == set(range(16)) and odd[q + 112:] == b"\xff" * 223


def test_reg2bin_is_the_specification_s(harness):
    from sailfish_amd import samfile
    for beg, want in zip(corpus.BIN_STARTS, corpus.BIN_WANT):
        assert harness.L.bamw_harness_reg2bin(beg, beg + 50) == samfile._reg2bin(beg, beg + 50)
        assert (want == 0) == (harness.L.bamw_harness_reg2bin(beg, beg + 50) == 0)
    rng = np.random.default_rng(5)
    for _ in range(2000):
        beg = int(rng.integers(0, 2 ** 29 - 1))
        end = min(2 ** 29, beg + int(rng.choice([1, 2, 50, 70000, 2 ** 20, 2 ** 27])))
        assert harness.L.bamw_harness_reg2bin(beg, end) == samfile._reg2bin(beg, end)
    assert harness.L.bamw_harness_reg2bin(2 ** 29 - 1, 2 ** 29) == 4681 + 32767


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_random_corpus(harness, paired):
    case = corpus.case(paired, n_reads=400, seed=3)
    assert len(case["hits"]) > 400
    same_as_host(harness, case, base=95)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_batches_bam_cannot_say(harness, paired):
    """every case names its lowest (read, record) and the first kind that record breaks; sam_to_bam refuses kinds 3 and 4 too, but for
    an unmapped SEQ above 65 535 bases (it has no rule for 5 either: a position beyond 2^29 gets a bin of the wrong level there)"""
    from sailfish_amd import samfile
    cases = corpus.failing(paired)
    assert {c[3] for c in cases} == {1, 2, 3, 4, 5}
    for case, read, record, kind in cases:
        res = harness.size(case)
        assert (res["kind"], res["read"], res["record"]) == (kind, read, record)
        unmapped = case["offsets"][read] == case["offsets"][read + 1]
        if kind == 3 or (kind == 4 and not unmapped):      # (sam_to_bam packs an unmapped SEQ of any length; l_seq of a read is 16 bits here)
            with pytest.raises(ValueError):
                samfile.sam_to_bam(sam_text(case))
    assert set(samfile.BAM_WRITE_KINDS) == {3, 4, 5} and not set(samfile.BAM_WRITE_KINDS) & set(samfile.WRITE_KINDS)
    # without the names given the default ones fit, without the bases nothing differs: kinds 3 and 4 need what they speak of
    case = cases[0][0]
    assert harness.size(dict(case, read_names=None))["kind"] == 4 and harness.size(dict(case, read_names=None, seqs=None))["kind"] == 0


def test_empty_batches(harness):
    from sailfish_amd import samfile
    names, ref_len = corpus._transcripts()
    for paired in (True, False):
        none = dict(names=names, ref_len=ref_len, hits=np.zeros(0, corpus.HIT_DTYPE), offsets=np.zeros(1, np.uint32), paired=paired, read_names=[], seqs=[])
        assert harness.records(none)[0] == b""
        seqs = [b"ACG", b"T", b"N", b"ACGTN", b"A" * 50]
        unmapped = dict(none, offsets=np.zeros(6, np.uint32), read_names=[b"a", b"b", b"c c", b"d" * 70, b"e"],
                        seqs=[(s, s[::-1]) for s in seqs] if paired else seqs)
        same_as_host(harness, unmapped)
