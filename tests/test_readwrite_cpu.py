"""The FASTA / FASTQ text of the device read writer as csrc/readwfmt.h states it (the functions readtext_write.hip runs inside its
kernels), compiled as plain C++ with g++ -Wall -Wextra -Werror (tests/readwrite_harness.cpp; nothing but libstdc++ is linked) and
judged by the host statement, readfile.reads_text_host: bytes, sizes, and the lowest (record, kind) of every batch that cannot be
written.  The text is then read back by the record rules of csrc/readfmt.h as tests/test_readfile_cpu.py restates them.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import readwrite_corpus as corpus
from test_readfile_cpu import restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "readwrite_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p
_ARGS = [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, _P, _P]


def _ptr(a):
    return None if a is None else a.ctypes.data


class Harness:
    def __init__(self, so):
        self.L = C.CDLL(so)
        self.L.readw_harness_size.argtypes = _ARGS
        self.L.readw_harness_format.argtypes = _ARGS

    def _call(self, fn, case, last):
        a = corpus.arrays(case)
        return fn(_ptr(a["bases"]), _ptr(a["off"]), a["n"], _ptr(a["qual"]), _ptr(a["names"]), _ptr(a["name_off"]), case["base"], _ptr(a["select"]), last)

    def size(self, case):
        """-> dict(n_selected, n_bytes, max_record_bytes, kind, record)"""
        out = np.zeros(6, np.uint64)
        kind = self._call(self.L.readw_harness_size, case, out.ctypes.data)
        assert out[5] == 0, "readw_record_len and readw_serial disagree"
        assert kind == out[3]
        return dict(zip(("n_selected", "n_bytes", "max_record_bytes", "kind", "record"), (int(x) for x in out[:5])))

    def text(self, case):
        res = self.size(case)
        assert res["kind"] == 0
        buf = np.full(res["n_bytes"] + 16, 0xAB, np.uint8)
        assert self._call(self.L.readw_harness_format, case, buf.ctypes.data) == 0
        assert (buf[res["n_bytes"]:] == 0xAB).all()
        return buf[:res["n_bytes"]].tobytes(), res


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("readw")), "libreadwrite_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    needed = re.findall(r"NEEDED.*\[(.*?)\]", subprocess.check_output(["readelf", "-d", so], text=True))
    assert all(re.match(r"lib(stdc\+\+|m|gcc_s|c)\.so", n) for n in needed), needed
    return Harness(so)


def same_as_host(harness, case):
    """the harness against the statement: the bytes, or the error -> the bytes or None"""
    if case["error"] is not None:
        res = harness.size(case)
        assert (res["record"], res["kind"]) == case["error"], case["label"]
        with pytest.raises(ValueError) as e:
            corpus.expected(case)
        assert str(e.value).startswith(f"record {case['error'][0]}: ") and str(e.value).endswith(f"(kind {case['error'][1]})"), case["label"]
        return None
    want = corpus.expected(case)
    got, res = harness.text(case)
    assert got == want, case["label"]
    recs = corpus.selected(case)
    assert res["n_selected"] == len(recs)
    assert res["max_record_bytes"] == max([corpus.record_len(len(n), len(s), q is not None) for n, s, q in recs], default=0)
    return want


def reads_back(case, text):
    """readfmt.h's rules (final = 1) give back the selected records"""
    recs = corpus.selected(case)
    got = restate(text, 1)
    assert got["rc"] == 0, case["label"]
    assert got["names"] == [n for n, _, _ in recs] and got["seqs"] == [s for _, s, _ in recs], case["label"]
    if recs:
        assert got["format"] == (1 if case["quals"] is None else 2) and got["consumed"] == len(text)
    if case["quals"] is not None:                          # the restatement keeps no qualities: they are the fourth lines
        lines = text.split(b"\n")
        assert lines[3::4] == [q for _, _, q in recs] and lines[-1] == b""


def test_corpus_matches_the_statement(harness):
    cases = corpus.cases()
    for case in cases:
        text = same_as_host(harness, case)
        if text is not None:
            reads_back(case, text)
    assert sum(c["error"] is not None for c in cases) >= 20


def test_random_batches(harness):
    seen = set()
    for i in range(corpus.N_RANDOM):
        case = corpus.random_case(i)
        reads_back(case, same_as_host(harness, case))
        seen.add((case["quals"] is None, case["names"] is None, case["select"] is None, case["misaligned"], len(case["seqs"]) == 0))
    assert {k[:3] for k in seen} == {(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)}
    assert any(k[3] for k in seen) and any(k[4] for k in seen)


def test_awkward_texts_read_back():
    """the texts the issue names: each comes back as one record"""
    from sailfish_amd.readfile import reads_text_host
    assert reads_text_host([b""], [b""], [b"a"]) == b"@a\n\n+\n\n"
    assert reads_text_host([b""], None, [b"a"]) == b">a\n\n"
    for text, names, seqs in ((b"@a\n\n+\n\n", [b"a"], [b""]), (b">a\n\n", [b"a"], [b""]), (b">a\n", [b"a"], [b""]), (b">\nAC\n", [b""], [b"AC"]),
                              (b"@\nAC\n+\nII\n", [b""], [b"AC"])):
        got = restate(text, 1)
        assert (got["rc"], got["names"], got["seqs"]) == (0, names, seqs), text
    for fastq in (False, True):                            # a 0-base record first, last, and both
        for seqs in ([b"", b"ACG"], [b"ACG", b""], [b"", b"A", b""], [b"", b""]):
            quals = [b"I" * len(s) for s in seqs] if fastq else None
            names = [b"n%d" % i for i in range(len(seqs))]
            got = restate(reads_text_host(seqs, quals, names), 1)
            assert (got["rc"], got["names"], got["seqs"]) == (0, names, seqs)


def test_statement_options():
    from sailfish_amd.readfile import WRITE_KINDS, reads_text_host
    assert reads_text_host([b"AC", b"G"], index_base=9) == b">r9\nAC\n>r10\nG\n"
    assert reads_text_host([b"AC", b"G"], [b"#I", b"!"], select=[0, 1], index_base=2 ** 32 + 5) == b"@r4294967302\nG\n+\n!\n"
    assert reads_text_host([], [], []) == b"" and reads_text_host([b"A\rC"], None, [b"x\ry"]) == b">x\ry\nA\rC\n"
    assert set(WRITE_KINDS) == {1, 2, 3, 4}
    with pytest.raises(ValueError, match=r"^record 1: .*\(kind 3\)$"):
        reads_text_host([b"A", b"C"], [b"I", b"\n"])
    assert reads_text_host([b"A", b"C"], [b"I", b"\n"], select=[1, 0]) == b"@r0\nA\n+\nI\n"


def _tiles_of(case):
    """[(first byte, bytes, name length, bases)] of the selected records in the text"""
    out, pos = [], 0
    for n, s, q in corpus.selected(case):
        ln = corpus.record_len(len(n), len(s), q is not None)
        out.append((pos, ln, len(n), len(s)))
        pos += ln
    return out


def test_corpus_holds_what_it_should():
    """the corpus reaches the edges it names"""
    by = {c["label"]: c for c in corpus.cases()}
    T = corpus.TILE
    for tag in ("fasta", "fastq"):
        for end in (T - 1, T, T + 1):
            recs = _tiles_of(by[f"end_{end}.{tag}"])
            assert len(recs) == 2 and recs[0][1] == end
        runs = by[f"runs.{tag}"]
        assert tuple(len(n) for n in runs["names"]) == corpus.NAME_RUNS and {len(s) for s in runs["seqs"]} == set(corpus.BASE_RUNS)
        tiny = _tiles_of(by[f"tiny.{tag}"])
        assert {r[1] for r in tiny} == ({6} if tag == "fastq" else {3}) and sum(1 for r in tiny if r[0] < T) > 256 and len(tiny) * tiny[0][1] > T
        sel = {k: by[f"select_{k}.{tag}"]["select"] for k in ("all", "none", "first", "last", "alternate", "far", "sparse")}
        assert all(sel["all"]) and not any(sel["none"]) and sel["first"][0] and sum(sel["first"]) == 1 and sel["last"][-1] and sum(sel["last"]) == 1
        assert sel["alternate"][:4] == [0, 1, 0, 1]
        assert sel["far"] == [1] + [0] * 5000 + [1] and sum(sel["sparse"]) * 100 == len(sel["sparse"]) >= 3000
        for base in corpus.INDEX_BASES:
            c = by[f"generated_names_{base}.{tag}"]
            assert c["names"] is None and c["base"] == base
        assert len({len(str(by[f"generated_names_9.{tag}"]["base"] + r)) for r in range(12)}) == 2          # across a digit edge
        mis = by[f"misaligned.{tag}"]
        a = corpus.arrays(mis)
        assert all(a[k].ctypes.data % 2 == 1 for k in ("bases", "names", "select")) and all(a[k].ctypes.data % 16 == 8 for k in ("off", "name_off"))
        assert tag == "fasta" or a["qual"].ctypes.data % 2 == 1
    big = [r for r in _tiles_of(by["runs.fastq"]) if r[3] == 10_000]
    assert len(big) == 1 and (big[0][0] + big[0][1] - 1) // T - big[0][0] // T == 5                           # six tiles
    for k in range(4):                                     # the second tile begins with byte k of \n+\n, or with the next '@'
        text = corpus.expected(by[f"plus_straddle_{k}.fastq"])
        assert text[T - k:T - k + 3] == b"\n+\n" if k < 3 else text[T - 1:T + 1] == b"\n@"
        assert len(_tiles_of(by[f"plus_straddle_{k}.fastq"])) == 3
    errs = {c["error"][1] for c in by.values() if c["error"] is not None}
    assert errs == {1, 2, 3, 4}
    assert by["error_two_records.fasta"]["error"] == (5, 2) and by["error_two_kinds.fastq"]["error"] == (12, 1)
    assert by["error_kind2_unselected.fastq"]["error"] is None and b"\n" in by["error_kind2_unselected.fastq"]["seqs"][17]
    assert b"\r" in by["carriage_return.fastq"]["seqs"][9] and b"\r" in corpus.expected(by["carriage_return.fastq"])
    assert max(len(corpus.expected(c)) for c in by.values() if c["error"] is None) < 300_000


def _case_file(path, case):
    a = corpus.arrays(dict(case, misaligned=False))
    n_bases = int(a["off"][-1])
    n_names = 0 if a["name_off"] is None else int(a["name_off"][-1])
    head = np.array([a["n"], a["qual"] is not None, a["names"] is not None, a["select"] is not None, case["base"], n_bases, n_names], np.uint64)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        f.write(a["off"].tobytes())
        f.write(a["bases"][:n_bases].tobytes())
        if a["qual"] is not None:
            f.write(a["qual"][:n_bases].tobytes())
        if a["names"] is not None:
            f.write(a["name_off"].tobytes())
            f.write(a["names"][:n_names].tobytes())
        if a["select"] is not None:
            f.write(a["select"][:a["n"]].tobytes())


def test_sanitized_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer and UBSan, over the same cases, with buffers exactly as large
    as the contract says (host code only)"""
    exe = str(tmp_path / "readwrite_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DREADW_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    good, bad = [], []
    for i, case in enumerate(corpus.cases() + [corpus.random_case(i) for i in range(corpus.N_RANDOM)]):
        p = str(tmp_path / f"case{i}")
        _case_file(p, case)
        if case["error"] is None:
            good.append((p, corpus.expected(case), len(corpus.selected(case))))
        else:
            bad.append((p,) + case["error"])
    r = subprocess.run([exe] + [g[0] for g in good] + [b[0] for b in bad], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("\n") == len(good) + len(bad) and " mismatch=1" not in r.stdout
    for p, want, n_sel in good:
        assert re.search(rf"^{re.escape(p)} kind=0 selected={n_sel} bytes={len(want)} ", r.stdout, re.M), p
        with open(p + ".out", "rb") as f:
            assert f.read() == want, p
    for p, record, kind in bad:
        assert re.search(rf"^{re.escape(p)} kind={kind} record={record} ", r.stdout, re.M), p
