"""The name blob and the mate-name rule of the device read parser (sailfish_amd/csrc/readfmt.h: rf_blob_record, rf_mate_stem_len,
rf_mates_agree) compiled as plain C++ with g++ (tests/readnames_harness.cpp; nothing but libstdc++ is linked), judged by the
record-by-record restatement of tests/test_readfile_cpu.py (its names) and by readfile.mate_stem.  The same source runs once more as
a stand-alone program under AddressSanitizer and UBSan.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import readnames_corpus as corpus
from test_readfile_cpu import ERR_RANGE, FASTA, FASTQ, OK, Result, random_texts, restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "readnames_harness.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "sailfish_amd", "csrc")]
ERR_INVALID = 1
NONE = 2 ** 64 - 1


def build_harness(dirpath):
    so = os.path.join(str(dirpath), "libreadnames_harness.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC"] + FLAGS + [SRC, "-o", so])
    return so


def round16(n):
    return (n + 15) & ~15


class NamesHarness:
    def __init__(self, so):
        L = C.CDLL(so)
        self.fn = L.readnames_harness_parse
        self.fn.restype = C.c_int
        self.fn.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                            C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(Result)]
        self.match_fn = L.readnames_harness_match
        self.match_fn.restype = C.c_uint64
        self.match_fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        self.stem_fn = L.readnames_harness_stem_len
        self.stem_fn.restype = C.c_uint64
        self.stem_fn.argtypes = [C.c_char_p, C.c_uint64]

    def parse(self, text, final, max_reads=1 << 40, cap_bases=1 << 40, cap_names=None, misalign=0):
        """-> dict(rc, n_reads, consumed, names, name_off, blob, n_name_bytes, spans)"""
        text = bytes(text)
        n = len(text)
        cap_names = max(round16(n), 16) if cap_names is None else cap_names
        bases = np.zeros(n + 1, np.uint8); off = np.zeros(n + 2, np.int64); span = np.zeros(2 * n + 2, np.uint64)
        room = np.zeros(cap_names + 32, np.uint8)
        at = (-room.ctypes.data) % 16 + misalign              # a 16-byte boundary inside the array (+ misalign)
        name_off = np.full(n + 2, 77, np.uint64)
        n_name = C.c_uint64(99)
        res = Result()
        rc = self.fn(text, n, int(final), max_reads, bases.ctypes.data, cap_bases, off.ctypes.data, span.ctypes.data, room.ctypes.data + at,
                     cap_names, name_off.ctypes.data, C.byref(n_name), C.byref(res))
        R, nb = int(res.n_reads), int(n_name.value)
        o = name_off[: R + 1].astype(np.int64) if rc == OK else np.zeros(1, np.int64)
        blob = room[at:at + nb].tobytes()
        return dict(rc=rc, n_reads=R, consumed=int(res.consumed), n_name_bytes=nb, name_off=o.tolist(), blob=blob,
                    names=[blob[o[r]:o[r + 1]] for r in range(R)] if rc == OK else [], pad=room[at + nb:at + round16(nb)].tobytes(),
                    spans=[(int(span[2 * r]), int(span[2 * r + 1])) for r in range(R)])

    def match(self, names1, names2):
        (b1, o1), (b2, o2) = corpus.blob_of(names1), corpus.blob_of(names2)
        a1, a2 = np.frombuffer(b1 + b"\0", np.uint8), np.frombuffer(b2 + b"\0", np.uint8)
        first = self.match_fn(a1.ctypes.data, o1.ctypes.data, a2.ctypes.data, o2.ctypes.data, len(names1))
        return None if first == NONE else int(first)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return NamesHarness(build_harness(tmp_path_factory.mktemp("rnh")))


def judge(got, text, final, max_reads=1 << 40, cap_bases=1 << 40, what=""):
    """the harness' blob against the names of the restatement"""
    want = restate(text, final, max_reads, cap_bases)
    assert got["rc"] == want["rc"], (what, got["rc"], want["rc"])
    if want["rc"] != OK:
        assert got["n_reads"] == 0 and got["consumed"] == 0 and got["n_name_bytes"] == 0, what
        return want
    b, o = corpus.blob_of(want["names"])
    assert got["names"] == want["names"] and got["blob"] == b and got["name_off"] == o.tolist(), what
    assert got["n_name_bytes"] == len(b) and got["consumed"] == want["consumed"] and got["spans"] == want["spans"], what
    assert got["pad"] == bytes(len(got["pad"])), what
    return want


def expected_first(names1, names2):
    from sailfish_amd import readfile
    return next((r for r, (a, b) in enumerate(zip(names1, names2)) if readfile.mate_stem(a) != readfile.mate_stem(b)), None)


def test_harness_links_nothing_else(tmp_path):
    so = build_harness(tmp_path)
    needed = re.findall(r"NEEDED.*\[(.*?)\]", subprocess.check_output(["readelf", "-d", so], text=True))
    assert needed and all(n.startswith(("libstdc++", "libm.", "libgcc_s", "libc.")) for n in needed), needed


def test_corpus_holds_what_it_should():
    """group starts inside, at the start of and at the end of names; the three totals; CRLF name-only headers"""
    _, off = corpus.blob_of([b"x" * ln for ln in corpus.ORDER])
    starts = set(off[1:-1].tolist())
    groups = set(range(16, int(off[-1]), 16))
    assert groups & starts and groups - starts and 0 in corpus.ORDER and set(corpus.LENS) <= set(corpus.ORDER)
    cases = {label: (text, names) for label, text, names in corpus.gather_cases()}
    for total in (4095, 4096, 4097):
        for fmt in ("fastq", "fasta"):
            assert sum(len(n) for n in cases[f"{fmt}_total_{total}"][1]) == total
    assert b"\r\n" in cases["fastq_alone_crlf"][0] and not cases["fasta_header_only_last_line"][0].endswith(b"\n")


def test_blob_of_the_listed_cases(harness):
    for label, text, names in corpus.gather_cases():
        got = harness.parse(text, 1)
        want = judge(got, text, 1, what=label)
        assert want["names"] == names and not any(b"\r" in n for n in got["names"]), label
        judge(harness.parse(text, 0), text, 0, what=label)
        for cut in (len(text) - 1, len(text) // 2):
            for final in (0, 1):
                judge(harness.parse(text[:cut], final), text[:cut], final, what=(label, cut, final))      # (a cut FASTQ record is TRUNCATED when final: nothing is emitted)


def test_cuts_and_capacity(harness):
    label, text, names = next(c for c in corpus.gather_cases() if c[0] == "fastq_mixed")
    for max_reads, cap in ((5, 1 << 40), (1 << 40, 60), (1, 1 << 40), (0, 0)):
        got = harness.parse(text, 1, max_reads, cap)
        want = judge(got, text, 1, max_reads, cap, what=(max_reads, cap))
        assert len(want["names"]) < len(names)                # only the emitted records' names
    total = sum(len(n) for n in names)
    assert harness.parse(text, 1, cap_names=round16(total))["names"] == names
    r = harness.parse(text, 1, cap_names=round16(total) - 16)
    assert r["rc"] == ERR_RANGE and r["n_reads"] == 0 and r["consumed"] == 0 and r["n_name_bytes"] == 0
    assert harness.parse(text, 1, misalign=4)["rc"] == ERR_INVALID
    assert harness.parse(text, 1, cap_names=round16(total) + 8)["rc"] == ERR_INVALID


@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_random_texts_match_the_restatement(harness, fmt):
    for text, seqs, names in random_texts(fmt, count=150, seed=31):
        assert judge(harness.parse(text, 1), text, 1, what=text)["names"] == names
        for final in (0, 1):
            for cut in (len(text) // 3, len(text) - 1):
                for max_reads, cap in ((1 << 40, 1 << 40), (2, 1 << 40), (1 << 40, 50)):
                    judge(harness.parse(text[:cut], final, max_reads, cap), text[:cut], final, max_reads, cap, what=(text[:cut], final))


def test_stem_rule(harness):
    from sailfish_amd import readfile
    rng = np.random.default_rng(41)
    names = [b"", b"/", b"/1", b"/2", b"/3", b"1", b"a", b"a/1", b"a/2", b"a/3", b"a/12", b"a/1/2", b"a//1", b"a/1 ", b"ab/", b"/1/1"]
    names += [bytes(rng.choice(np.frombuffer(b"a/123", np.uint8), int(rng.integers(0, 7)))) for _ in range(300)]
    for nm in names:
        assert harness.stem_fn(nm, len(nm)) == len(readfile.mate_stem(nm)) and nm.startswith(readfile.mate_stem(nm)), nm
    assert readfile.mate_stem(b"x/1") == readfile.mate_stem(b"x/2") == readfile.mate_stem(b"x") == b"x"
    assert readfile.mate_stem(b"x/3") == b"x/3" and readfile.mate_stem(b"/1") == b""


def test_match_cases(harness):
    seen = set()
    for label, n1, n2 in corpus.match_cases():
        want = expected_first(n1, n2)
        assert harness.match(n1, n2) == want, label
        seen.add(want)
    assert {None, 0, 3, 130, 66} <= seen
    rng = np.random.default_rng(43)
    for _ in range(300):                                      # short names over a tiny alphabet: every kind of near miss
        n = int(rng.integers(0, 6))
        n1 = [bytes(rng.choice(np.frombuffer(b"a/12", np.uint8), int(rng.integers(0, 5)))) for _ in range(n)]
        n2 = [nm if rng.integers(0, 2) else bytes(rng.choice(np.frombuffer(b"a/12", np.uint8), int(rng.integers(0, 5)))) for nm in n1]
        assert harness.match(n1, n2) == expected_first(n1, n2), (n1, n2)


def _parse_case(path, text, final, max_reads, cap_bases, cap_names):
    with open(path, "wb") as f:
        f.write(np.array([0, len(text), final, min(max_reads, 1 << 62), min(cap_bases, 1 << 62), cap_names], np.uint64).tobytes() + text)


def _match_case(path, n1, n2):
    (b1, o1), (b2, o2) = corpus.blob_of(n1), corpus.blob_of(n2)
    with open(path, "wb") as f:
        f.write(np.array([1, len(n1), len(b1), len(b2)], np.uint64).tobytes() + o1.tobytes() + o2.tobytes() + b1 + b2)


def test_sanitized_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer and UBSan, over the same cases (host code only); its
    buffers are exactly as large as the contract says"""
    exe = str(tmp_path / "readnames_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DREADNAMES_HARNESS_MAIN"] + FLAGS + [SRC, "-o", exe])
    parses, matches = [], []
    texts = [(label, text) for label, text, _ in corpus.gather_cases()]
    texts += [(f"random{fmt}_{i}", text) for fmt in (FASTA, FASTQ) for i, (text, _, _) in enumerate(random_texts(fmt, count=60, seed=31))]
    for label, text in texts:
        for final in (0, 1):
            for k, (max_reads, cap) in enumerate(((1 << 40, 1 << 40), (3, 1 << 40), (1 << 40, 50))):
                for cut in (len(text), len(text) - 1, len(text) // 2):
                    want = restate(text[:cut], final, max_reads, cap)
                    total = sum(len(n) for n in want["names"])
                    for cap_names in {round16(total), max(round16(total) - 16, 0)}:
                        p = str(tmp_path / f"{label}.{final}.{k}.{cut}.{cap_names}")
                        _parse_case(p, text[:cut], final, max_reads, cap, cap_names)
                        parses.append((p, want, total, cap_names))
    for label, n1, n2 in corpus.match_cases():
        p = str(tmp_path / f"match_{label}")
        _match_case(p, n1, n2)
        matches.append((p, expected_first(n1, n2)))
    files = [p for p, *_ in parses] + [p for p, _ in matches]
    for a in range(0, len(files), 500):
        r = subprocess.run([exe] + files[a:a + 500], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for p, want, total, cap_names in parses:
        out = open(p + ".out", "rb").read()
        w = np.frombuffer(out[:40], np.uint64)
        if want["rc"] != OK or total > cap_names:
            assert int(w[0]) == (want["rc"] if want["rc"] != OK else ERR_RANGE) and w[1] == 0 and w[3] == 0 and w[4] == 0, p
            continue
        R = len(want["names"])
        b, o = corpus.blob_of(want["names"])
        assert w.tolist() == [OK, R, sum(len(s) for s in want["seqs"]), want["consumed"], total], p
        assert np.array_equal(np.frombuffer(out[40:40 + 8 * (R + 1)], np.uint64), o.astype(np.uint64)) and out[40 + 8 * (R + 1):] == b, p
    for p, want in matches:
        assert int(np.frombuffer(open(p + ".out", "rb").read(), np.uint64)[0]) == (NONE if want is None else want), p
