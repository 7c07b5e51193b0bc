"""Qualities and orientation in the SAM / BAM writer's rules (csrc/samwfmt.h, csrc/bamwfmt.h) as plain C++
(tests/samqual_harness.cpp, g++ -Wall -Wextra -Werror), judged by the host statement samfile._sam_text(..., quals=, oriented=) and
sam_to_bam of it; the host statement in turn by a transform of the plain text written in tests/samqual_corpus.py.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bamwrite_corpus as bw
import samqual_corpus as corpus
import samwrite_corpus as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "samqual_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p


def _ptr(a):
    return None if a is None else a.ctypes.data


class Harness:
    def __init__(self, so):
        self.L = C.CDLL(so)
        self.L.samq_harness.argtypes = [C.c_int, _P, _P, C.c_uint32, C.c_int, _P, _P, C.c_uint32] + [_P] * 8 + [C.c_int, C.c_uint64, _P, _P]
        self.L.samq_comp.argtypes, self.L.samq_comp.restype = [C.c_uint8], C.c_uint8

    def run(self, case, quals, oriented, bam=False, base=0, write=True):
        """-> (dict(n_bytes, n_lines, n_units, max_unit_bytes, kind, read, record), bytes or None)"""
        a = corpus.arrays(case)
        args = lambda out, buf: (int(bam), _ptr(a["hits"]), _ptr(a["offsets"]), len(a["offsets"]) - 1, int(case["paired"]), _ptr(a["ref"]),
                                 _ptr(a["ref_off"]), len(case["names"]), _ptr(a["q"]), _ptr(a["q_off"]), _ptr(a["s1"]), _ptr(a["s1_off"]),
                                 _ptr(a["s2"]), _ptr(a["s2_off"]), _ptr(a["k1"]) if quals else None, _ptr(a["k2"]) if quals else None,
                                 int(oriented), base, out.ctypes.data, buf)
        out = np.zeros(8, np.uint64)
        kind = self.L.samq_harness(*args(out, None))
        assert out[7] == 0, "the per-unit sizes and the serial pass disagree"
        res = dict(zip(("n_bytes", "n_lines", "n_units", "max_unit_bytes", "kind", "read", "record"), (int(x) for x in out[:7])))
        if kind or not write:
            return res, None
        buf = np.full(res["n_bytes"] + 16, 0xAB, np.uint8)
        assert self.L.samq_harness(*args(out, buf.ctypes.data)) == 0 and out[7] == 0
        assert (buf[res["n_bytes"]:] == 0xAB).all()
        return res, buf[:res["n_bytes"]].tobytes()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("samq")), "libsamqual_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    return Harness(so)


def text_cases(paired):
    """(name, case, first read) for the text: the existing corpus dressed, and the reversed runs"""
    out = [("corner", corpus.dress(sw.corner(paired), 1), 0), ("random", corpus.dress(sw.random_case(0, paired), 2), 95),
           ("runs", corpus.reversed_runs(paired), 0)]
    if paired:
        out += [("mate1", corpus.only(out[2][1], 0), 0), ("mate2", corpus.only(corpus.dress(sw.random_case(1, paired), 3), 1), 7)]
    return out


def bam_cases(paired):
    names, ref_len = bw._transcripts()
    out = [("corner", corpus.dress(bw.corner(paired), 4), 0), ("random", corpus.dress(bw.case(paired, 300), 5), 0),
           ("runs", corpus.reversed_runs(paired, names, ref_len), 0)]
    if paired:
        out += [("mate1", corpus.only(out[2][1], 0), 0), ("mate2", corpus.only(out[1][1], 1), 0)]
    return out


def test_complement_table(harness):
    from sailfish_amd import samfile
    for table in (corpus.COMP, samfile._COMP):
        assert bytes(harness.L.samq_comp(c) for c in range(256)) == bytes(range(256)).translate(table)
    assert corpus.COMP[ord("U")] == ord("A") and corpus.COMP[ord("u")] == ord("a")
    for c in b"SWNswn*=.-@\t\n":
        assert corpus.COMP[c] == c


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_corpus_holds_what_it_should(paired):
    runs = corpus.reversed_runs(paired)
    hits = runs["hits"]
    lens = {len(x) for s in runs["seqs"] for x in (s if paired else (s,))}
    assert set(corpus.RUNS) <= lens and {n % 2 for n in lens} == {0, 1}
    assert 0 in np.diff(runs["offsets"].astype(np.int64))                      # record-less reads
    assert (np.diff(runs["offsets"].astype(np.int64)) > 1).any()               # secondary records
    if paired:
        pairs = hits[hits["mate_status"] == 3]
        assert {(int(f), int(m)) for f, m in zip(pairs["fwd"], pairs["mate_fwd"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert ((hits["mate_status"] == 1) & (hits["fwd"] == 0)).any() and ((hits["mate_status"] == 2) & (hits["fwd"] == 0)).any()
    dressed = corpus.dress(sw.corner(paired), 1)
    seen = set(b"".join(x for s in dressed["seqs"] for x in (s if paired else (s,))))
    assert seen == set(corpus.BASES.tolist())
    assert set(b"".join(x for k in dressed["quals"] for x in (k if paired else (k,)))) == set(range(33, 127))


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_host_statement_is_the_transformed_plain_text(paired):
    """_sam_text(quals=, oriented=) against the transform; without either it is the text it always was"""
    from sailfish_amd import samfile
    for name, case, base in text_cases(paired):
        for quals, oriented in corpus.MODES:
            got = corpus.expected(case, quals, oriented, base)
            assert got == corpus.transformed(case, quals, oriented, base), (name, quals, oriented)
        old = samfile._sam_text(case["names"], case["ref_len"], case["hits"], case["offsets"], case["read_names"], case["seqs"])
        assert old == corpus.expected(case, False, False, header=True)
        if name == "runs":
            flags = np.array([int(l.split(b"\t")[1]) for l in got.splitlines()])
            assert (flags & 0x10).any() and (flags & 0x100).any() and corpus.expected(case, True, True, base) != corpus.expected(case, True, False, base)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_text_is_the_host_statement(harness, paired):
    for name, case, base in text_cases(paired):
        for v in (case, dict(case, read_names=None)):
            for quals, oriented in corpus.MODES:
                want = corpus.expected(v, quals, oriented, base)
                res, got = harness.run(v, quals, oriented, base=base)
                assert got == want, (name, quals, oriented)
                assert res["n_lines"] == want.count(b"\n") and res["kind"] == 0


def _bam_roundtrip_text(text):
    """what bam_to_sam gives back for the text: bases through the 16 codes, an empty SEQ as '*' with QUAL '*'"""
    keep = bytes(c if c in b"=ACMGRSVTWYHKDBN" else ord("N") for c in range(256))
    out = []
    for l in text.splitlines():
        if l.startswith(b"@"):
            out.append(l)
            continue
        f = l.split(b"\t")
        f[9] = f[9].upper().translate(keep) or b"*"
        if f[9] == b"*":
            f[10] = b"*"
        out.append(b"\t".join(f))
    return b"\n".join(out) + b"\n"


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_records_are_sam_to_bam_of_the_host_statement(harness, paired):
    from sailfish_amd import samfile
    for name, case, base in bam_cases(paired):
        head = samfile.sam_to_bam(samfile.sam_header(case["names"], case["ref_len"]))
        for quals, oriented in corpus.MODES:
            text = corpus.expected(case, quals, oriented, base, header=True)
            want = samfile.sam_to_bam(text)
            res, got = harness.run(case, quals, oriented, bam=True, base=base)
            assert res["kind"] == 0 and head + got == want, (name, quals, oriented)
            lines = samfile.sam_header(case["names"], case["ref_len"]) + corpus.transformed(case, quals, oriented, base)
            assert samfile.bam_to_sam(want) == _bam_roundtrip_text(lines), (name, quals, oriented)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_quality_bytes_that_cannot_be_written(harness, paired):
    from sailfish_amd import samfile
    cases = corpus.failing(paired)
    assert {c[3] for c in cases} == {1, 2, 6}
    for case, read, record, kind in cases:
        for bam in (False, True):
            for oriented in (False, True):
                res, got = harness.run(case, True, oriented, bam=bam)
                assert got is None and (res["kind"], res["read"], res["record"]) == (kind, read, record)
        with pytest.raises(IndexError if kind == 2 else ValueError) as e:
            corpus.expected(case, True, False)
        if kind != 2:
            assert str(e.value).startswith(f"read {read}, record {record}: ")
            assert (samfile.QUAL_WRITE_KINDS[6] in str(e.value)) == (kind == 6)
        if kind == 6:                                      # without the qualities the rule is not in force
            assert harness.run(case, False, True)[0]["kind"] in (0, 1)
    assert set(samfile.QUAL_WRITE_KINDS) == {6}
    # 32 and 127 are the edges: 33 and 126 pass
    case = cases[0][0]
    fine = dict(case, quals=[tuple(b"!~~!" for _ in k) if paired else b"!~~!" for k in case["quals"]])
    assert harness.run(fine, True, True)[0]["kind"] == 0


def test_qualities_without_bases(harness):
    from sailfish_amd import samfile
    case = corpus.reversed_runs(False)
    a = corpus.arrays(case)
    out = np.zeros(8, np.uint64)
    rc = harness.L.samq_harness(0, _ptr(a["hits"]), _ptr(a["offsets"]), len(a["offsets"]) - 1, 0, _ptr(a["ref"]), _ptr(a["ref_off"]), len(case["names"]),
                                None, None, None, None, None, None, _ptr(a["k1"]), None, 0, 0, out.ctypes.data, None)
    assert rc == -1
    with pytest.raises(ValueError, match="bases are not given"):
        samfile._sam_text(case["names"], case["ref_len"], case["hits"], case["offsets"], None, None, quals=case["quals"])


def _case_file(path, case, quals, oriented, bam, base):
    a = corpus.arrays(case)
    n = lambda x: 0 if x is None else len(x)
    k1, k2 = (a["k1"], a["k2"]) if quals else (None, None)
    head = np.array([len(a["offsets"]) - 1, len(case["hits"]), int(case["paired"]), len(case["names"]), a["q_off"] is not None,
                     a["s1_off"] is not None, a["s2_off"] is not None, base, n(a["ref"]), n(a["q"]), n(a["s1"]), n(a["s2"]),
                     k1 is not None, k2 is not None, int(oriented), int(bam)], np.uint64)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for x in [a[k] for k in ("hits", "offsets", "ref", "ref_off", "q", "q_off", "s1", "s1_off", "s2", "s2_off")] + [k1, k2]:
            if x is not None:
                f.write(x.tobytes())


def test_sanitized_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer and UBSan, over the same corpus (host code only)"""
    from sailfish_amd import samfile
    exe = str(tmp_path / "samqual_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSAMQ_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    good, bad = [], []
    for paired in (True, False):
        tag = "pe" if paired else "se"
        for bam, cases in ((False, text_cases(paired)), (True, bam_cases(paired))):
            for name, case, base in cases:
                for i, (quals, oriented) in enumerate(corpus.MODES):
                    p = tmp_path / f"{name}.{tag}.{int(bam)}.{i}"
                    _case_file(p, case, quals, oriented, bam, base)
                    text = corpus.expected(case, quals, oriented, base, header=bam)
                    want = samfile.sam_to_bam(text)[len(samfile.sam_to_bam(samfile.sam_header(case["names"], case["ref_len"]))):] if bam else text
                    good.append((str(p), want))
        for j, (case, read, record, kind) in enumerate(corpus.failing(paired)):
            for bam in (False, True):
                p = tmp_path / f"failing{j}.{tag}.{int(bam)}"
                _case_file(p, case, True, True, bam, 0)
                bad.append((str(p), read, record, kind))
    r = subprocess.run([exe] + [p for p, _ in good] + [b[0] for b in bad], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("\n") == len(good) + len(bad) and " mismatch=1" not in r.stdout
    for p, want in good:
        assert re.search(rf"^{re.escape(p)} kind=0 .* bytes={len(want)} ", r.stdout, re.M), p
        with open(p + ".out", "rb") as f:
            assert f.read() == want, p
    for p, read, record, kind in bad:
        assert re.search(rf"^{re.escape(p)} kind={kind} read={read} record={record} ", r.stdout, re.M), p
