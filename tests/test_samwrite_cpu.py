"""The SAM lines of the device writer as csrc/samwfmt.h states them (the functions samtext_write.hip runs inside its kernels),
compiled as plain C++ with g++ -Wall -Wextra -Werror (tests/samwrite_harness.cpp) and judged by the host statement:
samfile._sam_text minus its header.  Bytes, sizes, line counts, and the lowest (read, record) of every batch that cannot be
written.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import samwrite_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "samwrite_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p
_ARGS = [_P, _P, C.c_uint32, C.c_int, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, C.c_uint64, _P]


def _ptr(a):
    return None if a is None else a.ctypes.data


class Harness:
    def __init__(self, so):
        self.L = C.CDLL(so)
        self.L.samw_harness_size.argtypes = _ARGS
        self.L.samw_harness_format.argtypes = _ARGS

    def _call(self, fn, case, base, last):
        a = corpus.arrays(case)
        self._keep = a
        return fn(_ptr(a["hits"]), _ptr(a["offsets"]), len(a["offsets"]) - 1, int(case["paired"]), _ptr(a["ref"]), _ptr(a["ref_off"]),
                  len(case["names"]), _ptr(a["q"]), _ptr(a["q_off"]), _ptr(a["s1"]), _ptr(a["s1_off"]), _ptr(a["s2"]), _ptr(a["s2_off"]), base, last)

    def size(self, case, base=0):
        """-> dict(n_bytes, n_lines, n_units, max_unit_bytes, kind, read, record)"""
        out = np.zeros(8, np.uint64)
        self._call(self.L.samw_harness_size, case, base, out.ctypes.data)
        assert out[7] == 0, "samw_unit_len and samw_serial disagree"
        return dict(zip(("n_bytes", "n_lines", "n_units", "max_unit_bytes", "kind", "read", "record"), (int(x) for x in out[:7])))

    def text(self, case, base=0):
        res = self.size(case, base)
        assert res["kind"] == 0
        buf = np.full(res["n_bytes"] + 16, 0xAB, np.uint8)
        assert self._call(self.L.samw_harness_format, case, base, buf.ctypes.data) == 0
        assert (buf[res["n_bytes"]:] == 0xAB).all()
        return buf[:res["n_bytes"]].tobytes(), res


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("samw")), "libsamwrite_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    return Harness(so)


def same_as_host(harness, case, base=0):
    for v in corpus.variants(case):
        want = corpus.expected(v, base)
        got, res = harness.text(v, base)
        assert got == want
        assert res["n_lines"] == want.count(b"\n")
    return want


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_corner_batch(harness, paired):
    case = corpus.corner(paired)
    hits, off = case["hits"], case["offsets"]
    per_read = np.diff(off.astype(np.int64))
    assert {0, 1, 3} <= set(per_read.tolist())
    assert set(hits["mate_status"].tolist()) == ({1, 2, 3} if paired else {0}) and set(hits["fwd"].tolist()) == {0, 1}
    assert {0, -1}.issubset(hits["pos"].tolist()) and (hits["pos"] == -(hits["read_len"].astype(np.int64) - 1))[hits["read_len"] > 1].any()
    assert hits["pos"].max() == 2 ** 31 - 1 and (not paired or hits["frag_len"].max() == 2 ** 32 - 1)
    if paired:
        pairs = hits[hits["mate_status"] == 3]
        assert (pairs["pos"] == pairs["mate_pos"]).any() and (pairs["pos"] < pairs["mate_pos"]).any() and (pairs["pos"] > pairs["mate_pos"]).any()
    assert {0, 300} <= {len(q) for q in case["read_names"]}
    seq_lens = {len(s) for sq in case["seqs"] for s in (sq if paired else (sq,))}
    assert {0, 1, 100, 9000} <= seq_lens
    text = same_as_host(harness, case)                     # (the variant without names and without bases comes last)
    assert text.startswith((b"r0\t77\t*\t0\t255\t*\t*\t0\t0\t*\t*\nr0\t141\t" if paired else b"r0\t4\t*\t0\t255\t*\t*\t0\t0\t*\t*\n"))
    same_as_host(harness, case, base=999_999_999_990)      # default names across a digit edge, past 2^32


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
@pytest.mark.parametrize("seed", range(3))
def test_random_batches(harness, seed, paired):
    case = corpus.random_case(seed, paired)
    assert len(case["offsets"]) - 1 == 300 and len(case["hits"]) > 300
    same_as_host(harness, case, base=seed * 95)


@pytest.mark.parametrize("paired", [True, False], ids=["paired", "single"])
def test_batches_that_cannot_be_written(harness, paired):
    from sailfish_amd import samfile
    cases = corpus.failing(paired)
    assert {c[3] for c in cases} == {1, 2}
    for case, read, record, kind in cases:
        for v in corpus.variants(case):
            res = harness.size(v)
            assert (res["kind"], res["read"], res["record"]) == (kind, read, record)
            with pytest.raises(ValueError if kind == 1 else IndexError) as e:
                corpus.expected(v)
            assert kind != 1 or str(e.value).startswith(f"read {read}, record {record}: ")
    assert set(samfile.WRITE_KINDS) == {1, 2}


def test_empty_batches(harness):
    for paired in (True, False):
        none = dict(names=corpus.NAMES, ref_len=corpus.REF_LEN, hits=np.zeros(0, corpus.HIT_DTYPE), offsets=np.zeros(1, np.uint32), paired=paired,
                    read_names=[], seqs=[])
        assert harness.text(none)[0] == b""
        unmapped = dict(none, offsets=np.zeros(6, np.uint32), read_names=[b"a", b"", b"c c", b"d" * 70, b"e"],
                        seqs=[(b"AC", b"") if paired else b"AC"] * 5)
        same_as_host(harness, unmapped, base=7)


def test_header_is_sam_text_s():
    from sailfish_amd import samfile
    text = samfile._sam_text(corpus.NAMES, corpus.REF_LEN, np.zeros(0, corpus.HIT_DTYPE), np.zeros(1, np.uint32), None, None)
    assert text == samfile.sam_header(corpus.NAMES, corpus.REF_LEN) and text.count(b"\n") == 1 + len(corpus.NAMES)


def _case_file(path, case, base):
    a = corpus.arrays(case)
    n = lambda x: 0 if x is None else len(x)
    head = np.array([len(a["offsets"]) - 1, len(case["hits"]), int(case["paired"]), len(case["names"]), a["q_off"] is not None,
                     a["s1_off"] is not None, a["s2_off"] is not None, base, n(a["ref"]), n(a["q"]), n(a["s1"]), n(a["s2"])], np.uint64)
    with open(path, "wb") as f:
        f.write(head.tobytes())
        for k in ("hits", "offsets", "ref", "ref_off", "q", "q_off", "s1", "s1_off", "s2", "s2_off"):
            if a[k] is not None:
                f.write(a[k].tobytes())


def test_sanitized_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer and UBSan, over the same corpus (host code only)"""
    exe = str(tmp_path / "samwrite_harness_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSAMW_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    good, bad = [], []
    for paired in (True, False):
        tag = "pe" if paired else "se"
        for name, case, base in [("corner", corpus.corner(paired), 0), ("far", corpus.corner(paired), 2 ** 40)] + \
                [(f"random{s}", corpus.random_case(s, paired), s) for s in range(3)]:
            for i, v in enumerate(corpus.variants(case)):
                p = tmp_path / f"{name}.{tag}.{i}"
                _case_file(p, v, base)
                good.append((str(p), corpus.expected(v, base)))
        for j, (case, read, record, kind) in enumerate(corpus.failing(paired)):
            p = tmp_path / f"failing{j}.{tag}"
            _case_file(p, case, 0)
            bad.append((str(p), read, record, kind))
    r = subprocess.run([exe] + [p for p, _ in good] + [b[0] for b in bad], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("\n") == len(good) + len(bad) and " mismatch=1" not in r.stdout
    for p, want in good:
        assert re.search(rf"^{re.escape(p)} kind=0 .* bytes={len(want)} lines={want.count(10)} ", r.stdout, re.M), p
        with open(p + ".out", "rb") as f:
            assert f.read() == want, p
    for p, read, record, kind in bad:
        assert re.search(rf"^{re.escape(p)} kind={kind} read={read} record={record} ", r.stdout, re.M), p
