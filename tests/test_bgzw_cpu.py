"""The arithmetic of the device BGZF writer (sailfish_amd/csrc/bgzwfmt.h, used by bgzf_write.hip) compiled as plain C++ with g++
(tests/bgzw_harness.cpp; nothing but libstdc++ is linked) and judged by Python's zlib and gzip and by the project's own serial
inflater (bgzfmt.h through tests/bgzf_harness.cpp): every member the serial encoder writes is valid, stored where coding does not
pay, carries the matches the parse is stated to find, and alignment files come out below zlib's Z_RLE.  No GPU."""
import ctypes as C
import gzip
import json
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import bamwrite_corpus
import test_bgzf_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
STORED_OVERHEAD = 31          # 18 header bytes, 5 of the stored block, CRC-32 + ISIZE
STEP, SLICE = 256, 64         # kBgzwStep, kBgzwSlice


def build_harness(dirpath):
    so = os.path.join(str(dirpath), "libbgzw_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "sailfish_amd", "csrc"), os.path.join(ROOT, "tests", "bgzw_harness.cpp"), "-o", so])
    return so


class Harness:
    def __init__(self, so):
        self.so = so
        lib = C.CDLL(so)
        lib.bgzw_harness_payload.restype = C.c_uint32
        self.P = int(lib.bgzw_harness_payload())
        self._enc = lib.bgzw_harness_encode
        self._enc.restype = C.c_int64
        self._enc.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        self._tok = lib.bgzw_harness_tokens
        self._tok.restype = C.c_uint32
        self._tok.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32]
        self._dsym = lib.bgzw_harness_dist_symbol
        self._dsym.restype = C.c_int
        self._dsym.argtypes = [C.c_uint32, C.POINTER(C.c_int), C.POINTER(C.c_uint32)]

    def encode(self, data, writes=()):
        """the serial encoder's file for `data` written in pieces of `writes` bytes -> (file, dict(members, stored, matches, literals))"""
        data = bytes(data)
        cap = len(data) + STORED_OVERHEAD * (len(data) // self.P + len(writes) + 2) + 28
        out = np.zeros(cap, np.uint8)
        stats = (C.c_uint64 * 4)()
        n = self._enc(data, len(data), (C.c_uint64 * max(len(writes), 1))(*writes), len(writes), out.ctypes.data, cap, stats)
        assert n >= 0
        return out[:n].tobytes(), dict(zip(("members", "stored", "matches", "literals"), (int(x) for x in stats)))

    def tokens(self, data):
        """[(position, length, distance)] of one member's parse; length 1 = a literal"""
        data = bytes(data)
        assert 1 <= len(data) <= self.P
        out = np.zeros((len(data), 3), np.uint32)
        k = self._tok(data, len(data), out.ctypes.data, len(data))
        return [tuple(int(x) for x in t) for t in out[:k]]

    def dist_symbol(self, d):
        eb, ev = C.c_int(), C.c_uint32()
        return self._dsym(d, C.byref(eb), C.byref(ev)), eb.value, ev.value


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return Harness(build_harness(tmp_path_factory.mktemp("bgzwh")))


@pytest.fixture(scope="module")
def inflater(tmp_path_factory):
    return test_bgzf_cpu.Harness(test_bgzf_cpu.build_harness(tmp_path_factory.mktemp("bgzh")))


def members(file):
    """walks BSIZE: [(member bytes, payload per zlib)]; checks header, stream end, CRC-32, ISIZE and the EOF member"""
    out, p = [], 0
    while p < len(file):
        assert file[p:p + 16] == b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0", p
        total = struct.unpack_from("<H", file, p + 16)[0] + 1
        m = file[p:p + total]
        assert len(m) == total
        d = zlib.decompressobj(-15)
        payload = d.decompress(m[18:-8]) + d.flush()
        assert d.eof and d.unused_data == b"", p                    # one final block, nothing behind it
        crc, isize = struct.unpack("<II", m[-8:])
        assert crc == zlib.crc32(payload) and isize == len(payload), p
        out.append((m, payload))
        p += total
    assert p == len(file) and file[-28:] == EOF and out[-1][1] == b""
    return out


def check_file(file, data, P, writes=(), inflater=None):
    """the file is valid BGZF for `data` cut at multiples of P within every write; returns the members"""
    data = bytes(data)
    ms = members(file)
    assert b"".join(p for _, p in ms) == data and gzip.decompress(file) == data
    pieces, used = [], 0
    for w in writes:
        w = min(w, len(data) - used); pieces.append(w); used += w
    if used < len(data):
        pieces.append(len(data) - used)
    want = [min(P, w - b) for w in pieces for b in range(0, w, P)] + [0]
    assert [len(p) for _, p in ms] == want
    for m, p in ms:
        assert len(m) <= len(p) + STORED_OVERHEAD
        if inflater is not None:
            kind, got, _ = inflater.member(m)
            assert kind == 0 and got == p
    return ms


def inputs(P):
    """name -> bytes: the smallest inputs that can break the encoder"""
    rng = np.random.default_rng(31)
    text = (b"SRR1.7\t99\tENST0001\t1234\t255\t100M\t=\t1400\t266\tACGTTGCAAGGCTTAACG\t*\n" * 2000)
    cases = {}
    for n in (1, 2, 3, 4, 257, 258, 259, 260, P - 1, P, P + 1, 2 * P + 3):
        cases[f"text{n}"] = text[:n]
        cases[f"zeros{n}"] = bytes(n)
    for period in (2, 3, 7):
        cases[f"period{period}"] = (bytes(range(65, 65 + period)) * (P // period + 300))[:P + 600]
    cases["random"] = rng.integers(0, 256, 2 * P + 77, dtype=np.uint8).tobytes()
    cases["no_match"] = bytes(range(256))
    one = bytearray(range(256)) * 2
    one[256:] = bytes(reversed(range(256)))               # descending: no 3-gram of the ascending half comes back
    one[STEP:STEP + 8] = bytes(range(10, 18))             # but this one does, once, at the start of a step
    cases["one_match"] = bytes(one[:STEP + 8]) + bytes([200, 100, 201, 101])
    tail = rng.integers(0, 256, 3 * STEP, dtype=np.uint8).tobytes()
    cases["match_ends_member"] = tail + tail[5:5 + 40]                           # the repeat is the member's last 40 bytes
    long_rep = rng.integers(0, 256, 400, dtype=np.uint8).tobytes()
    cases["across_slice_step_member"] = (rng.integers(0, 256, P - 200, dtype=np.uint8).tobytes() + long_rep + long_rep + long_rep)
    return cases


def test_harness_links_nothing_but_libstdcxx(harness):
    needed = re.findall(r"NEEDED.*\[(.*?)\]", subprocess.check_output(["readelf", "-d", harness.so], text=True))
    assert needed and all(n.startswith(("libstdc++", "libm.", "libgcc_s", "libc.")) for n in needed), needed
    assert harness.P <= 65280 and harness.P % STEP == 0 and STEP % SLICE == 0


def test_distance_symbols(harness):
    """RFC 1951 3.2.5: every distance 1 .. 32 768 against the table"""
    base, d = [], 1
    for sym in range(30):
        eb = max(0, sym // 2 - 1)
        base.append((d, eb)); d += 1 << eb
    assert d == 32769
    for sym, (lo, eb) in enumerate(base):
        for dist in {lo, lo + (1 << eb) - 1, lo + (1 << eb) // 2}:
            assert harness.dist_symbol(dist) == (sym, eb, dist - lo), dist
    rng = np.random.default_rng(32)
    for dist in rng.integers(1, 32769, 500):
        sym, eb, ev = harness.dist_symbol(int(dist))
        assert base[sym] == (int(dist) - ev, eb) and ev < 1 << eb


def test_every_member_is_valid(harness, inflater):
    P = harness.P
    for name, data in inputs(P).items():
        file, st = harness.encode(data)
        ms = check_file(file, data, P, inflater=inflater)
        assert st["members"] == len(ms) - 1, name
        if name == "random":
            assert st["stored"] == st["members"] == 3 and st["matches"] == st["literals"] == 0
            assert all(len(m) == len(p) + STORED_OVERHEAD for m, p in ms[:-1])
        if name.startswith(("zeros", "period")) and len(data) >= 257:
            assert st["stored"] == (1 if 0 < len(data) % P < 32 else 0) and len(file) < len(data) // 8 + 200, name      # a tiny last member


def several_writes_case(P):
    return bamwrite_corpus.stream(True, "sam", 300)[:3 * P + 1000], (1, P - 1, 0, P + 1, 7)


def test_empty_file_and_several_writes(harness, inflater):
    P = harness.P
    file, st = harness.encode(b"")
    assert file == EOF and st["members"] == 0
    data, writes = several_writes_case(P)
    file, st = harness.encode(data, writes)
    check_file(file, data, P, writes, inflater)
    assert st["members"] == 1 + 1 + 0 + 2 + 1 + 2 and file != harness.encode(data)[0]


def test_no_match_and_one_match(harness):
    c = inputs(harness.P)
    assert all(l == 1 for _, l, _ in harness.tokens(c["no_match"]))
    toks = harness.tokens(c["one_match"])
    assert [(p, l, d) for p, l, d in toks if l > 1] == [(STEP, 8, STEP - 10)]
    file, st = harness.encode(c["one_match"])
    check_file(file, c["one_match"], harness.P)
    assert (st["matches"], st["literals"]) == (1, len(c["one_match"]) - 8) or st["stored"] == 1


def test_matches_end_at_slice_and_member_ends(harness):
    c = inputs(harness.P)
    data = c["match_ends_member"]
    toks = harness.tokens(data)
    assert toks[-1][0] + toks[-1][1] == len(data) and toks[-1][1] >= 3          # the last token is a match onto the last byte
    covered = sum(l for p, l, d in toks if l > 1 and p >= 3 * STEP)
    assert covered >= 36                                                         # the 40 repeated bytes, but for a slice restart
    data = c["across_slice_step_member"][:harness.P]
    for p, l, d in harness.tokens(data):
        assert p // SLICE == (p + l - 1) // SLICE and p + l <= len(data)         # no token leaves its slice
        assert l == 1 or (3 <= l <= 258 and 1 <= d <= p and data[p:p + l] == bytes(data[p - d + k % d] for k in range(l)))


def _planted(rng, n, at, dist, length):
    """n random bytes with bytes [at - dist, at - dist + length) repeated at `at`"""
    b = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    for k in range(length):
        b[at + k] = b[at - dist + k]
    return bytes(b)


def _repeat_at(P, dist):
    """(data, at): zeros with a 12-byte pattern that comes back `dist` bytes later at `at`, its source in an earlier step"""
    m = -(-8 // dist)                                     # periods in front of `at`, so that a whole 4-gram lies there
    at = -(-dist * m // STEP) * STEP
    if at > P - 4:
        at = dist
    n = min(at + 40, P)
    period = (b"ABCDEFGHIJKL" + bytes(max(dist - 12, 0)))[:dist]
    buf = bytearray(n)
    for k in range(at - dist * m, min(at + 12, n)):
        buf[k] = period[(k - at) % dist]
    return bytes(buf), at


def symbol_distances(P):
    """the lowest and highest distance of every distance symbol that fits a member"""
    dists, d = [], 1
    for sym in range(30):
        eb = max(0, sym // 2 - 1)
        dists += [d, d + (1 << eb) - 1]; d += 1 << eb
    # the greatest distance is P - 4, not P - 3: the parse finds a repeat through its 4-byte hash, so the last position that can
    # start one is P - 4, and its farthest source is position 0
    return sorted({min(x, P - 4) for x in dists})


def member_cut_case(P):
    block = np.random.default_rng(33).integers(0, 256, P, dtype=np.uint8).tobytes()
    return block, block + block[-50:]


def test_every_distance_symbol(harness):
    """the lowest and highest distance of every distance symbol that fits a member: the token at the repeat is a match at exactly
    that distance.  A repeat across the member cut is not a match: the next member starts afresh."""
    P = harness.P
    dists = symbol_distances(P)
    assert dists[:12] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16] and dists[-2:] == [24577, P - 4]
    seen = set()
    for dist in dists:
        data, at = _repeat_at(P, dist)
        toks = harness.tokens(data)
        want = min(12, len(data) - at)
        assert any(p == at and d == dist and l >= want for p, l, d in toks), (dist, at, [t for t in toks if t[0] >= at - 2][:4])
        seen.add(harness.dist_symbol(dist)[0])
        file, st = harness.encode(data)
        check_file(file, data, P)
        assert st["stored"] == 0 and st["matches"] >= 1
    assert seen == set(range(30))
    block, twice = member_cut_case(P)
    file, st = harness.encode(twice)
    check_file(file, twice, P)
    assert st["stored"] == 2 and all(l == 1 for _, l, _ in harness.tokens(block[-50:]))


def planted_cases():
    """a repeat of every length 3 .. 258 at a slice start and across a slice end"""
    rng = np.random.default_rng(34)
    return {f"len{length}@{at}": _planted(rng, at + length + 9, at, STEP + 11, length)
            for length in range(3, 259) for at in (2 * STEP, 2 * STEP + SLICE - 3)}


def test_every_match_length(harness):
    """a repeat of every length 3 .. 258 planted at a slice start and across a slice end: the file inflates, no token leaves its
    slice, and every length a slice can hold is emitted.  Lengths 65 .. 258 (length symbols up to 285) are never emitted by this
    parse: a match ends at the end of its 64-byte slice, so that one lane owns one slice; the planted repeats of those
    lengths are coded as several matches, and gz_len_symbol's upper half is exercised by gzfmt.h's own tests only."""
    P = harness.P
    lengths = set()
    for data in planted_cases().values():
        toks = harness.tokens(data)
        assert all(p // SLICE == (p + l - 1) // SLICE for p, l, _ in toks)
        lengths |= {l for _, l, _ in toks if l > 1}
        file, _ = harness.encode(data)
        check_file(file, data, P)
    assert lengths == set(range(3, SLICE + 1))         # nothing above SLICE: see the docstring


def _zlib_file(data, P, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    """bytes of the BGZF file zlib writes at the same member cut"""
    n = 28
    for a in range(0, len(data), P):
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        n += 18 + len(z.compress(data[a:a + P]) + z.flush()) + 8
    return n


@pytest.mark.parametrize("paired,kind", [(True, "sam"), (True, "bam"), (False, "sam"), (False, "bam")])
def test_size_against_zlib(harness, inflater, paired, kind):
    """the point of the change: alignment files strictly below zlib's Z_RLE (the token class of gzfmt.h) at the same member cut.
    The ratios to level 1 and level 6 are printed, not gated; DESIGN 4.22 records them."""
    P = harness.P
    data = bamwrite_corpus.stream(paired, kind)
    file, st = harness.encode(data)
    check_file(file, data, P, inflater=inflater if (paired, kind) == (True, "sam") else None)
    rle, l1, l6 = (_zlib_file(data, P, 6, zlib.Z_RLE), _zlib_file(data, P, 1), _zlib_file(data, P, 6))
    print(f"{'paired' if paired else 'single-end'} {kind}: {len(data)} B -> {len(file)} B in {st['members']} members ({st['stored']} stored), "
          f"{st['matches']} matches, {st['literals']} literals; zlib Z_RLE {rle}, level 1 {l1}, level 6 {l6}; "
          f"ratio to level 1 {len(file) / l1:.3f}, to level 6 {len(file) / l6:.3f}, to Z_RLE {len(file) / rle:.3f}")
    assert len(file) < rle


def digest_sets(P):
    """name -> (payload, write cuts), or a list of them digested as one: every input the tests above hand to the serial encoder"""
    sets = {f"inputs/{k}": (v, ()) for k, v in inputs(P).items()}
    sets["empty"] = (b"", ())
    data, writes = several_writes_case(P)
    sets["several_writes"] = (data, writes)
    sets["several_writes/one_write"] = (data, ())
    sets["every_distance_symbol"] = [(_repeat_at(P, d)[0], ()) for d in symbol_distances(P)]
    sets["member_cut"] = (member_cut_case(P)[1], ())
    sets["every_match_length"] = [(v, ()) for v in planted_cases().values()]
    for paired, kind in ((True, "sam"), (True, "bam"), (False, "sam"), (False, "bam")):
        sets[f"corpus/{'paired' if paired else 'single'}.{kind}"] = (bamwrite_corpus.stream(paired, kind), ())
    return sets


def test_serial_file_digests(harness):
    """the serial encoder still writes the files it wrote when tests/golden/deflate_writer_digests.json was recorded: zlib accepts
    any valid file, this pins the bytes that tests/test_gpu_bgzw.py compares the device with"""
    from test_gzwrite_cpu import DIGESTS, stream_digests
    with open(DIGESTS) as f:
        want = json.load(f)["bgzf"]
    got = stream_digests(lambda data, writes: harness.encode(data, writes)[0], digest_sets(harness.P))
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
