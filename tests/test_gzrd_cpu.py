"""The rules of the chunked inflater of ordinary gzip (sailfish_amd/csrc/gzrdfmt.h, used by gz_read.hip) compiled as plain C++ with
g++ (tests/gzrd_harness.cpp: finder, pass A, chain, window propagation, pass B and trailer run serially behind the ABI's four
calls) and judged by zlib: round trips of what zlib writes at chunk_bytes = 512, streaming over cut points and capacities, a
false start on purpose, one file per error kind, agreement with zlib on 1200 single-bit flips, and the finder's yield at the
default chunk_bytes on a realistic stream.  Block counts and true block starts come from a plain serial walk that is the same
decoder with a stop rule that never stops: independent of the chunking, not of the decoder (zlib judges the payload, and the block
mixes are asserted per shape).  The file sets and the call loop are shared with tests/test_gpu_gzrd.py.  No GPU."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_bgzf_cpu import (BAD_BLOCK_TYPE, BAD_CODE_LENGTHS, BAD_HEADER, BAD_SYMBOL, CRC_MISMATCH, DISTANCE_TOO_FAR, SIZE_MISMATCH,
                           STORED_LEN, TRUNCATED, Bits, dynamic_header, fixed_block)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_FORMAT = 0, 8
NONE = 2 ** 64 - 1
CHUNK = 512
PLAIN_HEADER = b"\x1f\x8b\x08\0\0\0\0\0\0\xff"


# ---- the harness -----------------------------------------------------------------------------------------------------------

def build_harness(dirpath):
    so = os.path.join(str(dirpath), "libgzrd_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "sailfish_amd", "csrc"), os.path.join(ROOT, "tests", "gzrd_harness.cpp"), "-o", so])
    return so


class Result(C.Structure):             # sfgpu_gzrd_result
    _fields_ = [("consumed", C.c_uint64), ("n_bytes_out", C.c_uint64), ("n_chunks", C.c_uint64), ("n_candidates", C.c_uint64),
                ("n_false_starts", C.c_uint64), ("n_stored_blocks", C.c_uint64), ("n_fixed_blocks", C.c_uint64),
                ("n_dynamic_blocks", C.c_uint64), ("need_cap", C.c_uint64), ("error_offset", C.c_uint64), ("member_end", C.c_int32),
                ("error_kind", C.c_int32), ("ms_copy", C.c_double), ("ms_find", C.c_double), ("ms_decode", C.c_double),
                ("ms_propagate", C.c_double), ("ms_emit", C.c_double)]


class Harness:
    def __init__(self, so):
        self.so = so
        L = self.L = C.CDLL(so)
        L.gzrd_harness_open.argtypes = [C.POINTER(C.c_void_p), C.c_uint32]
        L.gzrd_harness_close.argtypes = [C.c_void_p]
        L.gzrd_harness_plan.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(Result)]
        L.gzrd_harness_emit.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Result)]
        for name in ("gzrd_harness_chain", "gzrd_harness_candidates"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
            getattr(L, name).restype = C.c_uint64
        L.gzrd_harness_walk.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_int32)]
        L.gzrd_harness_walk.restype = C.c_uint64

    def open(self, chunk_bytes=CHUNK):
        return HarnessHandle(self.L, chunk_bytes)

    def walk(self, data, start_bit):
        """a plain serial walk of the DEFLATE stream at start_bit -> (bit positions of its block starts, (stored, fixed, dynamic))"""
        starts = np.zeros(1 << 16, np.uint64)
        blocks, status = (C.c_uint32 * 3)(), C.c_int32()
        k = self.L.gzrd_harness_walk(bytes(data), len(data), start_bit, starts.ctypes.data, starts.size, blocks, C.byref(status))
        assert k <= starts.size and status.value == 1
        return starts[:k].tolist(), tuple(blocks)


class HarnessHandle:
    """one stream: call(bytes, final, cap) -> (rc of the last call made, Result, payload) = plan, then emit when there is something to emit"""

    def __init__(self, L, chunk_bytes):
        self.L, self.h = L, C.c_void_p()
        assert L.gzrd_harness_open(C.byref(self.h), chunk_bytes) == OK

    def call(self, buf, final, cap):
        res = Result()
        rc = self.L.gzrd_harness_plan(self.h, buf, len(buf), int(final), cap, C.byref(res))
        if rc not in (OK, ERR_FORMAT):
            raise RuntimeError(f"plan: {rc}")
        if rc == ERR_FORMAT and res.n_chunks == 0:
            return rc, res, b""
        out = np.full(int(res.n_bytes_out) + 1, 0xA5, np.uint8)
        rc = self.L.gzrd_harness_emit(self.h, out.ctypes.data, C.byref(res))
        assert out[-1] == 0xA5
        return rc, res, out[:-1].tobytes()

    def chain(self):
        starts = np.zeros(1 << 16, np.uint64)
        k = self.L.gzrd_harness_chain(self.h, starts.ctypes.data, starts.size)
        return starts[:k].tolist()

    def candidates(self):
        cand = np.zeros(1 << 16, np.uint64)
        k = self.L.gzrd_harness_candidates(self.h, cand.ctypes.data, cand.size)
        return cand[:k].tolist()

    def close(self):
        if self.h:
            self.L.gzrd_harness_close(self.h); self.h = None


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return Harness(build_harness(tmp_path_factory.mktemp("gzrdh")))


def run(handle, data, cuts=(), cap=None):
    """The file in pieces: the bytes up to each cut point (final only at the last), call after call until nothing moves; a caller
    with a capacity grows it to need_cap when not even one chunk fits.  -> everything the ABI reports, summed over the calls."""
    data = bytes(data)
    cuts = sorted({c for c in cuts if c < len(data)} | {len(data)})
    tot = dict(rc=OK, out=[], consumed=0, n_bytes_out=0, n_chunks=0, n_candidates=0, n_false_starts=0, blocks=[0, 0, 0], member_end=0,
               error=(0, NONE), calls=0, grown=0, most_chunks=0)
    cap_now = NONE if cap is None else cap
    pos = 0
    for c in cuts:
        while True:
            rc, r, payload = handle.call(data[pos:c], c == len(data), cap_now)
            tot["calls"] += 1
            for k in ("n_bytes_out", "n_chunks", "n_candidates", "n_false_starts", "member_end"):
                tot[k] += int(getattr(r, k))
            for t, k in enumerate(("n_stored_blocks", "n_fixed_blocks", "n_dynamic_blocks")):
                tot["blocks"][t] += int(getattr(r, k))
            tot["most_chunks"] = max(tot["most_chunks"], int(r.n_chunks))
            tot["out"].append(payload)
            assert len(payload) == r.n_bytes_out
            if rc != OK:
                tot["rc"], tot["error"] = rc, (r.error_kind, pos + int(r.error_offset))
                break
            assert r.error_kind == 0 and r.error_offset == NONE
            pos += int(r.consumed)
            if r.need_cap:
                assert r.n_chunks == 0 and r.need_cap > cap_now
                cap_now = int(r.need_cap); tot["grown"] += 1
                continue
            if r.consumed == 0 and r.n_chunks == 0:
                break
        if tot["rc"] != OK:
            break
    tot["consumed"] = pos
    tot["out"] = b"".join(tot["out"]) if tot["rc"] == OK else b""
    tot["blocks"] = tuple(tot["blocks"])
    return tot


def run_fresh(harness, data, cuts=(), cap=None, chunk_bytes=CHUNK):
    h = harness.open(chunk_bytes)
    try:
        return run(h, data, cuts, cap)
    finally:
        h.close()


# ---- files -----------------------------------------------------------------------------------------------------------------

def fastq_like(seed, n, length=100):
    """n FASTQ records of `length` bases whose qualities are skewed towards the high values, as a sequencer's are (fastq_text draws
    them uniformly from all printable bytes, and zlib answers that with fixed blocks)"""
    rng = np.random.default_rng(seed)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, length))
    w = np.exp(np.arange(39) / 6.0)
    qual = rng.choice(np.arange(35, 74, dtype=np.uint8), (n, length), p=w / w.sum())
    return b"".join(b"@SRR0.%d %d/1\n%s\n+\n%s\n" % (r, r, seq[r].tobytes(), qual[r].tobytes()) for r in range(n))


def text_630():
    return fastq_like(51, 630)


def deflated(data, level=6, wbits=31, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    z = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    return z.compress(data) + z.flush()


def member(body, payload, name=None, extra=None, comment=None, hcrc=False, crc=None, isize=None, flg_or=0, cm=8):
    flg = (8 if name is not None else 0) | (4 if extra is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0) | flg_or
    head = bytes([0x1f, 0x8b, cm, flg, 0, 0, 0, 0, 0, 0xff])
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if name is not None:
        head += name + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xffff)
    return head + body + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, (len(payload) if isize is None else isize) & 0xffffffff)


ROUND_TRIP_NAMES = ([f"level{lv}_mem{m}" for lv in (1, 6, 9) for m in (1, 2, 8)]
                    + ["fixed", "level0", "huffman_only", "rle", "random", "empty", "flushes", "far_matches_32700", "far_matches_32500",
                       "three_members"])
STREAM_NAMES = ["level6_mem1", "flushes", "three_members"]


def round_trip_files():
    """name -> (file bytes, payload)"""
    text = text_630()
    assert 130_000 < len(text) < 140_000
    files = {}
    for lv in (1, 6, 9):
        for m in (1, 2, 8):
            files[f"level{lv}_mem{m}"] = (deflated(text, lv, mem=m), text)
    files["fixed"] = (deflated(text, strategy=zlib.Z_FIXED), text)
    files["level0"] = (deflated(text, 0), text)
    files["huffman_only"] = (deflated(text, mem=2, strategy=zlib.Z_HUFFMAN_ONLY), text)
    files["rle"] = (deflated(text, mem=2, strategy=zlib.Z_RLE), text)
    noise = np.random.default_rng(52).integers(0, 256, 40000, dtype=np.uint8).tobytes()
    files["random"] = (deflated(noise), noise)
    files["empty"] = (deflated(b""), b"")
    z = zlib.compressobj(6, zlib.DEFLATED, 31)
    parts = []
    for i, at in enumerate(range(0, len(text), 3000)):
        parts += [z.compress(text[at:at + 3000]), z.flush(zlib.Z_SYNC_FLUSH if i % 2 == 0 else zlib.Z_FULL_FLUSH)]
    files["flushes"] = (b"".join(parts) + z.flush(), text)
    # 32700 random bytes four times over.  zlib's deflate looks back 32768 - 262 bytes at the most, so it finds no match here and
    # stores the lot; the second file is what reaches far: a period of 32500, with every 16th byte of the repeats redrawn so that
    # the matches stay short and the blocks (256 symbols each at memLevel 2) many
    rng = np.random.default_rng(53)
    far = rng.integers(0, 256, 32700, dtype=np.uint8).tobytes() * 4
    files["far_matches_32700"] = (deflated(far, 6, mem=2), far)
    rep = np.tile(rng.integers(0, 256, 32500, dtype=np.uint8), 4)
    rep[32500 + 7::16] = rng.integers(0, 256, rep[32500 + 7::16].size, dtype=np.uint8)
    files["far_matches_32500"] = (deflated(rep.tobytes(), 6, mem=2), rep.tobytes())
    a, b, c = text[:50000], text[50000:50010], text[50010:]
    files["three_members"] = (member(deflated(a, 6, -15, 1), a, name=b"reads_1.fastq", extra=b"XY\x03\0abc")
                              + member(deflated(b, 6, -15), b, comment=b"ten bytes", hcrc=True)
                              + member(deflated(c, 9, -15, 2), c, name=b"n", comment=b"c", extra=b"", hcrc=True) + bytes(37), text)
    assert sorted(files) == sorted(ROUND_TRIP_NAMES)
    return files


def header_len(data):
    """of the first member (what zlib leaves in front of the DEFLATE stream)"""
    flg, p = data[3], 10
    if flg & 4:
        p += 2 + (data[p] | data[p + 1] << 8)
    for bit in (8, 16):
        if flg & bit:
            p = data.index(b"\0", p) + 1
    return p + (2 if flg & 2 else 0)


def bit_at(data, b):
    return data[b >> 3] >> (b & 7) & 1


def serial_blocks(harness, data):
    """(stored, fixed, dynamic) of every member of the file, by a plain serial walk"""
    tot, pos = [0, 0, 0], 0
    while pos < len(data) and data[pos] != 0:
        d = zlib.decompressobj(31)
        d.decompress(data[pos:])
        assert d.eof
        used = len(data) - pos - len(d.unused_data)
        _, blocks = harness.walk(data[pos:pos + used], header_len(data[pos:]) * 8)
        tot = [x + y for x, y in zip(tot, blocks)]
        pos += used
    return tuple(tot)


# what the shapes must hold, by name: (stored, fixed, dynamic) -> bool, and whether more than one chunk is expected
MIXES = {"fixed": lambda s, f, d: s == 0 and f >= 1 and d == 0,
         "level0": lambda s, f, d: s >= 3 and f == 0 and d == 0,
         "random": lambda s, f, d: s >= 1 and d == 0,
         "empty": lambda s, f, d: s + f + d == 1,
         "flushes": lambda s, f, d: s >= 40 and d >= 40,
         "huffman_only": lambda s, f, d: d >= 20 and s == 0,
         "rle": lambda s, f, d: d >= 20 and s == 0,
         "far_matches_32700": lambda s, f, d: s >= 100 and d == 0,
         "far_matches_32500": lambda s, f, d: d >= 20,
         "three_members": lambda s, f, d: d >= 100}
for _lv in (1, 6, 9):
    MIXES[f"level{_lv}_mem1"] = lambda s, f, d: d >= 200 and s == 0
    MIXES[f"level{_lv}_mem2"] = lambda s, f, d: d >= 100 and s == 0
    MIXES[f"level{_lv}_mem8"] = lambda s, f, d: d >= 2 and s == 0
ONE_CHUNK = {"fixed", "level0", "random", "empty", "far_matches_32700"}          # no dynamic block: no candidate


@pytest.fixture(scope="module")
def files():
    return round_trip_files()


def test_harness_links_nothing_but_libstdcxx(harness):
    out = subprocess.check_output(["readelf", "-d", harness.so], text=True)
    assert "amdhip" not in out and "libz" not in out


@pytest.mark.parametrize("name", ROUND_TRIP_NAMES)
def test_round_trips(harness, files, name):
    data, payload = files[name]
    assert gzip.decompress(data) == payload
    r = run_fresh(harness, data)
    blocks = serial_blocks(harness, data)
    print(name, len(data), "bytes:", {k: r[k] for k in ("n_chunks", "n_candidates", "n_false_starts", "blocks", "calls", "member_end")})
    assert r["rc"] == OK and r["out"] == payload
    assert r["consumed"] == len(data) and r["n_bytes_out"] == len(payload)
    assert r["blocks"] == blocks and MIXES[name](*blocks), blocks
    assert r["member_end"] == (3 if name == "three_members" else 1)
    if name in ONE_CHUNK:
        assert r["n_candidates"] == 0 and r["n_chunks"] == 1
    else:
        assert r["most_chunks"] > 1 and r["n_candidates"] >= r["most_chunks"] - 1
    if blocks[2] >= 100:                         # many dynamic blocks in a few hundred spans: the chunks follow the spans
        assert r["n_chunks"] >= min(blocks[2], len(data) // CHUNK) // 2


# ---- streaming -------------------------------------------------------------------------------------------------------------

def stream_cuts(data):
    return list(range(997, len(data), 997)) + list(range(1, 41)) + list(range(len(data) - 8, len(data)))


@pytest.mark.parametrize("name", STREAM_NAMES)
def test_streaming_over_cut_points(harness, files, name):
    data, payload = files[name]
    one = run_fresh(harness, data)
    cut = run_fresh(harness, data, stream_cuts(data))
    assert cut["rc"] == OK and cut["out"] == one["out"] == payload
    assert cut["consumed"] == len(data) and cut["blocks"] == one["blocks"] and cut["member_end"] == one["member_end"]
    assert cut["calls"] > len(data) // 997


@pytest.mark.parametrize("cap", [1, 5000])
def test_capacities(harness, files, cap):
    data, payload = files["level6_mem1"]
    one = run_fresh(harness, data)
    r = run_fresh(harness, data, cap=cap)
    assert r["rc"] == OK and r["out"] == payload and r["blocks"] == one["blocks"]
    assert r["calls"] > 10
    if cap == 1:
        assert r["grown"] >= 1                   # need_cap: not even the first chunk fits
    else:
        assert r["grown"] == 0 and 1 < r["most_chunks"] < one["most_chunks"]      # a prefix of the chain


# ---- a false start on purpose ----------------------------------------------------------------------------------------------

def false_start_file():
    """A member whose first block is a STORED block that holds a raw DEFLATE stream, placed so that its dynamic block header is
    the first bit of span 1; dynamic blocks of text follow.  -> (file, payload, the bit position of the embedded header)"""
    text = text_630()
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    inner = z.compress(text[:400]) + z.flush(zlib.Z_SYNC_FLUSH)
    assert inner[0] & 7 == 4                     # BFINAL 0, BTYPE 2
    at = len(PLAIN_HEADER) + CHUNK               # span 1 begins here (spans count from the byte in which the stream begins)
    filler = bytes([0xff]) * (at - len(PLAIN_HEADER) - 5)
    held = filler + inner + bytes([0xff]) * 30
    stored = b"\0" + struct.pack("<HH", len(held), len(held) ^ 0xffff) + held
    payload = held + text
    return member(stored + deflated(text, 6, -15, 1), payload), payload, at * 8


def test_false_start(harness):
    data, payload, at = false_start_file()
    assert gzip.decompress(data) == payload
    h = harness.open()
    try:
        r = run(h, data)
    finally:
        h.close()
    h = harness.open()
    try:
        h.call(data, True, NONE)
        cand, chain = h.candidates(), h.chain()
    finally:
        h.close()
    assert cand[1] == at and at not in chain
    assert r["rc"] == OK and r["out"] == payload
    assert r["n_false_starts"] >= 1 and r["n_chunks"] > 10


# ---- errors ----------------------------------------------------------------------------------------------------------------

def error_files():
    """name -> (file, kind)"""
    good_body, good = fixed_block(list(b"a good member, ") + [(40, 15)])
    ok = member(good_body, good)
    out = {"reserved_flag": (member(good_body, good, flg_or=0x20), BAD_HEADER),
           "cm_7": (member(good_body, good, cm=7), BAD_HEADER),
           "garbage_behind": (ok + b"garbage behind a member", BAD_HEADER),
           "garbage_behind_padding": (ok + bytes(5) + b"\x1f\x8c", BAD_HEADER),
           "not_gzip": (b"@r0\nACGT\n+\nIIII\n", BAD_HEADER),
           "block_type_3": (member(b"\x07\0\0", b""), BAD_BLOCK_TYPE),
           "stored_len": (member(b"\x01\x03\0\xfc\xfeabc", b"abc"), STORED_LEN)}
    pad = bytes(40)
    out["hlit_287"] = (member(dynamic_header(287, 1, {0: 1, 8: 1}, []).bytes() + pad, b""), BAD_CODE_LENGTHS)
    out["repeat_without_previous"] = (member(dynamic_header(257, 1, {16: 1, 8: 1}, [(16, 0)]).bytes() + pad, b""), BAD_CODE_LENGTHS)
    out["code_length_code_incomplete"] = (member(dynamic_header(257, 1, {0: 2, 8: 2, 18: 2}, []).bytes() + pad, b""), BAD_CODE_LENGTHS)
    b = Bits(); b.put(1, 1); b.put(1, 2); b.fixed_sym(65); b.fixed_sym(286)
    out["length_symbol_286"] = (member(b.bytes() + pad, b"A"), BAD_SYMBOL)
    b = Bits(); b.put(1, 1); b.put(1, 2); b.fixed_sym(65); b.fixed_match(3, 2); b.fixed_sym(256)
    out["distance_too_far_at_start"] = (member(b.bytes(), b"A"), DISTANCE_TOO_FAR)
    b = Bits(); b.put(1, 1); b.put(1, 2)
    for ch in range(100):
        b.fixed_sym(ch)
    b.fixed_match(5, 101); b.fixed_sym(256)
    out["distance_too_far_100_in"] = (member(b.bytes(), bytes(range(100))), DISTANCE_TOO_FAR)
    out["crc"] = (member(good_body, good, crc=zlib.crc32(good) ^ 0x100), CRC_MISMATCH)
    out["isize_one_less"] = (member(good_body, good, isize=len(good) - 1), SIZE_MISMATCH)
    return out


def rejected(data):
    """by Python's gzip, or by zlib (gzip does not look at the reserved flags)"""
    try:
        gzip.decompress(data)
    except Exception:
        return True
    return zlib_says(data) is None


def test_error_kinds(harness):
    for name, (data, kind) in error_files().items():
        assert rejected(data), name
        r = run_fresh(harness, data)
        assert r["rc"] == ERR_FORMAT and r["error"][0] == kind, (name, r["error"])
        at = {"garbage_behind": len(data) - 23, "garbage_behind_padding": len(data) - 2, "not_gzip": 0, "reserved_flag": 0, "cm_7": 0}
        assert r["error"][1] == at.get(name, 10), (name, r["error"])


def test_an_error_deep_in_a_file_names_its_chunk(harness, files):
    data, _ = files["level6_mem1"]
    starts, _ = harness.walk(data, 80)
    k = len(starts) // 2
    bad = bytearray(data)
    for b in (starts[k] + 1, starts[k] + 2):     # BTYPE 2 -> 3
        bad[b >> 3] |= 1 << (b & 7)
    r = run_fresh(harness, bytes(bad))
    assert r["rc"] == ERR_FORMAT and r["error"][0] == BAD_BLOCK_TYPE
    assert 0 <= starts[k] // 8 - r["error"][1] < 4 * CHUNK        # the chunk that runs into the block starts a few spans before it


def test_truncated_at_every_cut(harness):
    text = text_630()[:3000]
    data = member(deflated(text, 6, -15, 1), text, name=b"x")
    assert run_fresh(harness, data, chunk_bytes=64)["out"] == text
    for cut in range(1, len(data)):
        r = run_fresh(harness, data[:cut], chunk_bytes=64)
        assert r["rc"] == ERR_FORMAT and r["error"][0] == TRUNCATED, cut
    assert run_fresh(harness, b"")["rc"] == OK


def flip_file():
    text = text_630()[:6000]
    return deflated(text, 6, 31, 1), text


def flip_positions(n_bits, n=1200):
    """the eight bits of an MTIME byte (which nobody checks), then random ones"""
    return list(range(32, 40)) + (40 + np.random.default_rng(54).choice(n_bits - 40, n - 8, replace=False)).tolist()


def zlib_says(data):
    """-> the payload, or None where zlib raises or does not reach the end of the member"""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(data)
    except zlib.error:
        return None
    return out if d.eof else None


def test_single_bit_flips_agree_with_zlib(harness):
    data, text = flip_file()
    assert zlib_says(data) == text
    n_ok = 0
    for b in flip_positions(len(data) * 8):
        bad = bytearray(data)
        bad[b >> 3] ^= 1 << (b & 7)
        want = zlib_says(bytes(bad))
        r = run_fresh(harness, bytes(bad), chunk_bytes=128)
        assert (r["rc"] == OK) == (want is not None), b
        if want is not None:
            assert r["out"] == want, b
            n_ok += 1
    assert n_ok >= 8


# ---- the finder at the default chunk_bytes ---------------------------------------------------------------------------------

def test_finder_on_a_realistic_stream(harness):
    """~7 MB of FASTQ-like text at level 6, memLevel 8, chunk_bytes = 16384.  Candidates that are not block starts are allowed;
    the chain must hold a chunk for at least 90 % of the spans that contain a true (non-final) dynamic block start."""
    text = fastq_like(55, 30000)
    data = deflated(text, 6)
    assert 6_500_000 < len(text) < 7_500_000 and len(data) < len(text) // 2
    starts, blocks = harness.walk(data, 80)
    chunk = 16384
    dyn = [b for b in starts if bit_at(data, b) == 0 and bit_at(data, b + 1) == 0 and bit_at(data, b + 2) == 1]
    true_spans = {(b // 8 - 10) // chunk for b in dyn} - {0}
    h = harness.open(0)
    try:
        rc, res, out = h.call(data, True, NONE)
        chain, cand = h.chain(), h.candidates()
    finally:
        h.close()
    assert rc == OK and out == text
    chain_spans = {(b // 8 - 10) // chunk for b in chain[1:]}
    assert set(chain[1:]) <= set(starts)
    share = len(true_spans & chain_spans) / len(true_spans)
    print(f"blocks {blocks}, spans {len(cand)}, spans with a true dynamic start {len(true_spans)}, n_candidates {res.n_candidates}, "
          f"n_false_starts {res.n_false_starts}, n_chunks {res.n_chunks}, share {share:.4f}")
    assert res.n_chunks == len(chain) and res.n_candidates == sum(c != NONE for c in cand)
    assert share >= 0.90
