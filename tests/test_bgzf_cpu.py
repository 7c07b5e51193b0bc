"""The rules of the device BGZF inflater (sailfish_amd/csrc/bgzfmt.h, used by bgzf_read.hip) compiled as plain C++ with g++
(tests/bgzf_harness.cpp, a shared object; nothing but libstdc++ is linked) and judged by zlib: round trips of what
gzfile.write_bgzf and zlib lay out, members assembled bit by bit that zlib's deflate never emits, one member per error kind, and
agreement with gzip.decompress on 1200 single-bit flips.  The file sets are shared with tests/test_gpu_bgzf.py.  No GPU."""
import ctypes as C
import gzip
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from test_readfile_cpu import fastq_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_FORMAT = 0, 8
(BAD_HEADER, TRUNCATED, BAD_BLOCK_TYPE, STORED_LEN, BAD_CODE_LENGTHS, BAD_SYMBOL, DISTANCE_TOO_FAR, SIZE_MISMATCH,
 CRC_MISMATCH) = range(1, 10)
NONE = 2 ** 64 - 1
BC_HEADER = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"


# ---- the harness -----------------------------------------------------------------------------------------------------------

def build_harness(dirpath):
    so = os.path.join(str(dirpath), "libbgzf_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "sailfish_amd", "csrc"), os.path.join(ROOT, "tests", "bgzf_harness.cpp"), "-o", so])
    return so


class Result(C.Structure):             # sfgpu_bgzf_result
    _fields_ = [("n_members", C.c_uint64), ("consumed", C.c_uint64), ("n_bytes_out", C.c_uint64), ("n_stored_blocks", C.c_uint64),
                ("n_fixed_blocks", C.c_uint64), ("n_dynamic_blocks", C.c_uint64), ("error_member", C.c_uint64),
                ("error_kind", C.c_int32), ("pad_", C.c_int32), ("ms_copy", C.c_double), ("ms_kernels", C.c_double)]


def unpack(rc, res, out):
    return dict(rc=rc, out=bytes(out[: res.n_bytes_out]) if rc == OK else b"", n_members=int(res.n_members), consumed=int(res.consumed),
                n_bytes_out=int(res.n_bytes_out), blocks=(int(res.n_stored_blocks), int(res.n_fixed_blocks), int(res.n_dynamic_blocks)),
                error=(res.error_kind, int(res.error_member)))


class Harness:
    def __init__(self, so):
        self.so = so
        lib = C.CDLL(so)
        self.fn = lib.bgzf_harness_inflate
        self.fn.restype = C.c_int
        self.fn.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(Result)]
        self.one = lib.bgzf_harness_member
        self.one.restype = C.c_int
        self.one.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]

    def inflate(self, data, final=1, cap=None, n_bytes=None):
        """-> dict(rc, out, n_members, consumed, n_bytes_out, blocks=(stored, fixed, dynamic), error=(kind, member))"""
        data = bytes(data)
        n = len(data) if n_bytes is None else n_bytes
        room = 65536 * (n // 26 + 1) if cap is None else cap
        out = np.zeros(min(room, 1 << 28) + 1, np.uint8)
        res = Result()
        rc = self.fn(data, n, int(final), out.ctypes.data, room, C.byref(res))
        return unpack(rc, res, out)

    def member(self, data):
        """one member alone -> (kind, payload, (stored, fixed, dynamic))"""
        out = np.zeros(65536, np.uint8)
        n_out, blocks = C.c_uint32(), (C.c_uint32 * 3)()
        kind = self.one(bytes(data), len(data), out.ctypes.data, 65536, C.byref(n_out), blocks)
        return kind, bytes(out[: n_out.value]), tuple(blocks)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return Harness(build_harness(tmp_path_factory.mktemp("bgzh")))


# ---- members ---------------------------------------------------------------------------------------------------------------

def frame(body, payload, extra_front=b"", crc=None, isize=None, bsize=None):
    """a BGZF member around a raw DEFLATE body; the keyword arguments overrule what would be right"""
    extra = extra_front + b"BC\x02\0"
    total = 12 + len(extra) + 2 + len(body) + 8
    bs = struct.pack("<H", (total - 1 if bsize is None else bsize) & 0xffff)
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", len(extra) + 2) + extra + bs + body
            + struct.pack("<II", zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize))


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bits:
    """a DEFLATE bit writer: fields from bit 0 up, Huffman code words from their first bit"""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n_bits):
        self.acc |= (value & ((1 << n_bits) - 1)) << self.n
        self.n += n_bits

    def code(self, word, n_bits):
        self.put(int(format(word, f"0{n_bits}b")[::-1], 2), n_bits)

    def fixed_sym(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def fixed_match(self, length, dist):
        i = max(k for k in range(29) if LEN_BASE[k] <= length and (k == 28 or length != 258))
        self.fixed_sym(257 + i); self.put(length - LEN_BASE[i], LEN_EXTRA[i])
        j = max(k for k in range(30) if DIST_BASE[k] <= dist)
        self.code(j, 5); self.put(dist - DIST_BASE[j], DIST_EXTRA[j])

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def fixed_block(tokens, final=1, eob=True):
    """tokens: ints (literals) and (length, distance) pairs -> (body, payload)"""
    b, out = Bits(), bytearray()
    b.put(final, 1); b.put(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            b.fixed_match(*t)
            for _ in range(t[0]):
                out.append(out[-t[1]])
        else:
            b.fixed_sym(t); out.append(t)
    if eob:
        b.fixed_sym(256)
    return b.bytes(), bytes(out)


def text_3000():
    return fastq_text(np.random.default_rng(41), 3000, lens=[100] * 3000)[0]


def flushed_member(payload, at):
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = z.compress(payload[:at]) + z.flush(zlib.Z_FULL_FLUSH) + z.compress(payload[at:]) + z.flush()
    return frame(body, payload)


ROUND_TRIP_NAMES = ["level0", "level1", "level6", "level9", "fixed", "huffman_only", "rle", "full_flush_100", "full_flush_20000",
                    "full_flush_20001", "random_65000", "zeros_65280"]


def round_trip_files():
    """name -> (file bytes, payload, the block types that must occur, those that must not)"""
    import io
    from sailfish_amd import gzfile
    text = text_3000()
    assert 600_000 < len(text) < 660_000
    files = {}

    def written(data, **kw):
        f = io.BytesIO()
        gzfile.write_bgzf(f, data, **kw)
        return f.getvalue()
    for level in (0, 1, 6, 9):
        files[f"level{level}"] = (written(text, level=level), text, (0,) if level == 0 else (2,), (1, 2) if level == 0 else (0, 1))
    files["fixed"] = (written(text, strategy=zlib.Z_FIXED), text, (1,), (0, 2))
    files["huffman_only"] = (written(text, strategy=zlib.Z_HUFFMAN_ONLY), text, (2,), (0, 1))
    files["rle"] = (written(text, strategy=zlib.Z_RLE), text, (2,), (0, 1))
    for at in (100, 20000, 20001):
        files[f"full_flush_{at}"] = (flushed_member(text[:60000], at) + gzfile.BGZF_EOF, text[:60000], (0, 2), ())
    noise = np.random.default_rng(42).integers(0, 256, 65000, dtype=np.uint8).tobytes()
    files["random_65000"] = (written(noise), noise, (0,), (2,))
    files["zeros_65280"] = (written(bytes(65280)), bytes(65280), (2,), (0,))
    assert sorted(files) == sorted(ROUND_TRIP_NAMES)
    return files


def hand_members():
    """name -> (member, payload): fixed-Huffman members that zlib's deflate does not emit"""
    rng = np.random.default_rng(43)
    lits = rng.integers(0, 256, 32768, dtype=np.uint8).tolist()
    out = {}
    body, payload = fixed_block(lits + [(258, 32768)])
    out["distance_32768"] = (frame(body, payload), payload)
    body, payload = fixed_block([ord("a"), (3, 1)])
    out["overlap_3_1"] = (frame(body, payload), payload)
    body, payload = fixed_block([7] + [(258, 1)] * 254 + [(3, 1)])
    assert len(payload) == 65536
    out["exactly_65536"] = (frame(body, payload), payload)
    body, payload = fixed_block(list(b"foreign subfield") + [(200, 7), (9, 16)])
    out["foreign_subfield"] = (frame(body, payload, extra_front=b"XY\x03\0abc"), payload)
    return out


def dynamic_header(hlit, hdist, cl_lens, symbols):
    """a final dynamic block up to the end of its code lengths: cl_lens = lengths of the code-length code by symbol (a dict),
    symbols = [(code-length symbol, extra value)]; canonical codes for the code-length code"""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    b = Bits()
    b.put(1, 1); b.put(2, 2); b.put(hlit - 257, 5); b.put(hdist - 1, 5)
    hclen = max(i for i in range(19) if cl_lens.get(order[i], 0)) + 1
    hclen = max(hclen, 4)
    b.put(hclen - 4, 4)
    for i in range(hclen):
        b.put(cl_lens.get(order[i], 0), 3)
    code, codes = 0, {}
    for ln in range(1, 8):
        for s in range(19):
            if cl_lens.get(s, 0) == ln:
                codes[s] = (code, ln); code += 1
        code <<= 1
    for s, ev in symbols:
        b.code(*codes[s])
        b.put(ev, {16: 2, 17: 3, 18: 7}.get(s, 0))
    return b


def error_members():
    """name -> (member, kind): one member per way of failing"""
    good_body, good = fixed_block(list(b"a good member, ") + [(40, 15)])
    ok = frame(good_body, good)
    out = {"no_bc": (ok.replace(b"BC\x02\0", b"BX\x02\0"), BAD_HEADER),
           "bsize_too_small": (frame(good_body, good, bsize=20), BAD_HEADER),
           "isize_65537": (frame(good_body, good, isize=65537), BAD_HEADER),
           "not_deflate": (ok[:2] + b"\x07" + ok[3:], BAD_HEADER),
           "stream_ends_early": (frame(good_body + b"\0\0", good), BAD_HEADER)}
    body, payload = fixed_block(list(b"no end of block"), eob=False)
    out["truncated"] = (frame(body, payload), TRUNCATED)
    out["truncated_empty_body"] = (frame(b"", b""), TRUNCATED)
    out["stored_runs_out"] = (frame(b"\x01\x05\0\xfa\xffabc", b"abc"), TRUNCATED)
    out["block_type_3"] = (frame(b"\x07\0\0", b""), BAD_BLOCK_TYPE)
    out["stored_len"] = (frame(b"\x01\x03\0\xfc\xfeabc", b"abc"), STORED_LEN)
    pad = bytes(40)
    b = Bits(); b.put(1, 1); b.put(2, 2); b.put(30, 5); b.put(0, 5); b.put(0, 4)
    out["hlit_287"] = (frame(b.bytes() + pad, b""), BAD_CODE_LENGTHS)
    b = Bits(); b.put(1, 1); b.put(2, 2); b.put(0, 5); b.put(30, 5); b.put(0, 4)
    out["hdist_31"] = (frame(b.bytes() + pad, b""), BAD_CODE_LENGTHS)
    out["repeat_without_previous"] = (frame(dynamic_header(257, 1, {16: 1, 8: 1}, [(16, 0)]).bytes() + pad, b""), BAD_CODE_LENGTHS)
    out["repeat_past_the_end"] = (frame(dynamic_header(257, 1, {18: 1, 8: 1}, [(18, 127), (18, 127)]).bytes() + pad, b""), BAD_CODE_LENGTHS)
    out["code_length_code_over_subscribed"] = (frame(dynamic_header(257, 1, {0: 1, 8: 1, 16: 1}, []).bytes() + pad, b""), BAD_CODE_LENGTHS)
    out["code_length_code_incomplete"] = (frame(dynamic_header(257, 1, {0: 2, 8: 2, 18: 2}, []).bytes() + pad, b""), BAD_CODE_LENGTHS)
    # 256 zeros, then a length for symbol 256 ... and without one
    out["no_code_for_256"] = (frame(dynamic_header(257, 1, {18: 1, 1: 1}, [(18, 127), (18, 108), (1, 0)]).bytes() + pad, b""),
                              BAD_CODE_LENGTHS)
    # literal code: 0 and 256 with one bit each and a third symbol with one bit: over-subscribed
    out["over_subscribed"] = (frame(dynamic_header(258, 1, {18: 2, 1: 2, 0: 1}, [(1, 0), (18, 127), (18, 106), (0, 0), (0, 0), (0, 0), (0, 0),
                                                                                (0, 0), (0, 0), (1, 0), (1, 0), (1, 0)]).bytes() + pad, b""),
                              BAD_CODE_LENGTHS)
    # literal code: 0 with one bit, 256 with two bits: incomplete, and not the single code zlib lets pass
    out["incomplete"] = (frame(dynamic_header(257, 1, {18: 2, 1: 2, 2: 2, 0: 2}, [(1, 0), (18, 127), (18, 106), (0, 0), (0, 0), (0, 0), (0, 0),
                                                                                (0, 0), (0, 0), (2, 0), (1, 0)]).bytes() + pad, b""),
                         BAD_CODE_LENGTHS)
    b = Bits(); b.put(1, 1); b.put(1, 2); b.fixed_sym(65); b.fixed_sym(286)
    out["length_symbol_286"] = (frame(b.bytes() + pad, b"A"), BAD_SYMBOL)
    b = Bits(); b.put(1, 1); b.put(1, 2); b.fixed_sym(65); b.fixed_sym(257); b.code(30, 5)
    out["distance_symbol_30"] = (frame(b.bytes() + pad, b"A"), BAD_SYMBOL)
    # the single one-bit literal/length code zlib accepts (256 alone): its other code word is nobody's
    b = dynamic_header(257, 1, {18: 1, 1: 1}, [(18, 127), (18, 107), (1, 0), (1, 0)]); b.put(1, 1)
    out["unassigned_code"] = (frame(b.bytes() + pad, b""), BAD_SYMBOL)
    b = Bits(); b.put(1, 1); b.put(1, 2); b.fixed_sym(65); b.fixed_match(3, 2); b.fixed_sym(256)
    out["distance_too_far"] = (frame(b.bytes(), b"A"), DISTANCE_TOO_FAR)
    out["isize_one_less"] = (frame(good_body, good, isize=len(good) - 1), SIZE_MISMATCH)
    out["isize_one_more"] = (frame(good_body, good, isize=len(good) + 1), SIZE_MISMATCH)
    out["crc"] = (frame(good_body, good, crc=zlib.crc32(good) ^ 0x100), CRC_MISMATCH)
    return out


def zlib_accepts(member):
    try:
        return True, gzip.decompress(member)
    except Exception:                  # noqa: BLE001  (zlib.error, gzip.BadGzipFile, EOFError: every way of saying no)
        return False, b""


# ---- tests -----------------------------------------------------------------------------------------------------------------

def test_harness_links_nothing_but_libstdcxx(harness):
    needed = re.findall(r"NEEDED.*\[(.*?)\]", subprocess.check_output(["readelf", "-d", harness.so], text=True))
    assert needed and all(n.startswith(("libstdc++", "libm.", "libgcc_s", "libc.")) for n in needed), needed


def test_write_bgzf_is_bgzf():
    import io
    from sailfish_amd import gzfile
    assert gzfile.bgzf_member(b"") == gzfile.BGZF_EOF == bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    text = text_3000()
    f = io.BytesIO()
    n = gzfile.write_bgzf(f, text)
    data = f.getvalue()
    assert n == len(data) and gzip.decompress(data) == text and data.endswith(gzfile.BGZF_EOF)
    p, members = 0, 0
    while p < len(data):
        assert data[p:p + 16] == BC_HEADER
        p += struct.unpack_from("<H", data, p + 16)[0] + 1
        members += 1
    assert p == len(data) and members == -(-len(text) // 65280) + 1 >= 10


@pytest.mark.parametrize("name", ROUND_TRIP_NAMES)
def test_round_trips(harness, name):
    data, payload, must, must_not = FILES()[name]
    assert gzip.decompress(data) == payload
    r = harness.inflate(data)
    assert r["rc"] == OK and r["error"] == (0, NONE) and r["out"] == payload
    assert r["consumed"] == len(data) and r["n_bytes_out"] == len(payload)
    eof = (0, 1, 0)                 # the EOF member is one empty fixed block
    assert all(r["blocks"][t] > eof[t] for t in must) and all(r["blocks"][t] == eof[t] for t in must_not), r["blocks"]
    if name == "level6":
        assert r["n_members"] >= 10 and r["blocks"][2] > r["n_members"] - 1        # members of more than one block
    if name.startswith("full_flush"):
        assert r["blocks"][0] == 1 and r["blocks"][2] >= 2                          # the empty stored block of the flush


_FILES = {}


def FILES():
    if not _FILES:
        _FILES.update(round_trip_files())
    return _FILES


def test_hand_assembled_members(harness):
    for name, (member, payload) in hand_members().items():
        assert gzip.decompress(member) == payload, name
        kind, out, blocks = harness.member(member)
        assert kind == 0 and out == payload and blocks == (0, 1, 0), (name, kind)


def test_error_kinds(harness):
    for name, (member, want) in error_members().items():
        if name not in ("no_bc", "bsize_too_small"):       # gzip members all the same: what is wrong is the BGZF framing
            assert not zlib_accepts(member)[0], name
        kind, _, _ = harness.member(member)
        assert kind == want, (name, kind, want)
        r = harness.inflate(member)
        assert r["rc"] == ERR_FORMAT and r["error"] == (want, 0), (name, r)
    assert set(k for _, k in error_members().values()) == set(range(1, 10))


def test_first_bad_member_in_file_order(harness):
    from sailfish_amd import gzfile
    errs = error_members()
    good = hand_members()["overlap_3_1"][0]
    data = good + good + errs["crc"][0] + good + errs["distance_too_far"][0] + errs["no_bc"][0] + gzfile.BGZF_EOF
    r = harness.inflate(data)
    assert r["rc"] == ERR_FORMAT and r["error"] == (CRC_MISMATCH, 2) and r["n_members"] == 5
    data = good + errs["block_type_3"][0] + errs["no_bc"][0] + good
    r = harness.inflate(data)
    assert r["error"] == (BAD_BLOCK_TYPE, 1) and r["n_members"] == 2
    data = good + good + errs["no_bc"][0] + good
    assert harness.inflate(data)["error"] == (BAD_HEADER, 2)
    # a member cut by the end of the input: left for the next call, or TRUNCATED when the input is final
    data = good + good
    r = harness.inflate(data, final=0, n_bytes=len(data) - 1)
    assert r["rc"] == OK and r["consumed"] == len(good) and r["n_members"] == 1 and r["out"] == b"aaaa"
    r = harness.inflate(data, final=1, n_bytes=len(data) - 1)
    assert r["rc"] == ERR_FORMAT and r["error"] == (TRUNCATED, 1)
    r = harness.inflate(data, cap=7)
    assert r["rc"] == OK and r["n_members"] == 1 and r["consumed"] == len(good)


def flip_members():
    from sailfish_amd import gzfile
    text = text_3000()
    m = [gzfile.bgzf_member(text[:1500], 0), gzfile.bgzf_member(text[:1900], 6, zlib.Z_FIXED), gzfile.bgzf_member(text[:2600], 6)]
    assert all(len(x) <= 2048 for x in m)
    return m


def test_single_bit_flips_agree_with_zlib(harness):
    rng = np.random.default_rng(44)
    accepted = 0
    for k, member in enumerate(flip_members()):
        kind, out, blocks = harness.member(member)
        assert kind == 0 and blocks[k] == 1 and sum(blocks) == 1 and out == gzip.decompress(member)
        for pos in rng.integers(18 * 8, len(member) * 8, 400).tolist():
            bad = bytearray(member)
            bad[pos >> 3] ^= 1 << (pos & 7)
            ok, want = zlib_accepts(bytes(bad))
            kind, out, _ = harness.member(bytes(bad))
            assert (kind == 0) == ok, (k, pos, kind, ok)
            if ok:
                assert out == want, (k, pos)
                accepted += 1
    assert accepted < 200        # most flips are fatal; the padding bits behind a block are not
