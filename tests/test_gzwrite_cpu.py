"""The arithmetic of the device gzip writer (sailfish_amd/csrc/gzfmt.h, used by gzwrite.hip) compiled as plain C++ with g++
(tests/gzwrite_harness.cpp; nothing but libstdc++ is linked) and judged by Python's zlib: CRC-32 by slices, the length-limited
code builder, the serial encoder that the device stream is compared with byte for byte (tests/test_gpu_gzwrite.py), and its size
against zlib level 6.  No GPU."""
import functools
import gzip
import hashlib
import json
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK = 65536
STORED_OVERHEAD = 10          # kGzStoredOverhead: a 64 KB block that does not compress is two stored blocks of 5 header bytes each
FRAME = 10 + 5 + 8            # gzip header, the final empty stored block, CRC-32 + ISIZE


def build_harness(dirpath):
    exe = os.path.join(str(dirpath), "gzwrite_harness")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "sailfish_amd", "csrc"),
                           os.path.join(ROOT, "tests", "gzwrite_harness.cpp"), "-o", exe])
    return exe


def host_encode(exe, dirpath, data, writes=()):
    """the serial encoder's gzip stream for `data`, written in pieces of `writes` bytes; returns (stream, stats dict)"""
    src, dst = os.path.join(str(dirpath), "in.bin"), os.path.join(str(dirpath), "out.gz")
    with open(src, "wb") as f:
        f.write(data)
    r = subprocess.run([exe, "enc", src, dst] + [str(w) for w in writes], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    t = r.stdout.split()
    with open(dst, "rb") as f:
        return f.read(), {t[i]: int(t[i + 1]) for i in range(0, len(t), 2)}


def check_stream(gz, payload):
    """one gzip member that inflates to `payload` under zlib and gzip; the trailer is CRC-32 and ISIZE of the payload"""
    d = zlib.decompressobj(31)
    out = d.decompress(gz) + d.flush()
    assert d.eof and d.unused_data == b"" and out == payload
    assert gzip.decompress(gz) == payload
    crc, isize = struct.unpack("<II", gz[-8:])
    assert crc == zlib.crc32(payload) and isize == len(payload) % 2 ** 32


def level6(raw):
    o = zlib.compressobj(6, zlib.DEFLATED, 31)
    return len(o.compress(raw) + o.flush())


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("gzh"))


def test_harness_links_no_zlib(harness):
    needed = re.findall(r"NEEDED.*\[(.*?)\]", subprocess.check_output(["readelf", "-d", harness], text=True))
    assert needed and all(n.startswith(("libstdc++", "libm.", "libgcc_s", "libc.")) for n in needed), needed


def test_crc32(harness, tmp_path):
    rng = np.random.default_rng(5)
    cases = [b"123456789", b"", b"\0", bytes(64), bytes(65)] + [rng.integers(0, 256, n, dtype=np.uint8).tobytes()
                                                                for n in (1, 63, 64, 65, 4113, 65536, 65537, 1_000_003)]
    for k, data in enumerate(cases):
        p = tmp_path / "c.bin"
        p.write_bytes(data)
        for seed in (1, 2, 3):
            got = subprocess.check_output([harness, "crc", str(p), str(seed + 10 * k)], text=True).split()
            assert [int(g, 16) for g in got] == [zlib.crc32(data)] * 3, (k, seed, got)
    assert zlib.crc32(b"123456789") == 0xCBF43926


def _canonical(lens):
    """RFC 1951 3.2.2: symbol -> (code, length)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l); nxt[l] += 1
    return out


def test_code_builder(harness, tmp_path):
    rng = np.random.default_rng(6)
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])
    hists = []
    for max_bits, n in ((15, 286), (7, 19)):
        one = [0] * n; one[n // 2] = 7
        first = [0] * n; first[0] = 3
        two = [0] * n; two[1] = 5; two[n - 1] = 1
        hists += [(max_bits, h) for h in (one, first, two, [0] * n, [1] * n, list(range(1, n + 1)),
                                          (fib[:n] + [0] * n)[:n], (fib[:30][::-1] + [1] * n)[:n],
                                          [int(x) for x in 2 ** rng.integers(0, 24, n)])]
        for _ in range(40):
            h = rng.integers(0, 1000, n) * (rng.random(n) < rng.random())
            hists.append((max_bits, [int(x) for x in h]))
        for _ in range(20):
            hists.append((max_bits, [int(x) for x in rng.geometric(0.001, n) ** 2 * (rng.random(n) < 0.7)]))
    p = tmp_path / "h.txt"
    p.write_text("".join(f"{mb} {len(h)} " + " ".join(map(str, h)) + "\n" for mb, h in hists))
    lines = subprocess.check_output([harness, "huff", str(p)], text=True).strip().split("\n")
    assert len(lines) == 2 * len(hists)
    saw_limit = False
    for i, (max_bits, h) in enumerate(hists):
        lens = [int(x) for x in lines[2 * i].split()[1:]]
        codes = [int(x) for x in lines[2 * i + 1].split()[1:]]
        used = [s for s, f in enumerate(h) if f]
        assert all(lens[s] > 0 for s in used) and max(lens) <= max_bits
        coded = [s for s, l in enumerate(lens) if l]
        if len(used) >= 2:
            assert coded == used
        else:                               # zlib's form: the code is filled up to two symbols of one bit
            assert len(coded) == 2 and all(lens[s] == 1 for s in coded) and set(used) <= set(coded)
        assert sum(2 ** (max_bits - l) for l in lens if l) == 2 ** max_bits          # Kraft sum exactly 1
        saw_limit |= max(lens) == max_bits and len(used) > 2
        # rarer symbols never get shorter codes
        for a in used:
            for b in used:
                assert not (h[a] < h[b] and lens[a] < lens[b])
        # the harness's codes are the canonical ones, bit-reversed, and a table-driven decoder reads every symbol back
        canon = _canonical(lens)
        table = {}
        for s in coded:
            c, l = canon[s]
            assert codes[s] == int(format(c, f"0{l}b")[::-1], 2)
            table[(l, c)] = s
        bits = []
        for s in coded:
            bits += [(codes[s] >> k) & 1 for k in range(lens[s])]           # sent from bit 0
        got, c, l = [], 0, 0
        for b in bits:
            c, l = (c << 1) | b, l + 1
            if (l, c) in table:
                got.append(table[(l, c)]); c = l = 0
        assert got == coded and l == 0
    assert saw_limit


def _runs(r):
    return b"a" + b"b" * r + b"c" + b"d" * (r + 1) + b"e" + b"\0" * r


def round_trip_cases():
    rng = np.random.default_rng(7)
    cases = {"empty": b"", "one": b"\x07", "zeros": bytes(3 * BLOCK + 17), "block": bytes(BLOCK), "block+1": b"\1" * (BLOCK + 1),
             "ramp": bytes(range(256)) * 300}
    for r in (2, 3, 258, 259, 260):
        cases[f"run{r}"] = _runs(r)
    # runs across every block boundary: a long run of one byte interrupted just before and just after the boundaries
    edge = bytearray(b"\5" * (4 * BLOCK + 300))
    for b in (1, 2, 3, 4):
        for d in (-259, -3, -2, -1, 1, 2, 3, 258):
            edge[b * BLOCK + d] = 9
    cases["edges"] = bytes(edge)
    for n in (BLOCK - 1, BLOCK + 2, 2 * BLOCK + 258):
        cases[f"sparse{n}"] = (rng.integers(0, 9, n) * (rng.random(n) < 0.2)).astype(np.uint8).tobytes()
    return cases


def test_serial_encoder_round_trips(harness, tmp_path):
    cases = round_trip_cases()
    for name, data in cases.items():
        gz, st = host_encode(harness, tmp_path, data)
        check_stream(gz, data)
        assert st["bytes_in"] == len(data) and st["bytes_out"] == len(gz) and st["blocks"] == -(-len(data) // BLOCK), name
    gz, _ = host_encode(harness, tmp_path, cases["zeros"])
    assert len(gz) < 400


def random_cases():
    """random bytes of three sizes, then float64 mantissas"""
    rng = np.random.default_rng(8)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (1000, BLOCK, 5 * BLOCK + 123)] + [rng.random(100_000).tobytes()]


def test_random_bytes_are_stored(harness, tmp_path):
    *stored, floats = random_cases()
    for data in stored:
        n = len(data)
        gz, st = host_encode(harness, tmp_path, data)
        check_stream(gz, data)
        assert st["stored"] == st["blocks"] and len(gz) <= n + STORED_OVERHEAD * st["blocks"] + FRAME
    data = floats                                        # float64 mantissas: must not grow beyond the stated overhead
    gz, st = host_encode(harness, tmp_path, data)
    check_stream(gz, data)
    assert len(gz) <= len(data) + STORED_OVERHEAD * st["blocks"] + FRAME


SEVERAL_WRITES = (1, 65535, 0, 65537, 100_000, 7)


def several_writes_case():
    rng = np.random.default_rng(9)
    return (rng.integers(0, 40, 400_000) * (rng.random(400_000) < 0.3)).astype(np.uint8).tobytes()


def test_several_writes_give_one_member(harness, tmp_path):
    data = several_writes_case()
    gz, st = host_encode(harness, tmp_path, data, writes=SEVERAL_WRITES)
    check_stream(gz, data)
    assert st["blocks"] == 1 + 1 + 2 + 2 + 1 + 3


@functools.lru_cache(maxsize=None)
def _oracle_samples(M, P, R, n_gibbs, n_boot):
    from oracle import oracle as O
    from sailfish_amd import synth
    ref_len, ids, off = synth.workload(M, P, R)
    b = O.EqBuilder()
    b.add_batch(ids.numpy().view(np.uint32), off.numpy().view(np.uint32).astype(np.uint64))
    rp, ii, cc, _ = b.finish()
    eff = O.efflen_smoothed(ref_len.numpy().view(np.uint32), O.cf_gaussian())
    rc, alpha, mass, _ = O.em_optimize(eff, rp, ii, cc, R)
    assert rc == 0
    out = {"alpha": alpha}
    rc, out["gibbs"] = O.gibbs(eff, mass, rp, ii, cc, R, n_gibbs)
    if n_boot:
        rc, out["bootstrap"], _ = O.bootstrap(eff, rp, ii, cc, n_boot, max_iter=2000)
    return {k: np.ascontiguousarray(v).tobytes() for k, v in out.items()}


def test_oracle_samples_round_trip(built, harness, tmp_path):
    for name, raw in _oracle_samples(500, 2000, 50_000, 8, 0).items():
        gz, _ = host_encode(harness, tmp_path, raw, writes=(len(raw) // 3,))
        check_stream(gz, raw)


def level6_cases():
    s = dict(_oracle_samples(5000, 40000, 1_000_000, 16, 4))
    a = np.frombuffer(s["alpha"], np.float64).copy()
    a[np.random.default_rng(10).random(a.size) < 0.9] = 0.0
    s["alpha_90pct_zero"] = a.tobytes()
    return s


def test_size_against_zlib_level_6(built, harness, tmp_path):
    """the cap of the GPU size test: no larger than 1.10 x zlib level 6, on the oracle's Gibbs draws, its EM abundance vector,
    its EM bootstrap replicates and that vector with 90 % zeros"""
    for name, raw in level6_cases().items():
        gz, st = host_encode(harness, tmp_path, raw)
        check_stream(gz, raw)
        ratio = len(gz) / level6(raw)
        print(f"{name}: {len(raw)} B -> {len(gz)} B, {ratio:.3f} x level 6, {st['stored']} of {st['blocks']} blocks stored")
        assert ratio <= 1.10, (name, ratio)


DIGESTS = os.path.join(ROOT, "tests", "golden", "deflate_writer_digests.json")


def digest_sets():
    """name -> (payload, write cuts): every input the tests above hand to the serial encoder.  Needs the built oracle."""
    sets = {f"round_trip/{k}": (v, ()) for k, v in round_trip_cases().items()}
    sets.update({f"random/{i}": (v, ()) for i, v in enumerate(random_cases())})
    sets["several_writes"] = (several_writes_case(), SEVERAL_WRITES)
    sets.update({f"oracle_small/{k}": (v, (len(v) // 3,)) for k, v in _oracle_samples(500, 2000, 50_000, 8, 0).items()})
    sets.update({f"level6/{k}": (v, ()) for k, v in level6_cases().items()})
    return sets


def stream_digests(encode, sets):
    """name -> sha256 and length of encode(payload, write cuts), and of the payload itself; a list of cases is digested as one
    stream, in order"""
    out = {}
    for name, cases in sets.items():
        h, hi, n, ni = hashlib.sha256(), hashlib.sha256(), 0, 0
        for data, writes in cases if isinstance(cases, list) else [cases]:
            stream = encode(data, writes)
            h.update(stream); hi.update(data); n += len(stream); ni += len(data)
        out[name] = {"sha256": h.hexdigest(), "length": n, "input_sha256": hi.hexdigest(), "input_length": ni}
    return out


def test_serial_stream_digests(built, harness, tmp_path):
    """the serial encoder still writes the streams it wrote when tests/golden/deflate_writer_digests.json was recorded: zlib accepts
    any valid stream, this pins the bytes that tests/test_gpu_gzwrite.py compares the device with"""
    with open(DIGESTS) as f:
        want = json.load(f)["gzip"]
    got = stream_digests(lambda data, writes: host_encode(harness, tmp_path, data, writes)[0], digest_sets())
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
