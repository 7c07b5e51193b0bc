"""The device inflater of ordinary gzip (sfgpu_gzrd_*, sailfish_amd/csrc/gz_read.hip) against the serial run of the same contract
header (tests/gzrd_harness.cpp) in everything it reports, call by call; then the file driver (readfile.ReadFile with
inflate="device" on an ordinary gzip file) against the same text as a plain file, and quantify_files end to end."""
import ctypes as C
import gzip
import os
import zlib

import numpy as np
import pytest

from test_bgzf_cpu import text_3000
from test_gpu_bgzf import read_all
from test_gpu_readfile import _render, _sample
from test_gzrd_cpu import (CHUNK, ERR_FORMAT, OK, ROUND_TRIP_NAMES, Harness, build_harness, deflated, error_files, false_start_file,
                           flip_file, flip_positions, round_trip_files, run, stream_cuts)

KEYS = ("rc", "out", "consumed", "n_bytes_out", "n_chunks", "n_candidates", "n_false_starts", "blocks", "member_end", "error", "calls", "grown")
OFFSET = 3                            # the payload is written at an odd offset into a guarded buffer


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return Harness(build_harness(tmp_path_factory.mktemp("gzrdh")))


@pytest.fixture(scope="module")
def files():
    return round_trip_files()


class DeviceHandle:
    """HarnessHandle's call() over sfgpu_gzrd_*"""

    def __init__(self, gpu, chunk_bytes):
        import torch
        from sailfish_amd import _lib
        self.torch, self._lib, self.L, self.gpu, self.z = torch, _lib, _lib.lib(), gpu, C.c_void_p()
        with torch.cuda.device(gpu):
            _lib.check(self.L.sfgpu_gzrd_open(C.byref(self.z), chunk_bytes))

    def call(self, buf, final, cap):
        torch, _lib = self.torch, self._lib
        res = _lib.GzrdResult()
        with torch.cuda.device(self.gpu):
            rc = self.L.sfgpu_gzrd_plan_host(self.z, buf, len(buf), int(final), cap, C.byref(res), _lib.current_stream_ptr())
            if rc not in (OK, ERR_FORMAT):
                _lib.check(rc)
            if rc == ERR_FORMAT and res.n_chunks == 0:
                return rc, res, b""
            n = int(res.n_bytes_out)
            out = torch.full((OFFSET + n + 64,), 0xA5, dtype=torch.uint8, device=self.gpu)
            rc = self.L.sfgpu_gzrd_emit(self.z, _lib.ptr(out[OFFSET:]), C.byref(res), _lib.current_stream_ptr())
            if rc not in (OK, ERR_FORMAT):
                _lib.check(rc)
        host = out.cpu().numpy()
        assert (host[:OFFSET] == 0xA5).all() and (host[OFFSET + n:] == 0xA5).all()      # nothing outside [0, n_bytes_out) was touched
        for k in ("ms_copy", "ms_find", "ms_decode", "ms_propagate", "ms_emit"):
            assert getattr(res, k) >= 0
        return rc, res, host[OFFSET:OFFSET + n].tobytes()

    def close(self):
        if self.z:
            self.L.sfgpu_gzrd_close(self.z); self.z = None


def both(gpu, harness, data, cuts=(), cap=None, chunk_bytes=CHUNK, what=""):
    """the same calls on the device and in the harness -> the device's totals, equal to the harness's in every reported field"""
    h, d = harness.open(chunk_bytes), DeviceHandle(gpu, chunk_bytes)
    try:
        want, got = run(h, data, cuts, cap), run(d, data, cuts, cap)
    finally:
        h.close(); d.close()
    for k in KEYS:
        assert got[k] == want[k], (k, got[k] if k != "out" else len(got[k]), want[k] if k != "out" else len(want[k]), what)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROUND_TRIP_NAMES)
def test_device_equals_the_harness(gpu, harness, files, name):
    data, payload = files[name]
    got = both(gpu, harness, data, what=name)
    assert got["rc"] == OK and got["out"] == payload and got["consumed"] == len(data)


@pytest.mark.gpu
def test_streaming_cuts(gpu, harness, files):
    data, payload = files["level6_mem1"]
    got = both(gpu, harness, data, stream_cuts(data))
    assert got["rc"] == OK and got["out"] == payload and got["calls"] > len(data) // 997


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 5000])
def test_capacities(gpu, harness, files, cap):
    data, payload = files["level6_mem1"]
    got = both(gpu, harness, data, cap=cap)
    assert got["rc"] == OK and got["out"] == payload
    assert (got["grown"] >= 1) == (cap == 1)


@pytest.mark.gpu
def test_false_start(gpu, harness):
    data, payload, _ = false_start_file()
    got = both(gpu, harness, data)
    assert got["rc"] == OK and got["out"] == payload and got["n_false_starts"] >= 1


@pytest.mark.gpu
def test_error_files(gpu, harness):
    for name, (data, kind) in error_files().items():
        got = both(gpu, harness, data, what=name)
        assert got["rc"] == ERR_FORMAT and got["error"][0] == kind, name
    data = deflated(text_3000()[:20000], 6, 31, 1)
    for cut in (5, 300, len(data) // 2, len(data) - 9, len(data) - 1):
        got = both(gpu, harness, data[:cut], chunk_bytes=64, what=cut)
        assert got["rc"] == ERR_FORMAT and got["error"][0] == 2


@pytest.mark.gpu
def test_300_bit_flips(gpu, harness):
    data, text = flip_file()
    n_ok = 0
    for b in flip_positions(len(data) * 8)[:300]:
        bad = bytearray(data)
        bad[b >> 3] ^= 1 << (b & 7)
        got = both(gpu, harness, bytes(bad), chunk_bytes=128, what=b)
        n_ok += got["rc"] == OK
        if got["rc"] == OK:
            assert got["out"] == text
    assert n_ok >= 8


@pytest.mark.gpu
def test_default_chunk_bytes(gpu, harness, files):
    text = text_3000()
    for data, payload in ((deflated(text, 6), text), files["far_matches_32700"], files["far_matches_32500"]):
        got = both(gpu, harness, data, chunk_bytes=0)
        assert got["rc"] == OK and got["out"] == payload and got["calls"] == 2       # one call, and one that finds the end
    from sailfish_amd import _lib
    z = C.c_void_p()
    assert _lib.lib().sfgpu_gzrd_open(C.byref(z), 63) == 5                          # SFGPU_ERR_RANGE


# ---- ReadFile ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def text_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gz_files")
    text = text_3000()
    (d / "reads.fastq").write_bytes(text)
    (d / "reads.fastq.gz").write_bytes(deflated(text, 6))
    return d, text


@pytest.fixture(scope="module")
def plain_result(gpu, text_files):
    d, _ = text_files
    return read_all(d / "reads.fastq", gpu, 1 << 40)


@pytest.mark.gpu
@pytest.mark.parametrize("block_bytes", [20_000, 100_000, 32 << 20])
@pytest.mark.parametrize("batch", [1, 7, 1000, 1 << 40])
def test_read_file_device_gzip_equals_plain(gpu, text_files, plain_result, block_bytes, batch):
    d, text = text_files
    b, o, names, inflate, stats = read_all(d / "reads.fastq.gz", gpu, batch, block_bytes=block_bytes, inflate="device")
    assert inflate == "device" and plain_result[3] is None
    assert np.array_equal(b, plain_result[0]) and np.array_equal(o, plain_result[1]) and names == plain_result[2]
    assert stats["chunks"] > 1 and stats["members"] == 1 and stats["bytes_compressed"] == os.path.getsize(d / "reads.fastq.gz")
    assert stats["candidates"] >= 1 and stats["ms_inflate"] > 0 and stats["ms_find"] > 0


@pytest.mark.gpu
def test_read_file_many_members_and_errors(gpu, text_files, plain_result, tmp_path):
    from sailfish_amd import readfile
    d, text = text_files
    # members that end inside records, padding behind the last
    cuts = [0, 1000, 250_000, 250_001, len(text)]
    (tmp_path / "members.gz").write_bytes(b"".join(gzip.compress(text[a:b], 6) for a, b in zip(cuts, cuts[1:])) + bytes(100))
    b, o, names, inflate, stats = read_all(tmp_path / "members.gz", gpu, 1000, block_bytes=100_000, inflate="device")
    assert inflate == "device" and stats["members"] == 4 and stats["bytes_compressed"] == os.path.getsize(tmp_path / "members.gz")
    assert np.array_equal(b, plain_result[0]) and np.array_equal(o, plain_result[1]) and names == plain_result[2]
    # "auto" keeps the host for an ordinary gzip file
    with readfile.ReadFile(d / "reads.fastq.gz", gpu) as rf:
        assert rf.inflate == "host"
    with pytest.raises(ValueError, match="inflate must be"):
        readfile.ReadFile(d / "reads.fastq.gz", gpu, inflate="nonsense")
    data = bytearray((d / "reads.fastq.gz").read_bytes())
    data[-8] ^= 1                                         # the CRC
    (tmp_path / "bad_crc.gz").write_bytes(data)
    for block in (30_000, 32 << 20):
        with readfile.ReadFile(tmp_path / "bad_crc.gz", gpu, block_bytes=block, inflate="device") as rf:
            with pytest.raises(ValueError, match=r"bad_crc\.gz: gzip member 0 \(byte \d+ of the file\).*CRC-32 mismatch \(kind 9\)"):
                rf.read(1 << 40)
    (tmp_path / "cut.gz").write_bytes(bytes(data[: len(data) // 2]))
    with readfile.ReadFile(tmp_path / "cut.gz", gpu, inflate="device") as rf:
        with pytest.raises(ValueError, match=r"cut\.gz: gzip member 0 \(byte \d+ of the file\).*ends inside a member \(kind 2\)"):
            rf.read(1 << 40)


@pytest.mark.gpu
def test_quantify_files_from_gzip_on_the_device_writes_the_same_quant_sf(gpu, tmp_path):
    import sailfish_amd as sf
    names, seqs, r1, r2 = _sample()
    plain = _render(tmp_path, names, seqs, r1, r2)
    opts = dict(batch_reads=3000, cmd_options={"libType": "IU"}, device=gpu)
    rc, exp = sf.mapper.quantify_files(*plain, "IU", str(tmp_path / "plain"), sf.SailfishOpts(numFragSamples=5000), **opts)
    assert rc == 0 and exp.numMappedFragments() == 10000
    zipped = []
    for p in plain:
        zipped.append(str(p) + ".gz")
        with open(zipped[-1], "wb") as f:
            f.write(deflated(p.read_bytes(), 6))
        assert zlib.decompress(open(zipped[-1], "rb").read(), 31) == p.read_bytes()
    rc, exp = sf.mapper.quantify_files(*zipped, "IU", str(tmp_path / "gz"), sf.SailfishOpts(numFragSamples=5000), inflate="device", **opts)
    assert rc == 0 and exp.numMappedFragments() == 10000
    assert (tmp_path / "gz" / "quant.sf").read_bytes() == (tmp_path / "plain" / "quant.sf").read_bytes()


@pytest.mark.gpu
def test_a_plan_that_is_refused_is_no_plan(gpu):
    """more than 65536 spans in one call: SFGPU_ERR_RANGE, and an emit behind it has nothing to emit (SFGPU_ERR_STATE)"""
    import torch
    from sailfish_amd import _lib
    L, z, res = _lib.lib(), C.c_void_p(), _lib.GzrdResult()
    small = deflated(text_3000()[:5000], 6)
    data = small + bytes(64 * 65537)
    with torch.cuda.device(gpu):
        _lib.check(L.sfgpu_gzrd_open(C.byref(z), 64))
        try:
            assert L.sfgpu_gzrd_plan_host(z, small, len(small), 0, 1 << 30, C.byref(res), None) == OK and res.n_chunks >= 1
            assert L.sfgpu_gzrd_plan_host(z, data, len(data), 0, 1 << 30, C.byref(res), None) == _lib.ERR_RANGE
            assert L.sfgpu_gzrd_emit(z, None, C.byref(res), None) == _lib.ERR_STATE
        finally:
            L.sfgpu_gzrd_close(z)


@pytest.mark.gpu
def test_read_file_delivers_the_records_in_front_of_a_corrupt_block(gpu, harness, text_files, plain_result, tmp_path):
    from sailfish_amd import readfile
    d, text = text_files
    data = bytearray((d / "reads.fastq.gz").read_bytes())
    starts, _ = harness.walk(bytes(data), 80)
    at = starts[len(starts) // 2]
    for b in (at + 1, at + 2):                            # BTYPE 2 -> 3 in the middle of the file
        data[b >> 3] |= 1 << (b & 7)
    (tmp_path / "bad_block.gz").write_bytes(data)
    got = 0
    with readfile.ReadFile(tmp_path / "bad_block.gz", gpu, inflate="device") as rf:
        with pytest.raises(ValueError, match=r"bad_block\.gz: gzip member 0 \(byte \d+ of the file\).*block type 3 \(kind 3\)"):
            for _ in range(10):
                b, o = rf.read(1000)
                n = o.numel() - 1
                lo, hi = int(plain_result[1][got]), int(plain_result[1][got + n])
                assert n and np.array_equal(b.cpu().numpy()[: hi - lo], plain_result[0][lo:hi])
                got += n
    assert 500 <= got < 3000                              # the good chunks came first, whole records of them
