"""The device BGZF writer (sfgpu_bgzw_open / sfgpu_bgzw_write_device / sfgpu_bgzw_close, sailfish_amd/csrc/bgzf_write.hip) on the
GPU: the device file equals the serial host encoder's file byte for byte (tests/bgzw_harness.cpp over the same bgzwfmt.h, which
tests/test_bgzw_cpu.py holds against zlib, gzip and the project's serial inflater), for every input of the CPU tests at different
member indices, unaligned sources, split writes and forced chunks; the device inflater reads what the device wrote."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import bamwrite_corpus
from test_bgzw_cpu import EOF, STEP, Harness, _planted, _repeat_at, build_harness, check_file, inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return Harness(build_harness(tmp_path_factory.mktemp("bgzwh")))


def _dev(data, gpu, shift=0):
    """`data` on the device, its first byte `shift` bytes behind a 256-byte boundary"""
    t = torch.zeros(len(data) + shift, dtype=torch.uint8, device=gpu)
    if len(data):
        t[shift:] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(gpu)
    return t[shift:]


def _collect(tensors, chunk_bytes=0, refuse_at=None):
    """the C entries with a sink that keeps every chunk; returns (statuses of the writes, status of close, result dict, chunks)"""
    from sailfish_amd import _lib
    chunks = []

    def sink(addr, n, _user):
        if refuse_at is not None and len(chunks) + 1 == refuse_at:
            chunks.append(None)
            return 1
        chunks.append(bytes((C.c_char * n).from_address(addr)))
        return 0
    cb = _lib.TEXT_SINK(sink)
    L = _lib.lib()
    h = C.c_void_p()
    assert L.sfgpu_bgzw_open(C.byref(h), cb, None, chunk_bytes) == _lib.OK
    rcs = [L.sfgpu_bgzw_write_device(h, _lib.ptr(t) if t.numel() else None, t.numel(), _lib.current_stream_ptr()) for t in tensors]
    res = _lib.BgzwResult()
    rc_close = L.sfgpu_bgzw_close(h, C.byref(res))
    return rcs, rc_close, res.as_dict(), chunks


def _all_inputs(P):
    """every input of the CPU tests: the edge cases, a repeat at the lowest and highest distance of every distance symbol, a repeat
    of every length at and across a slice start"""
    cases = dict(inputs(P))
    d = 1
    for sym in range(30):
        eb = max(0, sym // 2 - 1)
        for dist in {min(d, P - 4), min(d + (1 << eb) - 1, P - 4)}:
            cases[f"dist{dist}"] = _repeat_at(P, dist)[0]
        d += 1 << eb
    rng = np.random.default_rng(34)
    for length in range(3, 259):
        for at in (2 * STEP, 2 * STEP + 61):
            cases[f"len{length}@{at}"] = _planted(rng, at + length + 9, at, STEP + 11, length)
    return cases


def test_device_bytes_equal_serial_bytes(built, gpu, harness):
    """one write per input (each its own first member), then all inputs back to back in one write and in one write shifted by a
    prefix, so that every input also lies at other member indices and offsets within a member"""
    from sailfish_amd import _lib
    P = harness.P
    cases = _all_inputs(P)
    names = list(cases)
    rcs, rc_close, res, chunks = _collect([_dev(cases[k], gpu) for k in names])
    assert all(r == _lib.OK for r in rcs) and rc_close == _lib.OK
    got = b"".join(chunks)
    data = b"".join(cases[k] for k in names)
    want, st = harness.encode(data, [len(cases[k]) for k in names])
    assert got == want
    check_file(got, data, P, [len(cases[k]) for k in names])
    assert (res["n_members"], res["n_stored_members"], res["n_matches"], res["n_literals"]) == (st["members"], st["stored"], st["matches"], st["literals"])
    assert res["n_bytes_in"] == len(data) and res["n_bytes_out"] == len(got) and res["n_chunks"] == len(chunks)
    for prefix in (b"", b"x" * 12345):
        rcs, rc_close, res, chunks = _collect([_dev(prefix + data, gpu)])
        assert rcs == [_lib.OK] and rc_close == _lib.OK
        assert b"".join(chunks) == harness.encode(prefix + data)[0]


def test_alignment_writes_and_chunks(built, gpu, harness):
    """the corpus text (about 4 MB) in one write: d_src at byte offsets 0 .. 3, the same bytes twice, two writes, forced chunks"""
    from sailfish_amd import _lib
    P = harness.P
    data = bamwrite_corpus.stream(True, "sam")
    want, st = harness.encode(data)
    check_file(want, data, P)
    files = []
    for shift in (0, 1, 2, 3, 0):
        rcs, rc_close, res, chunks = _collect([_dev(data, gpu, shift)])
        assert rcs == [_lib.OK] and rc_close == _lib.OK
        files.append(b"".join(chunks))
        assert res["n_members"] == st["members"] and res["n_stored_members"] == 0 and res["n_matches"] == st["matches"]
    assert all(f == want for f in files)
    print(f"{len(data)} B -> {len(want)} B, encode {res['encode_ms']:.3f} ms, copies {res['d2h_ms']:.3f} ms, sink {res['sink_ms']:.3f} ms")
    cut = 1_000_001
    d = _dev(data, gpu)
    rcs, rc_close, res, chunks = _collect([d[:cut], d[:0], d[cut:]])
    assert all(r == _lib.OK for r in rcs) and rc_close == _lib.OK
    split = b"".join(chunks)
    assert split == harness.encode(data, [cut])[0] and split != want
    check_file(split, data, P, [cut])
    small = data[:70_000]
    for chunk in (16, 20_000, 0):
        rcs, rc_close, res, chunks = _collect([_dev(small, gpu)], chunk_bytes=chunk)
        assert rcs == [_lib.OK] and rc_close == _lib.OK and res["n_chunks"] == len(chunks)
        assert max(len(c) for c in chunks) <= max(chunk or 1 << 25, 28)
        assert b"".join(chunks) == harness.encode(small)[0]
        assert chunk != 16 or len(chunks) > 100


def test_open_close_and_refusal(built, gpu):
    from sailfish_amd import _lib
    for tensors in ([], [torch.zeros(0, dtype=torch.uint8, device=gpu)]):
        rcs, rc_close, res, chunks = _collect(tensors)
        assert all(r == _lib.OK for r in rcs) and rc_close == _lib.OK and b"".join(chunks) == EOF
        assert res["n_members"] == 0 and res["n_bytes_out"] == 28
    t = _dev(bamwrite_corpus.stream(True, "sam")[:500_000], gpu)
    rcs, rc_close, res, chunks = _collect([t, t], chunk_bytes=4096, refuse_at=2)
    assert rcs == [_lib.ERR_IO, _lib.ERR_STATE] and rc_close == _lib.OK
    assert len(chunks) == 2 and chunks[1] is None and res["n_chunks"] == 2


def test_device_reads_what_the_device_wrote(built, gpu, harness):
    """sfgpu_bgzf_inflate_host on the device-written file returns the payload; BgzfDeviceWriter writes the same file"""
    from sailfish_amd import _lib, gzfile
    data = bamwrite_corpus.stream(False, "bam") + inputs(harness.P)["random"]
    out = io.BytesIO()
    with gzfile.BgzfDeviceWriter(out) as w:
        assert w.write(_dev(data, gpu)) == len(data)
    file = out.getvalue()
    assert file == harness.encode(data)[0]
    assert w.stats["n_bytes_in"] == len(data) and w.stats["n_bytes_out"] == len(file)
    assert w.stats["n_stored_members"] == harness.encode(data)[1]["stored"] >= 2
    with pytest.raises(ValueError):
        w.write(_dev(data, gpu))
    src = torch.from_numpy(np.frombuffer(file, np.uint8).copy())
    dst = torch.zeros(len(data) + 64, dtype=torch.uint8, device=gpu)
    res = _lib.BgzfResult()
    rc = _lib.lib().sfgpu_bgzf_inflate_host(_lib.ptr(src), src.numel(), 1, _lib.ptr(dst), len(data), C.byref(res), _lib.current_stream_ptr())
    assert rc == _lib.OK and int(res.n_bytes_out) == len(data) and int(res.consumed) >= len(file) - 28
    assert dst[:len(data)].cpu().numpy().tobytes() == data


def test_a_write_of_more_than_one_batch(built, gpu):
    """one write slightly over 64 MiB: 2048 members are a batch, so the handle encodes a second batch into its other output buffer
    while the first is copied, reuses the slots and sums the statistics.  gzip inflates the file to the bytes written and the BSIZE
    walk finds every member whole."""
    import gzip

    from sailfish_amd import _lib
    from test_bgzw_cpu import members
    text = bamwrite_corpus.stream(True, "sam")
    n = (64 << 20) + 100_003
    data = (text * (n // len(text) + 1))[:n]
    rcs, rc_close, res, chunks = _collect([_dev(data, gpu, shift=1)])
    assert rcs == [_lib.OK] and rc_close == _lib.OK
    file = b"".join(chunks)
    assert gzip.decompress(file) == data
    ms = members(file)
    assert len(ms) - 1 == res["n_members"] == -(-n // 32768) > 2048 and res["n_bytes_in"] == n and res["n_bytes_out"] == len(file)
    assert all(len(payload) == 32768 for _, payload in ms[:-2]) and len(ms[-2][1]) == n % 32768


def test_gzip_and_bgzf_handles_interleaved(built, gpu, harness, tmp_path):
    """a gzip handle and a BGZF handle open at once, their writes alternating: both run through the one driver (slotpipe.h), and
    neither sees the other's buffers, counters or chunk size.  Two writes of 200 000 bytes each (four 64 KB gzip blocks, seven
    BGZF members with a short last one), the second from a source one byte off alignment; one handle with 4096-byte chunks, which
    end inside blocks, the other with the default; both ways round.  Each file is its serial encoder's, cut for cut."""
    import test_gzwrite_cpu as G
    from sailfish_amd import _lib
    L = _lib.lib()
    n = 200_000
    data = bamwrite_corpus.stream(True, "sam")[:2 * n]
    srcs = [_dev(data[:n], gpu), _dev(data[n:], gpu, shift=1)]
    gz_exe = G.build_harness(tmp_path)
    want = {"gz": G.host_encode(gz_exe, tmp_path, data, writes=(n,))[0], "bgzw": harness.encode(data, (n,))[0]}
    for chunk in ({"gz": 4096, "bgzw": 0}, {"gz": 0, "bgzw": 4096}):
        chunks = {"gz": [], "bgzw": []}
        sinks = {k: _lib.TEXT_SINK(lambda addr, m, _user, k=k: chunks[k].append(bytes((C.c_char * m).from_address(addr))) or 0) for k in chunks}
        hs = {"gz": C.c_void_p(), "bgzw": C.c_void_p()}
        assert L.sfgpu_gz_open(C.byref(hs["gz"]), sinks["gz"], None, chunk["gz"]) == _lib.OK
        assert L.sfgpu_bgzw_open(C.byref(hs["bgzw"]), sinks["bgzw"], None, chunk["bgzw"]) == _lib.OK
        for t in srcs:
            assert L.sfgpu_gz_write_device(hs["gz"], _lib.ptr(t), t.numel(), _lib.current_stream_ptr()) == _lib.OK
            assert L.sfgpu_bgzw_write_device(hs["bgzw"], _lib.ptr(t), t.numel(), _lib.current_stream_ptr()) == _lib.OK
        res = {"gz": _lib.GzResult(), "bgzw": _lib.BgzwResult()}
        assert L.sfgpu_gz_close(hs["gz"], C.byref(res["gz"])) == _lib.OK
        assert L.sfgpu_bgzw_close(hs["bgzw"], C.byref(res["bgzw"])) == _lib.OK
        for k in chunks:
            got, r = b"".join(chunks[k]), res[k].as_dict()
            assert got == want[k], k
            assert (r["n_bytes_in"], r["n_bytes_out"], r["n_chunks"]) == (2 * n, len(want[k]), len(chunks[k])), k
            assert max(len(c) for c in chunks[k]) <= (chunk[k] or 1 << 25)
            assert (len(chunks[k]) > 10) == (chunk[k] == 4096)
        assert res["gz"].as_dict()["n_blocks"] == 8 and res["bgzw"].as_dict()["n_members"] == 14
