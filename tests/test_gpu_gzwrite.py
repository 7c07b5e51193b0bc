"""The device gzip writer (sfgpu_gz_open / sfgpu_gz_write_device / sfgpu_gz_close, sailfish_amd/csrc/gzwrite.hip) on the GPU:
every file inflates to the exact bytes of the device buffer, the device stream equals the serial host encoder's stream byte for
byte (tests/gzwrite_harness.cpp over the same gzfmt.h, which tests/test_gzwrite_cpu.py holds against zlib), quantify writes
bootstraps.gz through it as one gzip member with the payload of the host path, and the files are no larger than 1.10 x zlib
level 6."""
import ctypes as C
import gzip
import io
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gzwrite_cpu import BLOCK, FRAME, STORED_OVERHEAD, build_harness, check_stream, host_encode, level6

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("gzh"))


def _dev(data, gpu):
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(gpu) if len(data) else torch.zeros(0, dtype=torch.uint8, device=gpu)


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
    assert L.sfgpu_gz_open(C.byref(h), cb, None, chunk_bytes) == _lib.OK
    rcs = [L.sfgpu_gz_write_device(h, _lib.ptr(t), t.numel() * t.element_size(), _lib.current_stream_ptr()) for t in tensors]
    res = _lib.GzResult()
    rc_close = L.sfgpu_gz_close(h, C.byref(res))
    return rcs, rc_close, res.as_dict(), chunks


def _cases():
    rng = np.random.default_rng(17)
    cases = {"one": b"\x07", "zeros": bytes(3 * BLOCK + 17), "block": bytes(BLOCK), "block+1": b"\1" * (BLOCK + 1),
             "ramp": bytes(range(256)) * 300, "random": rng.integers(0, 256, 2 * BLOCK + 5, dtype=np.uint8).tobytes(),
             "doubles": rng.random(30_000).tobytes()}
    for r in (2, 3, 258, 259, 260):
        cases[f"run{r}"] = b"a" + b"b" * r + b"c" + b"d" * (r + 1) + b"e" + b"\0" * r
    edge = bytearray(b"\5" * (4 * BLOCK + 300))
    for b in (1, 2, 3, 4):
        for d in (-259, -3, -2, -1, 1, 2, 3, 258):
            edge[b * BLOCK + d] = 9
    cases["edges"] = bytes(edge)
    for n in (BLOCK - 1, BLOCK + 2, 2 * BLOCK + 258):
        cases[f"sparse{n}"] = (rng.integers(0, 9, n) * (rng.random(n) < 0.2)).astype(np.uint8).tobytes()
    counts = (rng.poisson(3.0, 700_000) * (rng.random(700_000) < 0.4)).astype(np.int32)
    cases["counts"] = counts.tobytes()
    return cases


def test_round_trip_and_host_stream(built, gpu, harness, tmp_path):
    """C entry with a collecting sink: inflates to the buffer, trailer = CRC-32 / ISIZE, and the stream is the host encoder's"""
    from sailfish_amd import _lib
    for name, data in _cases().items():
        rcs, rc_close, res, chunks = _collect([_dev(data, gpu)])
        assert rcs == [_lib.OK] and rc_close == _lib.OK, name
        gz = b"".join(chunks)
        check_stream(gz, data)
        want, st = host_encode(harness, tmp_path, data)
        assert gz == want, name
        assert res["n_bytes_in"] == len(data) and res["n_bytes_out"] == len(gz) and res["n_chunks"] == len(chunks)
        assert res["n_blocks"] == st["blocks"] and res["n_stored_blocks"] == st["stored"], name
        if name in ("random", "doubles"):                  # incompressible input does not grow beyond the stated overhead
            assert len(gz) <= len(data) + STORED_OVERHEAD * res["n_blocks"] + FRAME
        if name == "random":
            assert res["n_stored_blocks"] == res["n_blocks"]


def test_empty_stream_and_empty_write(built, gpu):
    from sailfish_amd import _lib
    for tensors in ([], [_dev(b"", gpu)]):
        rcs, rc_close, res, chunks = _collect(tensors)
        assert all(r == _lib.OK for r in rcs) and rc_close == _lib.OK and len(chunks) == 2
        check_stream(b"".join(chunks), b"")
        assert res["n_bytes_in"] == 0 and res["n_blocks"] == 0


def test_chunks_and_several_writes(built, gpu, harness, tmp_path):
    """a forced small chunk (chunk ends inside blocks), a buffer larger than one staging chunk and than one batch of blocks,
    several writes per stream, unaligned sources: one member, the host encoder's bytes for the same writes"""
    from sailfish_amd import _lib
    rng = np.random.default_rng(18)
    data = (rng.integers(0, 40, 1_500_000) * (rng.random(1_500_000) < 0.3)).astype(np.uint8).tobytes()
    d = _dev(data, gpu)
    want, _ = host_encode(harness, tmp_path, data)
    for chunk in (16, 1000, 4099, 1 << 16):
        if chunk == 16:
            small = data[:70_000]
            rcs, rc_close, res, chunks = _collect([_dev(small, gpu)], chunk_bytes=16)
            gz = b"".join(chunks)
            check_stream(gz, small)
            assert max(len(c) for c in chunks) <= 16
            continue
        rcs, rc_close, res, chunks = _collect([d], chunk_bytes=chunk)
        assert rcs == [_lib.OK] and rc_close == _lib.OK
        assert max(len(c) for c in chunks) <= max(chunk, 13) and res["n_chunks"] == len(chunks) > 3
        assert b"".join(chunks) == want
    sizes = (1, 65535, 0, 65537, 100_000, 7)
    cuts = np.concatenate([[0], np.cumsum(sizes), [len(data)]])
    parts = [d[int(a):int(b)] for a, b in zip(cuts[:-1], cuts[1:])]                 # odd offsets: unaligned device pointers
    rcs, rc_close, res, chunks = _collect(parts)
    assert all(r == _lib.OK for r in rcs) and rc_close == _lib.OK
    gz = b"".join(chunks)
    check_stream(gz, data)
    want_parts, _ = host_encode(harness, tmp_path, data, writes=sizes)
    assert gz == want_parts
    # more than one batch of 1024 blocks and more than one 32 MiB staging chunk: 100 MB of doubles that do not compress, then zeros
    big = torch.rand(12_500_000, dtype=torch.float64, device=gpu)
    rcs, rc_close, res, chunks = _collect([big, torch.zeros(5_000_000, dtype=torch.int32, device=gpu)])
    assert all(r == _lib.OK for r in rcs) and rc_close == _lib.OK and res["n_chunks"] > 5
    payload = big.cpu().numpy().tobytes() + bytes(20_000_000)
    check_stream(b"".join(chunks), payload)
    assert res["n_bytes_out"] <= 100_000_000 + STORED_OVERHEAD * 1526 + FRAME + 100_000


def test_sink_refusal(built, gpu):
    """a sink that refuses the second chunk: ERR_IO, no further sink call, later writes are ERR_STATE, the handle closes cleanly;
    an exception of the file object's write comes out of GzDeviceWriter.write and the library works afterwards"""
    from sailfish_amd import _lib, gzfile
    rng = np.random.default_rng(19)
    t = torch.from_numpy(rng.integers(0, 5, 3_000_000).astype(np.int32)).to(gpu)
    rcs, rc_close, res, chunks = _collect([t, t], chunk_bytes=4096, refuse_at=2)
    assert rcs == [_lib.ERR_IO, _lib.ERR_STATE] and rc_close == _lib.OK
    assert len(chunks) == 2 and chunks[1] is None and res["n_chunks"] == 2

    class Failing(io.RawIOBase):
        calls = 0

        def writable(self):
            return True

        def write(self, b):
            self.calls += 1
            if self.calls == 3:
                raise OSError("disk full")
            return len(b)
    f = Failing()
    w = gzfile.GzDeviceWriter(f, chunk_bytes=4096)
    with pytest.raises(OSError, match="disk full"):
        w.write(t)
    w.close()
    assert f.calls == 3
    out = io.BytesIO()
    with gzfile.GzDeviceWriter(out) as w2:
        w2.write(t)
    check_stream(out.getvalue(), t.cpu().numpy().tobytes())


def test_python_writers(built, gpu, tmp_path):
    """GzDeviceWriter (path and file object, any dtype) and BootstrapWriter.write_device; mixing the two ways raises"""
    import sailfish_amd as sf
    from sailfish_amd import gzfile
    rng = np.random.default_rng(20)
    a = torch.from_numpy(rng.poisson(2.0, (7, 5001)).astype(np.int32)).to(gpu)
    b = torch.from_numpy(np.round(rng.gamma(0.3, 50.0, (3, 5001)) * (rng.random((3, 5001)) < 0.5), 2)).to(gpu)
    p = tmp_path / "x.gz"
    with gzfile.GzDeviceWriter(str(p)) as w:
        w.write(a); w.write(b); w.write(a[2:5])
    payload = a.cpu().numpy().tobytes() + b.cpu().numpy().tobytes() + a[2:5].cpu().numpy().tobytes()
    check_stream(p.read_bytes(), payload)
    assert w.result["n_bytes_in"] == len(payload)
    assert subprocess.run(["gzip", "-t", str(p)]).returncode == 0
    with pytest.raises(ValueError):
        w.write(a)
    with pytest.raises(TypeError):
        gzfile.GzDeviceWriter(io.BytesIO()).write(a.cpu())
    with pytest.raises(ValueError):
        gzfile.GzDeviceWriter(io.BytesIO()).write(a.t())
    sopt = sf.SailfishOpts()
    bw = sf.writer.BootstrapWriter(str(tmp_path / "o1"), sopt)
    bw.write_device(b); bw.write_device(b[:1])
    with pytest.raises(RuntimeError):
        bw(b[0].cpu().numpy())
    bw.close()
    assert bw.written == 4
    got = (tmp_path / "o1" / "aux" / "bootstrap" / "bootstraps.gz").read_bytes()
    check_stream(got, b.cpu().numpy().tobytes() + b[:1].cpu().numpy().tobytes())
    old = sf.writer.BootstrapWriter(str(tmp_path / "o2"), sopt)
    old(b[0].cpu().numpy())
    with pytest.raises(RuntimeError):
        old.write_device(b)
    old.close()


def _members(gz):
    """walks the file with zlib: (payload, number of gzip members)"""
    out, n = b"", 0
    while gz:
        d = zlib.decompressobj(31)
        out += d.decompress(gz) + d.flush()
        assert d.eof
        gz, n = d.unused_data, n + 1
    return out, n


@pytest.mark.parametrize("kind", ["gibbs", "bootstrap"])
def test_quantify_writes_one_member(built, gpu, tmp_path, kind):
    """quantify with numGibbsSamples / numBootstraps on test_quant's kind of fixture: bootstraps.gz is one gzip member of n x M
    elements, equal to what the host path (BootstrapWriter.__call__ as the samplers' callback) writes for the same seed"""
    import sailfish_amd as sf
    from test_filter import _txome
    from test_gpu_eqfile import _hit_batches
    rng = np.random.default_rng(21)
    M, R, n = 300, 60_000, 6
    seq, so, rl = _txome(rng, M, lo=400, hi=3000)
    names = [f"tx{i:04d}" for i in range(M)]
    batches = _hit_batches(rng, rl, R, True)
    kw = dict(numGibbsSamples=n) if kind == "gibbs" else dict(numBootstraps=n)
    sopt = sf.SailfishOpts(numFragSamples=2000, **kw)
    out = str(tmp_path / "out")
    rc, exp = sf.quant.quantify(names, rl, batches, "IU", out, sopt, allow_orphans=True, seed=11, device=gpu)
    assert rc == 0
    p = os.path.join(out, "aux", "bootstrap", "bootstraps.gz")
    gz = open(p, "rb").read()
    d = zlib.decompressobj(31)
    payload = d.decompress(gz) + d.flush()
    assert d.eof and d.unused_data == b""
    assert _members(gz) == (payload, 1)
    assert gzip.open(p).read() == payload and subprocess.run(["gzip", "-t", p]).returncode == 0
    dt = np.int32 if kind == "gibbs" else np.float64
    got = np.frombuffer(payload, dt)
    assert got.size == n * M
    crc, isize = struct.unpack("<II", gz[-8:])
    assert crc == zlib.crc32(payload) and isize == len(payload)
    # the host path on the same experiment and seed
    w = sf.writer.BootstrapWriter(str(tmp_path / "old"), sopt)
    if kind == "gibbs":
        assert sf.CollapsedGibbsSampler().sample(exp, sopt, w, n, seed=11)
    else:
        assert sf.CollapsedEMOptimizer().gatherBootstraps(exp, sopt, w, 0.01, 10000, seed=11)
    w.close()
    old = gzip.open(os.path.join(str(tmp_path / "old"), "aux", "bootstrap", "bootstraps.gz")).read()
    diff = np.max(np.abs(np.frombuffer(old, dt).astype(np.float64) - got.astype(np.float64))) if len(old) == len(payload) else None
    print(f"{kind}: {len(payload)} payload bytes, {len(gz)} file bytes, max |device path - host path| = {diff}")
    assert old == payload
    assert got.reshape(n, M).sum(1).min() > 0


@pytest.fixture(scope="module")
def samples(built, gpu):
    """the suite's 5 000-transcript fixture (test_gpu_parity.midsize): Gibbs draws, plain-EM and VBEM bootstrap replicates and
    an abundance vector with 90 % zeros, as device tensors"""
    import sailfish_amd as sf
    from sailfish_amd import synth
    ref_len, ids, off = synth.workload(5000, 20000, 400_000)
    ob = O.EqBuilder()
    ob.add_batch(ids.numpy().view(np.uint32), off.numpy().view(np.uint32).astype(np.uint64))
    rp, ii, cc, _ = ob.finish()
    eff = O.efflen_smoothed(ref_len.numpy().view(np.uint32), O.cf_gaussian())
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(gpu)
    dev = (torch.from_numpy(eff).to(gpu), t(rp.astype(np.uint32), np.int32), t(ii.astype(np.uint32), np.int32), t(cc.astype(np.uint64), np.int64))
    p = sf.EMProblem(*dev, 400_000)
    rc, _ = p.optimize()
    assert rc == 0
    alpha = p.alpha.clone()
    rc, gs = sf.gibbs_sample(dev[0], p.mass, dev[1], dev[2], dev[3], 400_000, 16, seed=5)
    assert rc == 0
    rc, bs, _ = p.bootstrap(4, seed=5, use_vbem=False)
    assert rc == 0
    rc, vb, _ = p.bootstrap(4, seed=5, use_vbem=True)
    assert rc == 0
    sparse = alpha.clone()
    sparse[torch.from_numpy(np.random.default_rng(22).random(5000) < 0.9).to(gpu)] = 0.0
    return dict(gibbs=gs, bootstrap_em=bs, alpha_90pct_zero=sparse, bootstrap_vbem=vb)


def test_size_against_zlib_level_6(samples, gpu):
    """Measured on the MI355X (ratio = device file / zlib level 6 of the same bytes); see DESIGN 4.12 for the recorded figures.
    VBEM bootstrap replicates are measured and recorded, not capped (the issue: a 32 KB-window matcher finds the repeated doubles
    that the run-match class cannot)."""
    from sailfish_amd import gzfile
    ratios = {}
    for name, t in samples.items():
        out = io.BytesIO()
        with gzfile.GzDeviceWriter(out) as w:
            w.write(t)
        raw = t.cpu().numpy().tobytes()
        check_stream(out.getvalue(), raw)
        ratios[name] = len(out.getvalue()) / level6(raw)
        print(f"{name}: {len(raw)} B -> {len(out.getvalue())} B, {ratios[name]:.3f} x level 6, distinct values {len(np.unique(t.cpu().numpy()))}, "
              f"{w.result['n_stored_blocks']} of {w.result['n_blocks']} blocks stored, encode {w.result['encode_ms']:.3f} ms")
    for name in ("gibbs", "bootstrap_em", "alpha_90pct_zero"):
        assert ratios[name] <= 1.10, ratios


def test_cpp_adaptor_write_bootstraps(built, gpu, tmp_path):
    """writeBootstraps in include/sfgpu_sailfish.hpp, compiled with g++ and run: the file inflates to the matrix the program
    uploaded; a path that cannot be opened is refused with an exception"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "gzwrite_host_test"
    csrc = os.path.join(root, "sailfish_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(root, "include"),
                           "-I", "/opt/rocm/include", os.path.join(root, "tests", "gzwrite_host_test.cpp"), "-o", str(exe),
                           "-L", csrc, "-lsfgpu", "-L", "/opt/rocm/lib", "-lamdhip64", "-pthread",
                           "-Wl,-rpath," + csrc + ",-rpath,/opt/rocm/lib"])
    r = subprocess.run([str(exe), str(tmp_path / "b.gz"), str(tmp_path / "b.raw"), str(tmp_path / "no_such_dir" / "b.gz")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "wrote 9 samples" in r.stdout and "refused:" in r.stdout, r.stdout + r.stderr
    raw = (tmp_path / "b.raw").read_bytes()
    assert len(raw) == 9 * 12345 * 4
    check_stream((tmp_path / "b.gz").read_bytes(), raw)
