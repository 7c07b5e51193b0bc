"""quant.sf written from the device (sfgpu_quant_write_text, sailfish_amd/csrc/quant_write.hip with the %g of csrc/gfmt.h;
quantfile.write_rows / write_file / text_size; writer.write_abundances; writeAbundances in include/sfgpu_sailfish.hpp).  The
expected bytes are always quantfile.format_rows' -- the per-row loop over Python's "%g" -- on the host copy of the same arrays."""
import ctypes as C
import io
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(cols, gpu):
    """(names, length, eff, tpm, num_reads) on the host -> the arguments of quantfile.write_rows"""
    names, length, eff, tpm, nr = cols
    return (list(names), torch.from_numpy(np.asarray(length, np.uint32).view(np.int32).copy()).to(gpu),
            torch.from_numpy(np.asarray(eff, np.float64).copy()).to(gpu), torch.from_numpy(np.asarray(tpm, np.float64).copy()).to(gpu),
            torch.from_numpy(np.asarray(nr, np.float64).copy()).to(gpu))


def _want(cols):
    from sailfish_amd import quantfile
    return quantfile.format_rows(*cols)


def _blob(names, gpu):
    from sailfish_amd import quantfile
    b, o = quantfile.names_blob(names)
    return (torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(gpu), torch.from_numpy(o.view(np.int64).copy()).to(gpu))


def _collect(dev_cols, chunk_bytes=0, refuse_at=None, null_sink=False):
    """the C entry with a sink that keeps every chunk; returns (status, result dict, chunks).  dev_cols[0] is a (blob, offsets)
    pair of device tensors"""
    from sailfish_amd import _lib
    (blob, off), length, eff, tpm, nr = dev_cols
    chunks = []

    def sink(addr, n, _user):
        chunks.append(C.string_at(addr, n))
        return 1 if refuse_at is not None and len(chunks) == refuse_at else 0

    res = _lib.QuantWriteResult()
    with torch.cuda.device(eff.device):
        rc = _lib.lib().sfgpu_quant_write_text(_lib.ptr(blob) if blob.numel() else None, _lib.ptr(off), _lib.ptr(length), _lib.ptr(eff),
                                               _lib.ptr(tpm), _lib.ptr(nr), eff.numel(), chunk_bytes,
                                               _lib.TEXT_SINK(0) if null_sink else _lib.TEXT_SINK(sink), None, C.byref(res),
                                               _lib.current_stream_ptr())
    return rc, res.as_dict(), chunks


def _written(cols, gpu, chunk_bytes=0):
    from sailfish_amd import quantfile
    f = io.BytesIO()
    res = quantfile.write_rows(f, *_dev(cols, gpu), chunk_bytes=chunk_bytes)
    return f.getvalue(), res


def _row_lengths(text):
    return np.diff(np.concatenate([[0], np.flatnonzero(np.frombuffer(text, np.uint8) == ord("\n")) + 1]))


def _greedy_chunks(row_len, chunk_bytes):
    n, cur = 0, 0
    for L in row_len:
        if cur and cur + L > chunk_bytes:
            n, cur = n + 1, 0
        cur += int(L)
    return n + (1 if cur else 0)


def _first_difference(got, want):
    n = min(len(got), len(want))
    a, b = np.frombuffer(got, np.uint8, n), np.frombuffer(want, np.uint8, n)
    d = np.flatnonzero(a != b)
    i = int(d[0]) if len(d) else n
    lo = want.rfind(b"\n", 0, i) + 1
    return f"lengths {len(got)} / {len(want)}, first difference at byte {i}: got {got[lo:i + 40]!r}, want {want[lo:i + 40]!r}"


def _check_equal(cols, gpu, chunk_bytes=0, names_have_newlines=False):
    want = _want(cols)
    got, res = _written(cols, gpu, chunk_bytes)
    assert got == want, _first_difference(got, want)
    assert res["n_bytes"] == len(want) and res["n_rows"] == len(cols[0])
    if len(want) and not names_have_newlines:
        row_len = _row_lengths(want)
        assert res["max_row_bytes"] == int(row_len.max())
        assert res["n_chunks"] == _greedy_chunks(row_len, chunk_bytes or (32 << 20))
    return res


def _ties():
    """every sampled exactly representable (d + 1/2) 10^j with both neighbours, j in -12 .. 16"""
    rng = np.random.default_rng(41)
    out = []
    for j in range(-12, 17):
        for d in rng.integers(100000, 1000000, 3000):
            v = Fraction(2 * int(d) + 1, 2) * Fraction(10) ** j
            f = float(v)
            if Fraction(f) == v:
                out.append(f)
            out += [math.nextafter(f, 0.0), math.nextafter(f, math.inf)]
    return out


def _edges():
    out = []
    for k in range(-320, 309):
        p = float(f"1e{k}")
        out += [p, math.nextafter(p, 0.0)]
        if k < 308:
            out.append(float(f"9.999995e{k}"))
    out += [0.0001, 9.9999949999e-05, 9.9999995e-05, 99999.95, 999999.5, 999999.4999999999, 1e5, 1e6, 0.0, -0.0, 5e-324,
            2.2250738585072014e-308, 1.7976931348623157e308, math.inf, -math.inf, math.nan, 1e22, 1e23, 1.0, 0.5, 123456.5]
    return out + [-x for x in out]


@pytest.mark.gpu
def test_formatter_alone(built, gpu):
    """rows with empty names and Length 0: the three double columns hold 3 M random bit patterns, the tie set and the edge
    list; every byte equals Python's "%g", and the slow path ran"""
    rng = np.random.default_rng(40)
    special = np.array(_ties() + _edges(), np.float64)
    n_rand = 3_000_000
    cells = np.concatenate([rng.integers(0, 2 ** 64, n_rand, dtype=np.uint64).view(np.float64), special])
    cells = np.concatenate([cells, np.zeros((-len(cells)) % 3)])
    n = len(cells) // 3
    cols = ([b""] * n, np.zeros(n, np.uint32), cells[:n], cells[n:2 * n], cells[2 * n:])
    res = _check_equal(cols, gpu)
    assert res["n_slow"] > 1_000_000 and res["max_row_bytes"] <= 5 + 1 + 3 * 13


def _cfg3_like(rng, n):
    length = rng.integers(200, 100_000, n).astype(np.uint32)
    eff = np.maximum(length.astype(np.float64) - rng.random(n) * 180.0, 1.0)
    cnt = np.where(rng.random(n) < 0.3, 0.0, 10.0 ** rng.uniform(-6, 5, n))
    rate = cnt / eff
    tpm = rate / rate.sum() * 1e6 if rate.sum() > 0 else np.zeros(n)
    if n >= 1000:                                                 # (a handful of rows may hold no zero, or nothing else)
        assert tpm[tpm > 0].min() >= 1e-13 and (cnt == 0).mean() > 0.25
    return length, eff, tpm, cnt


@pytest.mark.gpu
def test_random_table(built, gpu):
    """5 000 rows with realistic names"""
    rng = np.random.default_rng(42)
    n = 5000
    names = [f"ENST{rng.integers(0, 10 ** 11):011d}.{rng.integers(1, 20)}|ENSG{rng.integers(0, 10 ** 11):011d}" if i % 3 else f"tx{i}"
             for i in range(n)]
    res = _check_equal((names,) + _cfg3_like(rng, n), gpu)
    assert res["n_slow"] == 0
    _check_equal((names,) + _cfg3_like(rng, n), gpu, chunk_bytes=5000)


@pytest.mark.gpu
def test_cfg3_sized_table(built, gpu):
    """200 000 rows with cfg3-like columns (30 % exact zeros, nonzero TPM >= 1e-13) at the default chunk size and at 1 MiB"""
    rng = np.random.default_rng(43)
    n = 200_000
    names = [f"ENST{i:011d}.{1 + i % 9}" for i in range(n)]
    cols = (names,) + _cfg3_like(rng, n)
    res = _check_equal(cols, gpu)
    assert res["n_slow"] == 0 and res["n_chunks"] == 1
    res = _check_equal(cols, gpu, chunk_bytes=1 << 20)
    assert res["n_slow"] == 0 and res["n_chunks"] > 4


@pytest.mark.gpu
def test_names(built, gpu):
    """empty, 1 byte, 4 095 / 4 096 / 4 097 / 10 000 bytes, non-ASCII UTF-8; a long name first, last and alone"""
    rng = np.random.default_rng(44)

    def long_name(k):
        return bytes(rng.integers(33, 127, k, dtype=np.uint8))

    special = [b"", b"x", long_name(4095), long_name(4096), long_name(4097), long_name(10_000), "трансκρίπτ-転写".encode(), b"a b|c;d",
               long_name(48), long_name(49), long_name(47), b"", long_name(200)]
    names = []
    for i in range(600):
        names.append(special[(i // 7) % len(special)] if i % 7 == 0 else f"t{i}".encode())
    cols = (names,) + _cfg3_like(rng, len(names))
    res = _check_equal(cols, gpu)
    assert res["max_row_bytes"] > 10_000
    _check_equal(cols, gpu, chunk_bytes=10_100)
    for order in ([long_name(10_000), b"a", b"b"], [b"a", b"b", long_name(10_000)], [long_name(10_000)], [long_name(4096)], [b""],
                  [long_name(30_000), long_name(4097), long_name(5000)]):
        _check_equal((order,) + _cfg3_like(rng, len(order)), gpu)
    # all names empty: the blob is empty
    _check_equal(([b""] * 50,) + _cfg3_like(rng, 50), gpu)
    # name bytes are never inspected: tabs, newlines and NULs pass through
    odd = [b"a\tb", b"c\nd", b"\x00\x01", b"\xff\xfe"]
    _check_equal((odd,) + _cfg3_like(rng, 4), gpu, names_have_newlines=True)


@pytest.mark.gpu
def test_empty_table(built, gpu):
    from sailfish_amd import _lib
    e = np.zeros(0)
    dev = _dev(([], np.zeros(0, np.uint32), e, e, e), gpu)
    rc, res, chunks = _collect((_blob([], gpu),) + dev[1:])
    assert rc == _lib.OK and chunks == [] and res["n_bytes"] == 0 and res["n_chunks"] == 0 and res["n_rows"] == 0
    got, res = _written(([], np.zeros(0, np.uint32), e, e, e), gpu)
    assert got == b"" and res["n_bytes"] == 0


@pytest.mark.gpu
def test_chunk_edges(built, gpu):
    """every chunk size from the longest row up to a few hundred bytes: whole rows, greedy, in order; one byte less is refused
    before the sink is called; sizes outside [16, 2^30] are invalid arguments"""
    from sailfish_amd import _lib
    rng = np.random.default_rng(45)
    n = 400
    names = [f"tx{i}" * int(rng.integers(1, 4)) for i in range(n)]
    cols = (names,) + _cfg3_like(rng, n)
    want = _want(cols)
    row_len = _row_lengths(want)
    max_row = int(row_len.max())
    assert max_row >= 18
    d = _dev(cols, gpu)
    dev = (_blob(names, gpu),) + d[1:]
    for chunk in list(range(max_row, 321)) + [4095, 4096, 4097, len(want) - 1, len(want), len(want) + 1]:
        rc, res, chunks = _collect(dev, chunk)
        assert rc == _lib.OK, chunk
        assert b"".join(chunks) == want, chunk
        assert all(c.endswith(b"\n") and 0 < len(c) <= chunk for c in chunks), chunk
        assert res["n_chunks"] == len(chunks) == _greedy_chunks(row_len, chunk), chunk
        assert res["max_row_bytes"] == max_row and res["n_bytes"] == len(want)
    rc, res, chunks = _collect(dev, max_row - 1)
    assert max_row - 1 >= 16 and rc == _lib.ERR_RANGE and chunks == [] and res["n_chunks"] == 0
    assert res["max_row_bytes"] == max_row                        # the sizes are known when the call refuses
    for bad in (15, 2 ** 30 + 1):
        rc, res, chunks = _collect(dev, bad)
        assert rc == _lib.ERR_INVALID and chunks == []
    rc, _, chunks = _collect(dev, 2 ** 30)
    assert rc == _lib.OK and b"".join(chunks) == want


class _Refusing(io.RawIOBase):
    def __init__(self, fail_at):
        self.calls, self.fail_at = 0, fail_at

    def writable(self):
        return True

    def write(self, b):
        self.calls += 1
        if self.calls == self.fail_at:
            raise OSError(28, "No space left on device (test)")
        return len(b)


@pytest.mark.gpu
def test_sink_refusal(built, gpu):
    """a sink that returns 1 on its second call ends the call with ERR_IO after exactly two calls; an exception of the file
    object's write comes out of write_rows and the library works afterwards"""
    from sailfish_amd import _lib, quantfile
    rng = np.random.default_rng(46)
    n = 2000
    names = [f"tx{i}" for i in range(n)]
    cols = (names,) + _cfg3_like(rng, n)
    want = _want(cols)
    d = _dev(cols, gpu)
    dev = (_blob(names, gpu),) + d[1:]
    rc, res, chunks = _collect(dev, 1024, refuse_at=2)
    assert rc == _lib.ERR_IO and len(chunks) == 2 and res["n_chunks"] == 2
    assert b"".join(chunks) == want[:len(chunks[0]) + len(chunks[1])]
    assert b"sink" in _lib.lib().sfgpu_last_error()
    f = _Refusing(fail_at=3)
    with pytest.raises(OSError, match="No space left on device"):
        quantfile.write_rows(f, *d, chunk_bytes=1024)
    assert f.calls == 3
    rc, _, chunks = _collect(dev, 1024)
    assert rc == _lib.OK and b"".join(chunks) == want


@pytest.mark.gpu
def test_sizing_only(built, gpu):
    """sink = NULL: the sizes equal the host's, nothing is delivered"""
    from sailfish_amd import _lib, quantfile
    rng = np.random.default_rng(47)
    n = 3000
    names = [f"name{i}" * (i % 5) for i in range(n)]
    cols = (names,) + _cfg3_like(rng, n)
    want = _want(cols)
    res = quantfile.text_size(*_dev(cols, gpu))
    assert res["n_bytes"] == len(want) and res["n_rows"] == n and res["max_row_bytes"] == int(_row_lengths(want).max())
    assert res["n_chunks"] == 0 and res["d2h_ms"] == 0.0 and res["n_slow"] == 0
    d = _dev(cols, gpu)
    rc, res2, chunks = _collect((_blob(names, gpu),) + d[1:], null_sink=True)
    assert rc == _lib.OK and chunks == [] and res2["n_bytes"] == len(want)


@pytest.mark.gpu
def test_name_offsets_are_checked(built, gpu):
    """name offsets that decrease, or do not start at 0, are refused"""
    from sailfish_amd import _lib
    rng = np.random.default_rng(48)
    names = [f"tx{i}" for i in range(100)]
    cols = (names,) + _cfg3_like(rng, 100)
    d = _dev(cols, gpu)
    blob, off = _blob(names, gpu)
    bad = off.clone(); bad[50] = bad[49] - 1
    rc, _, chunks = _collect(((blob, bad),) + d[1:])
    assert rc == _lib.ERR_INVALID and chunks == []
    bad = off.clone(); bad[0] = 1
    rc, _, chunks = _collect(((blob, bad),) + d[1:])
    assert rc == _lib.ERR_INVALID and chunks == []
    rc, _, chunks = _collect(((blob[:0], off),) + d[1:])          # offsets that announce name bytes, and a null blob
    assert rc == _lib.ERR_INVALID and chunks == []
    rc, _, chunks = _collect(((blob, off),) + d[1:])
    assert rc == _lib.OK and b"".join(chunks) == _want(cols)


@pytest.mark.gpu
def test_stream_order(built, gpu):
    """columns produced by torch ops queued on the current stream just before the call are the ones formatted"""
    from sailfish_amd import quantfile
    rng = np.random.default_rng(49)
    n = 200_000
    names = [f"t{i}" for i in range(n)]
    length, eff, tpm, cnt = _cfg3_like(rng, n)
    d_names = _blob(names, gpu)
    _, d_len, d_eff, d_tpm, d_cnt = _dev((names, length, eff, tpm, cnt), gpu)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(gpu), torch.cuda.Stream(gpu)):
        with torch.cuda.stream(stream):
            e2, t2, c2 = d_eff.clone(), d_tpm.clone(), d_cnt.clone()
            for _ in range(20):                                     # a queue of dependent updates, no synchronise before the call
                e2 = e2 * 1.25 + 1.0
                t2 = t2 * 0.5 + 0.125
                c2 = c2 * 3.0 + 7.0
            f = io.BytesIO()
            quantfile.write_rows(f, d_names, d_len, e2, t2, c2)
        he, ht, hc = eff.copy(), tpm.copy(), cnt.copy()
        for _ in range(20):                                         # (IEEE multiply and add, not fused: the same doubles)
            he = he * 1.25 + 1.0
            ht = ht * 0.5 + 0.125
            hc = hc * 3.0 + 7.0
        want = _want((names, length, he, ht, hc))
        assert f.getvalue() == want, _first_difference(f.getvalue(), want)


@pytest.mark.gpu
@pytest.mark.parametrize("no_len", [False, True])
def test_quantify_writes_quant_sf(built, gpu, tmp_path, no_len):
    """quantify(...): quant.sf equals the header plus format_rows of the experiment's columns, with and without
    noEffectiveLengthCorrection"""
    import sailfish_amd as sf
    from sailfish_amd import quantfile, writer
    from test_filter import _txome
    from test_gpu_eqfile import _hit_batches
    rng = np.random.default_rng(37)
    M, R = 400, 60_000
    seq, so, rl = _txome(rng, M, lo=400, hi=3000)
    names = [f"tx{i:04d}" for i in range(M)]
    out = str(tmp_path / "run")
    sopt = sf.SailfishOpts(numFragSamples=2000, noEffectiveLengthCorrection=no_len)
    rc, exp = sf.quant.quantify(names, rl, _hit_batches(rng, rl, R, True), "IU", out, sopt, seq=seq, seq_off=so, allow_orphans=True,
                                seed=7, device=gpu)
    assert rc == 0
    txps = exp.transcripts()
    t, length = writer.tpm(exp, sopt)
    ref = txps.RefLength.cpu().numpy().view(np.uint32)
    if no_len:
        assert np.array_equal(length.cpu().numpy(), ref.astype(np.float64))
    want = quantfile.HEADER + quantfile.format_rows(names, ref, length.cpu().numpy(), t.cpu().numpy(), txps.estCount.cpu().numpy())
    got = open(os.path.join(out, "quant.sf"), "rb").read()
    assert got == want, _first_difference(got, want)
    assert got.count(b"\n") == M + 1 and float(t.sum()) > 0
    # and the loop write_abundances ran before
    cnt = txps.estCount.cpu().numpy(); hl = length.cpu().numpy(); ht = t.cpu().numpy()
    loop = "Name\tLength\tEffectiveLength\tTPM\tNumReads\n" + "".join(
        f"{n}\t{int(ref[i])}\t{writer.fmt_g(hl[i])}\t{writer.fmt_g(ht[i])}\t{writer.fmt_g(cnt[i])}\n" for i, n in enumerate(names))
    assert got == loop.encode()


@pytest.mark.gpu
def test_cpp_adaptor_write_abundances(built, gpu, tmp_path):
    """writeAbundances in include/sfgpu_sailfish.hpp, compiled with g++ and run: its files hold the bytes Python writes for the
    same columns, and an unwritable path is refused with a message"""
    import struct

    from sailfish_amd import _lib, quantfile
    rng = np.random.default_rng(50)
    n = 3000
    names = [f"n{i}|gene{i % 17}" for i in range(n)]
    length, eff, _, cnt = _cfg3_like(rng, n)
    num_mapped = 12_345_678
    with open(tmp_path / "columns.tsv", "w") as f:
        for i in range(n):
            f.write(f"{names[i]}\t{int(length[i])}\t{struct.unpack('<Q', struct.pack('<d', eff[i]))[0]:016x}\t"
                    f"{struct.unpack('<Q', struct.pack('<d', cnt[i]))[0]:016x}\n")
    exe = tmp_path / "quantwrite_host_test"
    csrc = os.path.join(ROOT, "sailfish_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "quantwrite_host_test.cpp"), "-o", str(exe),
                           "-L", csrc, "-lsfgpu", "-L", "/opt/rocm/lib", "-lamdhip64", "-pthread",
                           "-Wl,-rpath," + csrc + ",-rpath,/opt/rocm/lib"])
    p, p_nolen = tmp_path / "quant.sf", tmp_path / "quant_nolen.sf"
    r = subprocess.run([str(exe), str(tmp_path / "columns.tsv"), str(num_mapped), str(p), str(p_nolen), str(tmp_path / "no_such_dir" / "quant.sf")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"wrote {n} rows" in r.stdout, r.stdout + r.stderr
    assert "refused:" in r.stdout and "no_such_dir" in r.stdout, r.stdout
    _, d_len, d_eff, _, d_cnt = _dev((names, length, eff, cnt, cnt), gpu)
    for path, d_l in ((p, d_eff), (p_nolen, torch.from_numpy(length.astype(np.float64)).to(gpu))):
        t = torch.zeros(n, dtype=torch.float64, device=gpu)
        with torch.cuda.device(gpu):
            _lib.check(_lib.lib().sfgpu_tpm(_lib.ptr(d_cnt), _lib.ptr(d_l), n, float(num_mapped), _lib.ptr(t), _lib.current_stream_ptr()))
        want = quantfile.HEADER + quantfile.format_rows(names, length, d_l.cpu().numpy(), t.cpu().numpy(), cnt)
        got = path.read_bytes()
        assert got == want, _first_difference(got, want)
        p2 = str(tmp_path / "py.sf")
        quantfile.write_file(p2, names, d_len, d_l, t, d_cnt)
        assert open(p2, "rb").read() == got
