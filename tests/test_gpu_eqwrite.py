"""eq_classes.txt written from the device (sfgpu_eqvec_write_text, sailfish_amd/csrc/eqtext_write.hip; eqfile.write_classes /
write_file / text_size; writer.write_equiv_counts; writeEquivCounts in include/sfgpu_sailfish.hpp).  The expected bytes are always
eqfile.format_text's on the host copy of the same arrays and, for small tables, also the per-class loop's."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32_MAX, U64_MAX = 2 ** 32 - 1, 2 ** 64 - 1


def _loop_writer(names, rowptr, ids, counts):
    """the per-class loop of GZipWriter::writeEquivCounts (GZipWriter.cpp:51-92) over plain arrays"""
    s = f"{len(names)}\n{len(counts)}\n" + "".join(n + "\n" for n in names)
    for c in range(len(counts)):
        lab = ids[rowptr[c]:rowptr[c + 1]]
        s += f"{len(lab)}\t" + "".join(f"{t}\t" for t in lab) + f"{counts[c]}\n"
    return s.encode()


def _table(lens, ids, counts):
    lens = np.asarray(lens, np.int64)
    rowptr = np.zeros(len(lens) + 1, np.int64); rowptr[1:] = np.cumsum(lens)
    ids = np.asarray(ids, np.uint32); counts = np.asarray(counts, np.uint64)
    assert len(ids) == rowptr[-1] and len(counts) == len(lens)
    return rowptr, ids, counts


def _dev(table, gpu):
    rowptr, ids, counts = table
    return (torch.from_numpy(rowptr.astype(np.uint32).view(np.int32)).to(gpu), torch.from_numpy(ids.view(np.int32).copy()).to(gpu),
            torch.from_numpy(counts.view(np.int64).copy()).to(gpu))


def _want(table, loop=False):
    """the class section: format_text without its header"""
    from sailfish_amd import eqfile
    text = eqfile.format_text([], *table)
    head = f"0\n{len(table[2])}\n".encode()
    assert text.startswith(head)
    if loop:
        assert _loop_writer([], *table) == text
    return text[len(head):]


def _collect(dev_table, chunk_bytes=0, refuse_at=None):
    """the C entry with a sink that keeps every chunk; returns (status, result dict, chunks)"""
    from sailfish_amd import _lib
    rowptr, ids, counts = dev_table
    chunks = []

    def sink(addr, n, _user):
        chunks.append(C.string_at(addr, n))
        return 1 if refuse_at is not None and len(chunks) == refuse_at else 0

    res = _lib.EqTextWriteResult()
    with torch.cuda.device(rowptr.device):
        rc = _lib.lib().sfgpu_eqvec_write_text(_lib.ptr(rowptr), _lib.ptr(ids), _lib.ptr(counts), counts.numel(), chunk_bytes,
                                               _lib.TEXT_SINK(sink), None, C.byref(res), _lib.current_stream_ptr())
    return rc, res.as_dict(), chunks


def _written(table, gpu, chunk_bytes=0):
    from sailfish_amd import eqfile
    f = io.BytesIO()
    res = eqfile.write_classes(f, _dev(table, gpu), chunk_bytes=chunk_bytes)
    return f.getvalue(), res


def _line_lengths(text):
    return np.diff(np.concatenate([[0], np.flatnonzero(np.frombuffer(text, np.uint8) == ord("\n")) + 1]))


def _greedy_chunks(line_len, chunk_bytes):
    n, cur = 0, 0
    for L in line_len:
        if cur and cur + L > chunk_bytes:
            n, cur = n + 1, 0
        cur += int(L)
    return n + (1 if cur else 0)


def _check_equal(table, gpu, loop=False, chunk_bytes=0):
    want = _want(table, loop=loop)
    got, res = _written(table, gpu, chunk_bytes)
    assert len(got) == len(want) and got == want
    assert res["n_bytes"] == len(want) and res["n_lines"] == len(table[2]) and res["n_ids"] == len(table[1])
    if len(want):
        assert res["max_line_bytes"] == int(_line_lengths(want).max())
    return res


@pytest.mark.gpu
def test_random_table(built, gpu):
    """a few thousand classes, label lengths 1 .. 200, ids below 200 000, small and large counts"""
    rng = np.random.default_rng(31)
    Cn = 5000
    lens = rng.integers(1, 201, Cn)
    counts = rng.integers(1, 100_000, Cn).astype(np.uint64)
    big = rng.random(Cn) < 0.05
    counts[big] = rng.integers(2 ** 32, 2 ** 63, int(big.sum()), dtype=np.uint64)
    table = _table(lens, rng.integers(0, 200_000, int(lens.sum())), counts)
    _check_equal(table, gpu, loop=True)
    _check_equal(table, gpu, chunk_bytes=5000)


@pytest.mark.gpu
def test_digit_boundaries(built, gpu):
    """ids 9, 10, 99, 100, ..., 999 999 999, 1 000 000 000, 2^32 - 1; counts at every power of ten up to 10^19 and 2^64 - 1;
    k of 1, 9, 10, 99, 100, 200; k = 0"""
    edge_ids = [0] + [v for e in range(1, 10) for v in (10 ** e - 1, 10 ** e)] + [U32_MAX - 1, U32_MAX]
    edge_counts = [0] + [v for e in range(0, 20) for v in (10 ** e - 1, 10 ** e, 10 ** e + 1)] + [2 ** 32 - 1, 2 ** 32, 2 ** 63, U64_MAX - 1, U64_MAX]
    lens, ids, counts = [], [], []
    for i, v in enumerate(edge_ids):                       # one-id labels, and every edge id inside a longer label
        lens.append(1); ids.append(v); counts.append(edge_counts[i % len(edge_counts)])
    lens.append(len(edge_ids)); ids.extend(edge_ids); counts.append(7)
    for i, v in enumerate(edge_counts):
        lens.append(2); ids.extend([i, edge_ids[i % len(edge_ids)]]); counts.append(v)
    for k in (1, 9, 10, 99, 100, 200, 0, 0, 3):
        lens.append(k); ids.extend(range(1000, 1000 + k)); counts.append(10 ** (k % 20))
    table = _table(lens, ids, counts)
    _check_equal(table, gpu, loop=True)
    # k = 0 first, last and alone
    _check_equal(_table([0, 2, 0], [5, 6], [1, 2, U64_MAX]), gpu, loop=True)
    got, _ = _written(_table([0], [], [12]), gpu)
    assert got == b"0\t12\n"


@pytest.mark.gpu
def test_long_label_among_short_ones(built, gpu):
    """one label of 100 000 ids among short ones"""
    rng = np.random.default_rng(32)
    lens = rng.integers(1, 8, 3000); lens[1500] = 100_000
    table = _table(lens, rng.integers(0, U32_MAX, int(lens.sum()), dtype=np.uint64), rng.integers(1, 5000, 3000))
    res = _check_equal(table, gpu)
    assert res["max_line_bytes"] > 500_000


@pytest.mark.gpu
def test_empty_table(built, gpu):
    from sailfish_amd import _lib
    empty = _dev(_table([], [], []), gpu)
    rc, res, chunks = _collect(empty)
    assert rc == _lib.OK and chunks == [] and res["n_bytes"] == 0 and res["n_chunks"] == 0 and res["n_lines"] == 0
    got, res = _written(_table([], [], []), gpu)
    assert got == b"" and res["n_bytes"] == 0


@pytest.mark.gpu
def test_chunk_edges(built, gpu):
    """every chunk size from the longest line up to a few hundred bytes: whole lines, greedy, in order; one byte less is refused
    before the sink is called; sizes outside [16, 2^30] are invalid arguments"""
    from sailfish_amd import _lib
    rng = np.random.default_rng(33)
    Cn = 400
    lens = rng.integers(1, 7, Cn)
    counts = rng.integers(1, 10 ** 6, Cn).astype(np.uint64); counts[77] = U64_MAX
    table = _table(lens, rng.integers(0, 10 ** 6, int(lens.sum())), counts)
    want = _want(table, loop=True)
    line_len = _line_lengths(want)
    max_line = int(line_len.max())
    assert max_line >= 18
    dev = _dev(table, gpu)
    for chunk in list(range(max_line, 321)) + [4095, 4096, 4097, len(want) - 1, len(want), len(want) + 1]:
        rc, res, chunks = _collect(dev, chunk)
        assert rc == _lib.OK, chunk
        assert b"".join(chunks) == want, chunk
        assert all(c.endswith(b"\n") and 0 < len(c) <= chunk for c in chunks), chunk
        assert res["n_chunks"] == len(chunks) == _greedy_chunks(line_len, chunk), chunk
        assert res["max_line_bytes"] == max_line and res["n_bytes"] == len(want)
    rc, res, chunks = _collect(dev, max_line - 1)
    assert max_line - 1 >= 16 and rc == _lib.ERR_RANGE and chunks == [] and res["n_chunks"] == 0
    assert res["max_line_bytes"] == max_line                      # the sizes are known when the call refuses
    for bad in (15, 2 ** 30 + 1):
        rc, res, chunks = _collect(dev, bad)
        assert rc == _lib.ERR_INVALID and chunks == []
    # a row pointer that decreases, one that does not start at 0, ids announced by the row pointer and a null id array
    rowptr, ids, counts = dev
    down = rowptr.clone(); down[200] = down[199] - 1
    for bad in ((down, ids, counts), (rowptr + 1, ids, counts), (rowptr, None, counts)):
        rc, res, chunks = _collect(bad, 4096)
        assert rc == _lib.ERR_INVALID and chunks == []
    rc, _, chunks = _collect(dev, 2 ** 30)
    assert rc == _lib.OK and b"".join(chunks) == want


@pytest.mark.gpu
def test_several_default_sized_chunks(built, gpu):
    """about a million classes: 8 MiB chunks (> 4 of them) and the default size; equality by bytes"""
    rng = np.random.default_rng(34)
    Cn = 1_000_000
    lens = rng.integers(1, 13, Cn)
    wide = rng.random(Cn) < 0.01
    lens[wide] = rng.integers(1, 301, int(wide.sum()))
    counts = rng.integers(1, 1000, Cn).astype(np.uint64)
    big = rng.random(Cn) < 0.05
    counts[big] = rng.integers(2 ** 32, 2 ** 40, int(big.sum()), dtype=np.uint64)
    table = _table(lens, rng.integers(0, 200_000, int(lens.sum())), counts)
    want = _want(table)
    line_len = _line_lengths(want)
    for chunk in (8 << 20, 0):
        got, res = _written(table, gpu, chunk)
        assert len(got) == len(want) and got == want
        assert res["n_chunks"] == _greedy_chunks(line_len, chunk or (32 << 20))
        if chunk:
            assert res["n_chunks"] > 4
        assert res["n_bytes"] == len(want) and res["n_lines"] == Cn and res["max_line_bytes"] == int(line_len.max())


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
    object's write comes out of write_classes and the library works afterwards"""
    from sailfish_amd import _lib, eqfile
    rng = np.random.default_rng(35)
    lens = rng.integers(1, 9, 2000)
    table = _table(lens, rng.integers(0, 10 ** 5, int(lens.sum())), rng.integers(1, 10 ** 4, 2000))
    want = _want(table)
    dev = _dev(table, gpu)
    rc, res, chunks = _collect(dev, 1024, refuse_at=2)
    assert rc == _lib.ERR_IO and len(chunks) == 2 and res["n_chunks"] == 2
    assert b"".join(chunks) == want[:len(chunks[0]) + len(chunks[1])]
    assert b"sink" in _lib.lib().sfgpu_last_error()
    f = _Refusing(fail_at=3)
    with pytest.raises(OSError, match="No space left on device"):
        eqfile.write_classes(f, dev, chunk_bytes=1024)
    assert f.calls == 3
    rc, _, chunks = _collect(dev, 1024)
    assert rc == _lib.OK and b"".join(chunks) == want


@pytest.mark.gpu
def test_sizing_only(built, gpu):
    """sink = NULL: the sizes equal the host's, nothing is delivered"""
    from sailfish_amd import eqfile
    rng = np.random.default_rng(36)
    lens = rng.integers(0, 40, 3000)
    table = _table(lens, rng.integers(0, U32_MAX, int(lens.sum()), dtype=np.uint64), rng.integers(0, 2 ** 63, 3000, dtype=np.uint64))
    want = _want(table)
    res = eqfile.text_size(_dev(table, gpu))
    assert res["n_bytes"] == len(want) and res["n_lines"] == 3000 and res["n_ids"] == int(lens.sum())
    assert res["max_line_bytes"] == int(_line_lengths(want).max())
    assert res["n_chunks"] == 0 and res["d2h_ms"] == 0.0


@pytest.mark.gpu
def test_round_trip_through_a_builder(built, gpu, tmp_path):
    """builder -> write_file -> a fresh builder's add_eq_file: the same table, hashes included"""
    import sailfish_amd as sf
    from sailfish_amd import eqfile, synth
    M, P, R = 3000, 8000, 300_000
    _, ids, off = synth.workload(M, P, R, device="cpu")
    names = [f"t{i}" for i in range(M)]
    eq = sf.EquivalenceClassBuilder(device=gpu); eq.start(); eq.add_batch(ids.to(gpu), off.to(gpu)); eq.finish()
    p = str(tmp_path / "eq_classes.txt")
    res = eqfile.write_file(p, names, eq.eqVec())
    a = eq.eqVec().to_numpy()
    assert res["n_lines"] == eq.n_classes and res["n_ids"] == eq.nnz
    text = open(p, "rb").read()
    assert text == eqfile.format_text(names, a[0], a[1], a[2]) == _loop_writer(names, a[0], a[1], a[2])
    eq2 = sf.EquivalenceClassBuilder(device=gpu); eq2.start()
    back = eq2.add_eq_file(p, names=names)
    eq2.finish()
    assert back["n_lines"] == eq.n_classes and back["sum_counts"] == eq.total_reads
    for x, y, what in zip(a, eq2.eqVec().to_numpy(), ("rowptr", "ids", "counts", "hashes")):
        assert x.dtype == y.dtype and np.array_equal(x, y), what


@pytest.mark.gpu
def test_quantify_dump_eq(built, gpu, tmp_path):
    """quantify(dumpEq=True): aux/eq_classes.txt equals format_text(names, *table)"""
    import sailfish_amd as sf
    from sailfish_amd import eqfile
    from test_filter import _txome
    from test_gpu_eqfile import _hit_batches
    rng = np.random.default_rng(37)
    M, R = 400, 60_000
    seq, so, rl = _txome(rng, M, lo=400, hi=3000)
    names = [f"tx{i:04d}" for i in range(M)]
    out = str(tmp_path / "run")
    rc, exp = sf.quant.quantify(names, rl, _hit_batches(rng, rl, R, True), "IU", out, sf.SailfishOpts(dumpEq=True, numFragSamples=2000),
                                seq=seq, seq_off=so, allow_orphans=True, seed=7, device=gpu)
    assert rc == 0
    rp, ii, cc, _ = exp.equivalenceClassBuilder().eqVec().to_numpy()
    assert len(cc) > 100
    assert open(os.path.join(out, "aux", "eq_classes.txt"), "rb").read() == eqfile.format_text(names, rp, ii, cc)


@pytest.mark.gpu
def test_stream_order(built, gpu):
    """arrays produced by torch ops queued on the current stream just before the call are the ones formatted"""
    rng = np.random.default_rng(38)
    Cn = 200_000
    lens = rng.integers(1, 10, Cn)
    table = _table(lens, rng.integers(0, 10 ** 6, int(lens.sum())), rng.integers(1, 10 ** 5, Cn))
    rowptr, ids, counts = _dev(table, gpu)
    torch.cuda.synchronize()
    from sailfish_amd import eqfile
    for stream in (torch.cuda.current_stream(gpu), torch.cuda.Stream(gpu)):
        with torch.cuda.stream(stream):
            ids2, counts2 = ids.clone(), counts.clone()
            for _ in range(20):                                     # a queue of dependent updates, no synchronise before the call
                ids2 = ids2 * 3 + 1
                counts2 = counts2 * 5 + 7
            f = io.BytesIO()
            eqfile.write_classes(f, (rowptr, ids2, counts2))
        h_ids, h_counts = table[1].copy(), table[2].copy()
        for _ in range(20):
            h_ids = h_ids * np.uint32(3) + np.uint32(1)             # wraps like the int32 device arithmetic
            h_counts = h_counts * np.uint64(5) + np.uint64(7)
        assert f.getvalue() == _want((table[0], h_ids, h_counts))


@pytest.mark.gpu
def test_cpp_adaptor_write_equiv_counts(built, gpu, tmp_path):
    """writeEquivCounts in include/sfgpu_sailfish.hpp, compiled with g++ and run: the file loads back into the same table
    (checked by the program) and holds the bytes Python writes for it"""
    import sailfish_amd as sf
    from sailfish_amd import eqfile
    names = [f"n{i}" for i in range(300)]
    (tmp_path / "names.txt").write_text("".join(n + "\n" for n in names))
    exe = tmp_path / "eqwrite_host_test"
    csrc = os.path.join(ROOT, "sailfish_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "eqwrite_host_test.cpp"), "-o", str(exe),
                           "-L", csrc, "-lsfgpu", "-L", "/opt/rocm/lib", "-lamdhip64", "-pthread",
                           "-Wl,-rpath," + csrc + ",-rpath,/opt/rocm/lib"])
    p = tmp_path / "eq_classes.txt"
    r = subprocess.run([str(exe), str(tmp_path / "names.txt"), str(p), str(tmp_path / "no_such_dir" / "eq.txt")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "round trip ok" in r.stdout, r.stdout + r.stderr
    assert "refused:" in r.stdout and "no_such_dir" in r.stdout, r.stdout
    text = p.read_bytes()
    eq = sf.EquivalenceClassBuilder(device=gpu); eq.start()
    eq.add_eq_file(str(p), names=names)
    eq.finish()
    rp, ii, cc, _ = eq.eqVec().to_numpy()
    assert len(cc) > 1000 and int(cc.max()) == 4_000_000_000
    assert text == eqfile.format_text(names, rp, ii, cc)
    assert text == _loop_writer(names, rp, ii, cc)
    # and through Python's writer
    p2 = str(tmp_path / "py.txt")
    eqfile.write_file(p2, names, eq.eqVec())
    assert open(p2, "rb").read() == text
