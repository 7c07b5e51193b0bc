"""quant.genes.sf from the device (sfgpu_genes_aggregate / sfgpu_genes_write_text, sailfish_amd/csrc/genes.hip with the fold of
csrc/genefold.h and the printed-value rounding of csrc/gfmt.h; genes.aggregate_columns; quantify(..., gene_map=...);
aggregateEstimatesToGeneLevel in include/sfgpu_sailfish.hpp).  The expected bytes are always the host function's:
genes.aggregate_estimates_to_gene_level applied to the quant.sf that quantfile.write_file wrote from the same columns.  No
tolerance anywhere: files are compared byte for byte, doubles bit for bit."""
import ctypes as C
import io
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from test_genes_cpu import bits, build_harness, harness_fold, random_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "Name\tLength\tEffectiveLength\tTPM\tNumReads"


def _dev(length, eff, tpm, nr, gpu):
    return (torch.from_numpy(np.asarray(length, np.uint32).view(np.int32).copy()).to(gpu),
            torch.from_numpy(np.asarray(eff, np.float64).copy()).to(gpu), torch.from_numpy(np.asarray(tpm, np.float64).copy()).to(gpu),
            torch.from_numpy(np.asarray(nr, np.float64).copy()).to(gpu))


def _ids(a, gpu):
    return torch.from_numpy(np.asarray(a, np.uint32).view(np.int32).copy()).to(gpu)


def _first_difference(got, want):
    n = min(len(got), len(want))
    a, b = np.frombuffer(got, np.uint8, n), np.frombuffer(want, np.uint8, n)
    d = np.flatnonzero(a != b)
    i = int(d[0]) if len(d) else n
    lo = want.rfind(b"\n", 0, i) + 1
    return f"lengths {len(got)} / {len(want)}, first difference at byte {i}: got {got[lo:i + 60]!r}, want {want[lo:i + 60]!r}"


def _host_file(tmp_path, tgm, names, dcols):
    """the host function on the quant.sf written from the same device columns"""
    from sailfish_amd import genes, quantfile
    d = tmp_path / "host"
    d.mkdir(exist_ok=True)
    quantfile.write_file(str(d / "quant.sf"), list(names), *dcols)
    return open(genes.aggregate_estimates_to_gene_level(tgm, str(d / "quant.sf")), "rb").read()


def _check_columns(tmp_path, tgm, names, cols, gpu):
    """aggregate_columns against the host function; returns the result dicts"""
    from sailfish_amd import genes
    dcols = _dev(*cols, gpu)
    want = _host_file(tmp_path, tgm, names, dcols)
    out = str(tmp_path / "dev.genes.sf")
    res = genes.aggregate_columns(tgm, list(names), *dcols, out)
    got = open(out, "rb").read()
    assert got == want, _first_difference(got, want)
    assert res["aggregate"]["n_rows"] == len(names) and res["aggregate"]["n_genes"] == want.count(b"\n") - 1
    return res


def _map_for(names, gene_names):
    from sailfish_amd import genes
    return genes.TranscriptGeneMap(list(zip(names, gene_names)))


def _rows(table, gid, cols):
    """expected rows for write_gene_rows: Python's "%g" on all four columns"""
    out = []
    for k, i in enumerate(gid):
        nm = table[i] if isinstance(table[i], bytes) else table[i].encode()
        out.append(nm + ("\t%g\t%g\t%g\t%g\n" % (cols[0][k], cols[1][k], cols[2][k], cols[3][k])).encode())
    return out


@pytest.mark.gpu
def test_four_row_table(built, gpu, tmp_path):
    """the table of test_genes.py::test_gene_level_aggregation: the same five lines"""
    from sailfish_amd import genes
    (tmp_path / "map.tsv").write_text("tB g1\ntA g1\ntC g2\ntE g3\n")
    tgm = genes.TranscriptGeneMap.from_file(str(tmp_path / "map.tsv"))
    dcols = _dev([1000, 2000, 500, 700], [800.0, 1800.0, 300.0, 500.0], [30.0, 10.0, 0.0, 5.0], [60.0, 40.0, 0.0, 7.0], gpu)
    out = str(tmp_path / "quant.genes.sf")
    res = genes.aggregate_columns(tgm, ["tA", "tB", "tC", "tZ"], *dcols, out, comments=("# sailfish (quasi) v0.10.0", HEADER))
    assert open(out).read().split("\n") == ["# sailfish (quasi) v0.10.0", HEADER, "g1\t714.286\t600\t40\t100", "g2\t500\t300\t0\t0",
                                            "tZ\t700\t500\t5\t7", ""]
    assert res["aggregate"]["n_genes"] == 3 and res["aggregate"]["max_rows_per_gene"] == 2 and res["aggregate"]["n_slow"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [21, 22])
def test_random_tables(built, gpu, tmp_path, seed):
    """3 000 - 5 000 rows, gene sizes 1, 2, 63, 64, 65 and 257 among small ones, rows of a gene interleaved with the others', a
    third of the genes unexpressed: byte-equal through aggregate_columns, and through the two entries with sparse ids"""
    from sailfish_amd import genes
    rng = np.random.default_rng(seed)
    gene, length, eff, tpm, cnt, unexpressed = random_table(rng, [1, 2, 63, 64, 65, 257, 257, 65, 64, 63, 2, 1], 600)
    n = len(gene)
    assert 3000 <= n <= 5000 and 0.2 < unexpressed.mean() < 0.45
    names = [f"ENST{i:08d}.{1 + i % 7}" for i in range(n)]
    tgm = _map_for(names, [f"ENSG{g:07d}" for g in gene])
    res = _check_columns(tmp_path, tgm, names, (length, eff, tpm, cnt), gpu)
    assert res["aggregate"]["n_slow"] == 0 and res["write"]["n_slow"] == 0 and res["aggregate"]["max_rows_per_gene"] == 257
    # ids sparse in n_gene_ids: gene g is id 7 g + 3 of a table of 7 G + 10 names
    G = int(gene.max()) + 1
    table = [f"unused{i}" for i in range(7 * G + 10)]
    for g in range(G):
        table[7 * g + 3] = f"ENSG{g:07d}"
    dcols = _dev(length, eff, tpm, cnt, gpu)
    gid, *gcols, agg = genes.aggregate_device(_ids(7 * gene + 3, gpu), len(table), *dcols)
    f = io.BytesIO()
    genes.write_gene_rows(f, table, gid, *gcols)
    want = _host_file(tmp_path, tgm, names, dcols)
    got = (HEADER + "\n").encode() + f.getvalue()
    assert got == want, _first_difference(got, want)
    assert agg["n_genes"] == G and agg["n_slow"] == 0


def _wide_values():
    out = []
    rng = np.random.default_rng(23)
    for j in range(-12, 17):                                        # ties (d + 1/2) 10^j and their neighbours
        for d in rng.integers(100000, 1000000, 6):
            f = float(Fraction(2 * int(d) + 1, 2) * Fraction(10) ** j)
            out += [f, math.nextafter(f, 0.0), math.nextafter(f, math.inf)]
    for k in range(-320, 309, 7):                                   # decade edges, inside and outside the |k| <= 22 window
        p = float(f"1e{k}")
        out += [p, math.nextafter(p, 0.0)]
        if k < 308:
            out.append(float(f"9.999995e{k}"))
    out += [5e-324, 1e-323, 2.2250738585072014e-308, 2.225073858507201e-308, 1.7976931348623157e308, 1e23, 1e22, 8.5e-23, 1.234565e-30,
            7.3e40, 0.0, -0.0, math.inf, -math.inf, math.nan, 0.5, 1.0, 123456.5, 999999.5, 0.0001]
    return out + [-x for x in out]


@pytest.mark.gpu
def test_wide_range_table(built, gpu, tmp_path):
    """ties, decade edges, values outside the one-operation window, denormals, inf, nan and -0.0 in every double column, and a
    gene whose sums overflow: byte-equal, and the slow halves ran"""
    rng = np.random.default_rng(24)
    vals = np.array(_wide_values(), np.float64)
    n = 3 * len(vals)
    assert 2000 <= n <= 6000
    eff = np.concatenate([vals, rng.permutation(vals), 10.0 ** rng.uniform(0, 5, len(vals))])
    tpm = np.concatenate([10.0 ** rng.uniform(-3, 4, len(vals)), vals, np.abs(rng.permutation(vals))])
    cnt = np.concatenate([rng.permutation(vals), 10.0 ** rng.uniform(-3, 4, len(vals)), vals])
    length = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    gene = rng.permutation(np.arange(n) // 5)
    # a gene of three rows whose TPM and NumReads sums overflow to inf
    G = int(gene.max()) + 1
    gene = np.concatenate([gene, [G, G, G]])
    length = np.concatenate([length, [100, 200, 300]]).astype(np.uint32)
    eff = np.concatenate([eff, [90.0, 180.0, 270.0]])
    tpm = np.concatenate([tpm, [1.7e308, 1.7e308, 1.0]])
    cnt = np.concatenate([cnt, [1e308, 9e307, 8e307]])
    names = [f"t{i:05d}" for i in range(len(gene))]
    tgm = _map_for(names, [f"g{g}" for g in gene])
    res = _check_columns(tmp_path, tgm, names, (length, eff, tpm, cnt), gpu)
    assert res["aggregate"]["n_slow"] > 100 and res["write"]["n_slow"] > 0
    lines = open(tmp_path / "dev.genes.sf").read().split("\n")
    assert [l for l in lines if l.startswith(f"g{G}\t")][0].split("\t")[3:] == ["inf", "inf"]


@pytest.mark.gpu
def test_degenerate_tables(built, gpu, tmp_path):
    """one gene holding all 5 000 rows; every row its own gene; no rows; an own-gene name that collides with a map gene"""
    from sailfish_amd import genes
    rng = np.random.default_rng(25)
    n = 5000
    _, length, eff, tpm, cnt, _ = random_table(rng, [n], 0)
    names = [f"t{i:05d}" for i in range(n)]
    res = _check_columns(tmp_path, _map_for(names, ["only"] * n), names, (length, eff, tpm, cnt), gpu)
    assert res["aggregate"]["n_genes"] == 1 and res["aggregate"]["max_rows_per_gene"] == n
    # every name lies past the last name of the map: its own gene
    res = _check_columns(tmp_path, _map_for(["a"], ["ga"]), names, (length, eff, tpm, cnt), gpu)
    assert res["aggregate"]["n_genes"] == n and res["aggregate"]["max_rows_per_gene"] == 1
    # ... and with an empty map
    _check_columns(tmp_path, genes.TranscriptGeneMap([]), names[:100], (length[:100], eff[:100], tpm[:100], cnt[:100]), gpu)
    # no rows: the comment lines alone
    e = np.zeros(0)
    res = _check_columns(tmp_path, _map_for(["a"], ["ga"]), [], (np.zeros(0, np.uint32), e, e, e), gpu)
    assert res["aggregate"]["n_genes"] == 0 and open(tmp_path / "dev.genes.sf").read() == HEADER + "\n"
    # "zz" is past the last transcript name, so it is its own gene -- and a gene of the map is called "zz": they are one gene
    tgm = _map_for(["tA", "tB", "tC"], ["zz", "g2", "zz"])
    names6 = ["tB", "zz", "tA", "zy", "tC", "zz"]
    res = _check_columns(tmp_path, tgm, names6, (length[:6], eff[:6], np.abs(tpm[:6]) + 1.0, cnt[:6]), gpu)
    assert res["aggregate"]["n_genes"] == 3 and res["aggregate"]["max_rows_per_gene"] == 4
    assert [l.split("\t")[0] for l in open(tmp_path / "dev.genes.sf").read().split("\n")[1:-1]] == ["g2", "zz", "zy"]


@pytest.mark.gpu
def test_raw_doubles_fold(built, gpu, tmp_path):
    """as_printed = 0 folds the doubles as they are: bit-equal to genefold.h run by the g++ harness on the raw doubles, and
    different from as_printed = 1 on a table where the rounding matters"""
    from sailfish_amd import genes
    rng = np.random.default_rng(26)
    gene, length, eff, tpm, cnt, _ = random_table(rng, [1, 2, 63, 64, 65, 257], 500)
    G = int(gene.max()) + 1
    dcols = _dev(length, eff, tpm, cnt, gpu)
    exe = build_harness(tmp_path)
    first_seen = list(dict.fromkeys(gene.tolist()))
    outs = {}
    for as_printed in (False, True):
        gid, gl, ge, gt, gc, agg = genes.aggregate_device(_ids(gene, gpu), G, *dcols, as_printed=as_printed)
        assert gid.cpu().numpy().view(np.uint32).tolist() == first_seen and agg["n_genes"] == G
        got = [tuple(int(x) for x in row) for row in zip(*(t.cpu().numpy().view(np.uint64) for t in (gl, ge, gt, gc)))]
        want = harness_fold(exe, tmp_path, gene, length, eff, tpm, cnt, printed=as_printed)
        assert [w[0] for w in want] == first_seen
        assert got == [w[1:] for w in want]
        outs[as_printed] = got
    assert sum(a != b for a, b in zip(outs[False], outs[True])) > G // 2


@pytest.mark.gpu
def test_gene_id_out_of_range(built, gpu):
    """an id >= n_gene_ids is refused with SFGPU_ERR_INVALID and no output is written"""
    from sailfish_amd import _lib, genes
    rng = np.random.default_rng(27)
    n = 3000
    gene = rng.integers(0, 500, n)
    dcols = _dev(rng.integers(1, 1000, n), rng.random(n) * 100, rng.random(n), rng.random(n) * 10, gpu)
    outs = [torch.full((500,), -7, dtype=torch.int32, device=gpu)] + [torch.full((500,), -7.0, dtype=torch.float64, device=gpu) for _ in range(4)]
    for bad_row in (0, 1234, n - 1):
        bad = gene.copy(); bad[bad_row] = 500
        d_bad = _ids(bad, gpu)
        res = _lib.GenesResult()
        with torch.cuda.device(gpu):
            rc = _lib.lib().sfgpu_genes_aggregate(_lib.ptr(d_bad), *[_lib.ptr(c) for c in dcols], n, 500, 1, *[_lib.ptr(o) for o in outs],
                                                  C.byref(res), _lib.current_stream_ptr())
        torch.cuda.synchronize()
        assert rc == _lib.ERR_INVALID and b"gene id" in _lib.lib().sfgpu_last_error()
        assert res.n_genes == 0 and all(bool((o == -7).all()) for o in outs)
    with pytest.raises(_lib.SfgpuError):
        genes.aggregate_device(_ids(gene, gpu), 400, *dcols)
    gid, *_ = genes.aggregate_device(_ids(gene, gpu), 500, *dcols)      # the library works afterwards
    assert gid.numel() == len(set(gene.tolist()))


def _collect(table_dev, n_names, gid, gcols, chunk_bytes=0, refuse_at=None, null_sink=False):
    from sailfish_amd import _lib
    blob, off = table_dev
    chunks = []

    def sink(addr, n, _user):
        chunks.append(C.string_at(addr, n))
        return 1 if refuse_at is not None and len(chunks) == refuse_at else 0

    res = _lib.QuantWriteResult()
    with torch.cuda.device(gid.device):
        rc = _lib.lib().sfgpu_genes_write_text(_lib.ptr(blob) if blob.numel() else None, _lib.ptr(off), n_names, _lib.ptr(gid),
                                               *[_lib.ptr(c) for c in gcols], gid.numel(), chunk_bytes,
                                               _lib.TEXT_SINK(0) if null_sink else _lib.TEXT_SINK(sink), None, C.byref(res),
                                               _lib.current_stream_ptr())
    return rc, res.as_dict(), chunks


def _greedy_chunks(row_len, chunk_bytes):
    n, cur = 0, 0
    for L in row_len:
        if cur and cur + L > chunk_bytes:
            n, cur = n + 1, 0
        cur += int(L)
    return n + (1 if cur else 0)


@pytest.mark.gpu
def test_writer_edges(built, gpu):
    """sfgpu_genes_write_text: chunk sizes of 16 bytes, of exactly one row and of one byte less; greedy chunk counts; sizing only;
    a sink refusal at the second chunk; names of 0 and of 5 000 bytes; a name index outside the table"""
    from sailfish_amd import _lib, quantfile
    rng = np.random.default_rng(28)
    n_names, n = 900, 700
    table = [f"gene{i}".encode() * int(rng.integers(1, 3)) for i in range(n_names)]
    table[5] = b""
    table[17] = bytes(rng.integers(33, 127, 5000, dtype=np.uint8))
    gid = rng.permutation(n_names)[:n].astype(np.uint32)
    gid[0], gid[n // 2], gid[n - 1] = 17, 5, 17                     # (a name may serve several rows)
    cols = [np.where(rng.random(n) < 0.3, 0.0, 10.0 ** rng.uniform(-6, 6, n)) for _ in range(4)]
    cols[0][3], cols[1][4], cols[2][5], cols[3][6] = 1e-300, math.inf, -0.0, math.nan
    rows = _rows(table, gid, cols)
    want = b"".join(rows)
    row_len = [len(r) for r in rows]
    b, o = quantfile.names_blob(table)
    tdev = (torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(gpu), torch.from_numpy(o.view(np.int64).copy()).to(gpu))
    d_gid = _ids(gid, gpu)
    gcols = [torch.from_numpy(c.copy()).to(gpu) for c in cols]
    max_row = max(row_len)
    assert max_row > 5000
    for chunk in (0, max_row, max_row + 1, 2 * max_row, len(want) - 1, len(want)):
        rc, res, chunks = _collect(tdev, n_names, d_gid, gcols, chunk)
        assert rc == _lib.OK and b"".join(chunks) == want, chunk
        assert res["n_chunks"] == len(chunks) == _greedy_chunks(row_len, chunk or (32 << 20)), chunk
        assert all(c.endswith(b"\n") for c in chunks) and res["max_row_bytes"] == max_row and res["n_bytes"] == len(want)
        assert res["n_rows"] == n and res["n_slow"] == 1
    rc, res, chunks = _collect(tdev, n_names, d_gid, gcols, max_row - 1)
    assert rc == _lib.ERR_RANGE and chunks == [] and res["n_chunks"] == 0 and res["max_row_bytes"] == max_row
    # short rows only: 16-byte chunks hold one row each when a row is 9 .. 16 bytes long
    short_tab = [b"", b"ab", b"c"]
    sgid = np.array([1, 0, 2, 1, 1, 0], np.uint32)
    scols = [np.array([1.0, 2.5, 0.0, 10.0, 3.0, 4.0]), np.array([2.0, 0.5, 1.0, 7.0, 1.0, 1.0]), np.array([0.0, 1.0, 2.0, 3.0, 4.0, 5.0]),
             np.array([5.0, 1.0, 1.0, 0.0, 9.0, 1.0])]
    srows = _rows(short_tab, sgid, scols)
    assert max(len(r) for r in srows) <= 16 and min(len(r) for r in srows) >= 9
    b, o = quantfile.names_blob(short_tab)
    sdev = (torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(gpu), torch.from_numpy(o.view(np.int64).copy()).to(gpu))
    rc, res, chunks = _collect(sdev, 3, _ids(sgid, gpu), [torch.from_numpy(c).to(gpu) for c in scols], 16)
    assert rc == _lib.OK and chunks == srows and res["n_chunks"] == len(srows)
    for bad in (15, 2 ** 30 + 1):
        rc, _, chunks = _collect(tdev, n_names, d_gid, gcols, bad)
        assert rc == _lib.ERR_INVALID and chunks == []
    # sizing only
    rc, res, chunks = _collect(tdev, n_names, d_gid, gcols, null_sink=True)
    assert rc == _lib.OK and chunks == [] and res["n_bytes"] == len(want) and res["max_row_bytes"] == max_row
    assert res["n_chunks"] == 0 and res["d2h_ms"] == 0.0
    # a sink that refuses the second chunk
    rc, res, chunks = _collect(tdev, n_names, d_gid, gcols, 6000, refuse_at=2)
    assert rc == _lib.ERR_IO and len(chunks) == 2 and res["n_chunks"] == 2 and b"".join(chunks) == want[:len(chunks[0]) + len(chunks[1])]
    assert b"sink" in _lib.lib().sfgpu_last_error()
    # a name index that the table does not have
    bad = gid.copy(); bad[100] = n_names
    rc, _, chunks = _collect(tdev, n_names, _ids(bad, gpu), gcols)
    assert rc == _lib.ERR_INVALID and chunks == []
    rc, _, chunks = _collect(tdev, n_names, d_gid, gcols)
    assert rc == _lib.OK and b"".join(chunks) == want


@pytest.mark.gpu
def test_stream_order(built, gpu):
    """Both entries queue behind the caller's stream: 200 000 rows whose columns are produced by a chain of torch kernels queued
    just before the call, with no host copy, allocation from the host or synchronise in between -- ids, lengths and the name
    table are on the device beforehand, the entries are called directly (aggregate_device, write_gene_rows with a device name
    table).  The expectation comes from the same arithmetic on the host, uploaded and synchronised first."""
    from sailfish_amd import genes, quantfile
    rng = np.random.default_rng(29)
    n, G = 200_000, 24_000
    gene = rng.integers(0, G, n)
    length = rng.integers(200, 100_000, n).astype(np.uint32)
    eff = np.maximum(length.astype(np.float64) - rng.random(n) * 180.0, 1.0)
    cnt = np.where(rng.random(n) < 0.3, 0.0, 10.0 ** rng.uniform(-6, 5, n))
    tpm = cnt / eff / (cnt / eff).sum() * 1e6
    he, ht, hc = eff.copy(), tpm.copy(), cnt.copy()
    for _ in range(20):                                             # (IEEE multiply and add, not fused: the same doubles as below)
        he = he * 1.25 + 1.0
        ht = ht * 0.5 + 0.125
        hc = hc * 3.0 + 7.0
    d_gene = _ids(gene, gpu)
    d_len, d_eff, d_tpm, d_cnt = _dev(length, eff, tpm, cnt, gpu)
    # what the entries give for the finished columns, uploaded and waited for
    finished = _dev(length, he, ht, hc, gpu)                        # (kept alive: its blocks must not come back as e2, t2, c2)
    want_gid, *want_cols, want_agg = genes.aggregate_device(d_gene, G, *finished)
    want_cols_h = [c.cpu().numpy() for c in want_cols]
    n_genes = want_gid.numel()
    assert n_genes > 20_000 and want_agg["n_slow"] == 0
    table = [f"ENSG{g:011d}" for g in range(G)]
    b, o = quantfile.names_blob(table)
    d_table = (torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(gpu), torch.from_numpy(o.view(np.int64).copy()).to(gpu))
    hw = [c.copy() for c in want_cols_h]
    for _ in range(20):
        hw = [hw[0] * 1.25 + 1.0, hw[1] * 0.5 + 0.125, hw[2] * 3.0 + 7.0, hw[3] * 0.75 + 2.0]
    want_text = b"".join(_rows(table, want_gid.cpu().numpy().view(np.uint32), hw))
    ballast = torch.zeros(32 << 20, dtype=torch.float64, device=gpu)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(gpu), torch.cuda.Stream(gpu)):
        with torch.cuda.stream(stream):
            for _ in range(150):                                    # 150 passes over 256 MB, tens of milliseconds of work ahead of
                ballast.add_(1.0)                                   # the chain: the stream is busy when the entry is called
            e2, t2, c2 = d_eff.clone(), d_tpm.clone(), d_cnt.clone()
            for _ in range(20):                                     # a queue of dependent updates, no synchronise before the call
                e2 = e2 * 1.25 + 1.0
                t2 = t2 * 0.5 + 0.125
                c2 = c2 * 3.0 + 7.0
            gid, *gcols, agg = genes.aggregate_device(d_gene, G, d_len, e2, t2, c2)
            # ... and the writer behind a chain on the gene columns
            for _ in range(150):
                ballast.add_(1.0)
            w = [c.clone() for c in want_cols]
            for _ in range(20):
                w = [w[0] * 1.25 + 1.0, w[1] * 0.5 + 0.125, w[2] * 3.0 + 7.0, w[3] * 0.75 + 2.0]
            f = io.BytesIO()
            genes.write_gene_rows(f, d_table, want_gid, *w)
        ok = dict(lines=agg["n_genes"] == n_genes and torch.equal(gid, want_gid),
                  columns=all(np.array_equal(got.cpu().numpy().view(np.uint64), want.view(np.uint64)) for got, want in zip(gcols, want_cols_h)),
                  text=f.getvalue() == want_text)
        assert all(ok.values()), (ok, _first_difference(f.getvalue(), want_text))


def _toy_batches(rng, rl, M, R):
    """the workload of test_quant.py::test_quantify_matches_the_oracle_chain: pairs of transcripts sharing most fragments"""
    from oracle import oracle as O
    batches = []
    for b in range(3):
        n = R // 3
        j = rng.integers(0, M // 2, n)
        shared = rng.random(n) < 0.94
        k = np.where(shared, 2, 1)
        off = np.zeros(n + 1, np.uint32); off[1:] = np.cumsum(k)
        h = np.zeros(int(off[-1]), O.HIT_DTYPE)
        first = off[:-1].astype(np.int64)
        h["tid"][first] = 2 * j
        h["tid"][first[shared] + 1] = 2 * j[shared] + 1
        h["mate_status"] = 3
        L = rl[h["tid"]].astype(np.int64)
        left = (rng.random(len(h)) * np.maximum(L - 260, 1)).astype(np.int32)
        h["frag_len"] = rng.integers(120, 260, len(h))
        fw = np.repeat(rng.integers(0, 2, n), k)
        h["pos"] = np.where(fw == 1, left, left + h["frag_len"] - 50); h["mate_pos"] = np.where(fw == 1, left + h["frag_len"] - 50, left)
        h["read_len"] = 50; h["mate_len"] = 50; h["fwd"] = fw; h["mate_fwd"] = 1 - fw
        batches.append((h, off))
    return batches


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["tsv", "gtf", "gtf_gene_name"])
def test_quantify_with_a_gene_map(built, gpu, tmp_path, form):
    """quantify(..., gene_map=...): quant.genes.sf holds the bytes the host function writes afterwards from the written quant.sf,
    for the two-column map and for the .gtf form; txpAggregationKey selects the GTF attribute"""
    import sailfish_amd as sf
    from sailfish_amd import genes
    from test_filter import _txome
    rng = np.random.default_rng(41)
    M, R = 300, 60_000
    seq, so, rl = _txome(rng, M, lo=400, hi=3000)
    names = [f"tx{i:04d}" for i in range(M)]
    if form == "tsv":
        gm = tmp_path / "map.tsv"
        gm.write_text("".join(f"{n} g{i // 3}\n" for i, n in enumerate(names[:-4])))     # the last four: their own genes
    else:
        gm = tmp_path / "map.gtf"
        gm.write_text("".join(f'chr1\tsrc\texon\t1\t300\t.\t+\t.\tgene_id "G{i // 3}"; transcript_id "{n}"; gene_name "N{i // 5}";\n'
                              for i, n in enumerate(names)))
    key = "gene_name" if form == "gtf_gene_name" else "gene_id"
    sopt = sf.SailfishOpts(numFragSamples=2000, numBootstraps=2, txpAggregationKey=key)
    assert sf.SailfishOpts().txpAggregationKey == "gene_id"
    out = str(tmp_path / "out")
    rc, exp = sf.quant.quantify(names, rl, _toy_batches(rng, rl, M, R), "IU", out, sopt, seq=seq, seq_off=so, allow_orphans=True,
                                gene_map=str(gm), seed=3, device=gpu)
    assert rc == 0
    got = open(os.path.join(out, "quant.genes.sf"), "rb").read()
    os.rename(os.path.join(out, "quant.genes.sf"), os.path.join(out, "device.genes.sf"))
    tgm = genes.TranscriptGeneMap.from_file(str(gm)) if form == "tsv" else genes.TranscriptGeneMap.from_gtf(str(gm), key)
    want = open(genes.aggregate_estimates_to_gene_level(tgm, os.path.join(out, "quant.sf")), "rb").read()
    assert got == want, _first_difference(got, want)
    lines = got.decode().split("\n")
    assert lines[0] == HEADER and lines[-1] == ""
    n_genes = {"tsv": (M - 4 + 2) // 3 + 4, "gtf": M // 3, "gtf_gene_name": M // 5}[form]
    assert len(lines) == 2 + n_genes
    assert lines[1].startswith({"tsv": "g0\t", "gtf": "G0\t", "gtf_gene_name": "N0\t"}[form])
    assert sum(float(l.split("\t")[4]) for l in lines[1:-1]) > 0.5 * R
    # and what the entry point does without the columns is unchanged: the same file from the file
    assert open(genes.generate_gene_level_estimates(str(gm), out, key), "rb").read() == got


@pytest.mark.gpu
def test_cpp_adaptor_gene_level(built, gpu, tmp_path):
    """aggregateEstimatesToGeneLevel in include/sfgpu_sailfish.hpp, compiled with g++ and run: its file holds the bytes of the
    Python device path for the same columns, and an unwritable path is refused with a message"""
    from sailfish_amd import _lib, genes
    rng = np.random.default_rng(30)
    gene, length, eff, _, cnt, _ = random_table(rng, [1, 2, 63, 64, 65, 257], 500)
    n = len(gene)
    names = [f"n{i}|x" for i in range(n)]
    gene_names = [f"gene{g}" for g in gene]
    num_mapped = 12_345_678
    with open(tmp_path / "columns.tsv", "w") as f:
        for i in range(n):
            f.write(f"{names[i]}\t{int(length[i])}\t{bits(eff[i]):016x}\t{bits(cnt[i]):016x}\t{gene_names[i]}\n")
    exe = tmp_path / "genes_host_test"
    csrc = os.path.join(ROOT, "sailfish_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "genes_host_test.cpp"), "-o", str(exe),
                           "-L", csrc, "-lsfgpu", "-L", "/opt/rocm/lib", "-lamdhip64", "-pthread",
                           "-Wl,-rpath," + csrc + ",-rpath,/opt/rocm/lib"])
    p = tmp_path / "cpp.genes.sf"
    r = subprocess.run([str(exe), str(tmp_path / "columns.tsv"), str(num_mapped), str(p), str(tmp_path / "no_such_dir" / "quant.genes.sf")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"folded {n} rows" in r.stdout, r.stdout + r.stderr
    assert "refused:" in r.stdout and "no_such_dir" in r.stdout, r.stdout
    d_len, d_eff, _, d_cnt = _dev(length, eff, cnt, cnt, gpu)
    t = torch.zeros(n, dtype=torch.float64, device=gpu)
    with torch.cuda.device(gpu):
        _lib.check(_lib.lib().sfgpu_tpm(_lib.ptr(d_cnt), _lib.ptr(d_eff), n, float(num_mapped), _lib.ptr(t), _lib.current_stream_ptr()))
    tgm = _map_for(names, gene_names)
    out = str(tmp_path / "py.genes.sf")
    genes.aggregate_columns(tgm, names, d_len, d_eff, t, d_cnt, out)
    got, want = p.read_bytes(), open(out, "rb").read()
    assert got == want, _first_difference(got, want)
    assert want == _host_file(tmp_path, tgm, names, (d_len, d_eff, t, d_cnt))
