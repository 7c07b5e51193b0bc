"""The --geneMap file read on the device (sfgpu_gmap_*, sailfish_amd/csrc/genemap.hip; genes.DeviceGeneMap) against the host readers
that are its contract, genes.TranscriptGeneMap.from_gtf / .from_file: exact equality of transcript_names, t2g and gene_names over
the corpus of tests/gmap_corpus.py (the one tests/test_gmap_cpu.py judges the serial rules with), block by block, through the
tie groups and long lines the kernels treat specially, the host fallback, the name join, quantify(..., gene_map=...) and the C++
adaptor."""
import gzip
import os
import subprocess

import numpy as np
import pytest
import torch

import gmap_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_map(path, key="gene_id"):
    from sailfish_amd.genes import TranscriptGeneMap
    return TranscriptGeneMap.from_gtf(str(path), key) if str(path).endswith(".gtf") else TranscriptGeneMap.from_file(str(path))


def lists(m):
    return dict(transcript_names=m.transcript_names, t2g=[int(x) for x in m.t2g], gene_names=m.gene_names)


def device_map(path, key="gene_id", gpu="cuda", **kw):
    from sailfish_amd.genes import DeviceGeneMap
    with DeviceGeneMap.from_path(str(path), key, device=gpu, **kw) as d:
        return lists(d.to_host()), d.stats


def check(path, key, gpu, reader="device", **kw):
    got, stats = device_map(path, key, gpu, **kw)
    want = lists(host_map(path, key))
    assert stats["reader"] == reader, stats
    for k in ("transcript_names", "t2g", "gene_names"):
        assert got[k] == want[k], (k, key)
    return got, stats


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gmap")
    out = {}
    for name, text in [("corner.gtf", corpus.corner_gtf()), ("corner.tsv", corpus.corner_tsv())] + \
                      [(f"random{s}.gtf", corpus.random_gtf(s)) for s in range(5)] + [(f"random{s}.tsv", corpus.random_tsv(s)) for s in range(5)]:
        (d / name).write_bytes(text)
        out[name] = d / name
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("key", corpus.KEYS)
def test_corpus_against_the_host_readers(built, gpu, files, key):
    for name in ["corner.gtf"] + [f"random{s}.gtf" for s in range(5)]:
        _, stats = check(files[name], key, gpu)
        assert stats["n_lines"] == files[name].read_bytes().count(b"\n") + (not files[name].read_bytes().endswith(b"\n"))
    if key == "gene_id":
        for name in ["corner.tsv"] + [f"random{s}.tsv" for s in range(5)]:
            check(files[name], key, gpu)


@pytest.mark.gpu
def test_keys_no_field_can_have(built, gpu, files):
    for key in ("exon_number", "gene_id\x0b", "", "a;b", "gene_id "):
        check(files["corner.gtf"], key, gpu)


@pytest.mark.gpu
def test_small_blocks_against_one_block(built, gpu, files):
    """the smallest block_bytes the call accepts: lines straddle blocks (the carrier grows the text until a line ends in it) and a
    transcript's records spread over many calls"""
    from sailfish_amd.genes import DeviceGeneMap
    with pytest.raises(ValueError):
        DeviceGeneMap.from_path(str(files["corner.gtf"]), block_bytes=DeviceGeneMap.MIN_BLOCK - 1, device=gpu)
    for name in ("corner.gtf", "corner.tsv"):
        one, s1 = device_map(files[name], "gene_id", gpu)
        small, s2 = check(files[name], "gene_id", gpu, block_bytes=DeviceGeneMap.MIN_BLOCK)
        assert small == one and s1["calls"] == 1 and s2["calls"] > 5 and s2["n_lines"] == s1["n_lines"]
    # the kernels at every block length: a cut inside a name, between '\r' and '\n', behind the last line
    text = corpus.random_gtf(2, 300)
    p = files["corner.gtf"].parent / "cuts.gtf"
    p.write_bytes(text)
    want = lists(host_map(p))
    for block in (64, 65, 77, 127, 128, 1000, 4096):
        assert device_map(p, "gene_id", gpu, block_bytes=block)[0] == want, block


@pytest.mark.gpu
def test_tie_groups_wider_than_a_workgroup(built, gpu, tmp_path):
    """3 000 records of one id of which only the last carries the key (the first-with-key search spans a run far wider than a
    workgroup), then 3 000 distinct ids that share their first 16 bytes (the third sort round separates them)"""
    L = [corpus.gtf_line(f'transcript_id "one_id"; exon_number {i};') for i in range(2999)]
    L.append(corpus.gtf_line('transcript_id "one_id"; gene_id "late_gene"; gene_name "late_name";'))
    order = np.random.default_rng(5).permutation(3000)
    L += [corpus.gtf_line(f'gene_id "G{i % 7}"; transcript_id "SAMEHEADSAMEHEAD{i:05d}"; gene_name "SAMEHEADSAMEHEADN{i % 11}";') for i in order]
    p = tmp_path / "ties.gtf"
    p.write_text("".join(L))
    for key in ("gene_id", "gene_name"):
        got, stats = check(p, key, gpu)
        assert len(got["transcript_names"]) == 3001 and got["gene_names"][got["t2g"][got["transcript_names"].index("one_id")]].startswith("late_")
        assert stats["sort_rounds"] == 3
    # the same shapes in two-column form: equal names keep file order
    q = tmp_path / "ties.tsv"
    q.write_text("".join(f"one_id g{i}\n" for i in range(3000)) + "".join(f"SAMEHEADSAMEHEAD{i:05d} G{i % 7}\n" for i in order))
    got, _ = check(q, "gene_id", gpu)
    assert got["t2g"][got["transcript_names"].index("one_id"):][:3000] == list(range(3000))


@pytest.mark.gpu
def test_lines_longer_than_one_step(built, gpu, tmp_path):
    """attribute columns of 1 100 and 5 000 bytes (a wavefront reads 1 KB per step) with the keys in the last field; a long
    leading column as well, so that the tab count is carried across steps"""
    L = []
    for n, lead in ((1100, ""), (5000, ""), (1100, "c" * 1500), (5000, "c" * 2100)):
        filler = ""
        i = 0
        while len(filler) < n:
            filler += f'note{i} "filler value {i}"; '
            i += 1
        L.append(f"chr1{lead}\tS\texon\t1\t2\t.\t+\t.\t" + filler + f'gene_id "g{n}{len(lead)}"; transcript_id "t{n}{len(lead)}"\n')
        L.append(f"chr1{lead}\tS\texon\t1\t2\t.\t+\t.\t" + f'transcript_id "u{n}{len(lead)}"; ' + filler + f'gene_id "h{n}{len(lead)}";\tcol10\n')
    p = tmp_path / "long.gtf"
    p.write_text("".join(L))
    got, _ = check(p, "gene_id", gpu)
    assert len(got["transcript_names"]) == 8 and len(got["gene_names"]) == 8
    check(p, "gene_id", gpu, block_bytes=64)


@pytest.mark.gpu
def test_fallback_to_the_host_reader(built, gpu, tmp_path):
    """one non-ASCII byte: the host reader's map, uploaded; no exception"""
    p = tmp_path / "utf8.gtf"
    p.write_bytes(corpus.random_gtf(4, 200) + corpus.gtf_line('transcript_id "café"; gene_id "gé";').encode("utf-8"))
    got, stats = check(p, "gene_id", gpu, reader="host")
    assert "café" in got["transcript_names"] and "0x80" in stats["reason"]
    q = tmp_path / "utf8.tsv"
    q.write_bytes("a g\ncafé gé\nb g\n".encode("utf-8"))
    check(q, "gene_id", gpu, reader="host")
    for name, is_gtf, text, flag in corpus.flagged():
        if flag in (corpus.LONE_CR, corpus.LONG_NAME):
            f = tmp_path / (name + (".gtf" if is_gtf else ".tsv"))
            f.write_bytes(text)
            check(f, "gene_id", gpu, reader="host")
    # what was uploaded (sfgpu_gmap_from_host), read back from the device and used there: not the cached host object
    from sailfish_amd import genes
    host = host_map(p)
    rows = ["café", "caf", "cafz", "T0001", "", "ENST0500", "cafés", "gé", "zzzz", "é", "cafê", "gé"]        # six inside, then past the last name
    with genes.DeviceGeneMap.from_path(str(p), device=gpu) as d:
        assert d.stats["reader"] == "host"
        d._host = None
        assert lists(d.to_host()) == lists(host)
        for names in (rows[:6], rows):
            ids, n_past = d.lookup(_pair(names, gpu))
            want, _ = host.gene_ids_of(names)
            inside = np.array([n <= host.transcript_names[-1] for n in names])
            assert n_past == int((~inside).sum()) == len(names) - 6
            assert ids.cpu().numpy().view(np.uint32)[inside].tolist() == want[inside].tolist()
            cols = _columns(len(names), gpu, seed=3)
            a, b = str(tmp_path / "dev.sf"), str(tmp_path / "host.sf")
            genes.aggregate_columns(d, names, *cols, a)
            genes.aggregate_columns(host, names, *cols, b)
            assert open(a, "rb").read() == open(b, "rb").read()
    # a flagged byte in the first of many small blocks: the block loop ends there, the host reader takes the file
    big = tmp_path / "first.gtf"
    big.write_bytes(corpus.gtf_line('transcript_id "café"; gene_id "gé";').encode("utf-8") + corpus.random_gtf(3))
    _, stats = check(big, "gene_id", gpu, reader="host", block_bytes=64)
    assert stats["calls"] <= 2 and stats["bytes_parsed"] < 1000, stats
    # gzip-compressed and flagged: the host reader gets the inflated text
    z = tmp_path / "utf8z.gtf.gz"
    z.write_bytes(gzip.compress(p.read_bytes()))
    got_z, stats = device_map(z, "gene_id", gpu)
    assert got_z == got and stats["reader"] == "host"


def _columns(n, gpu, seed=0):
    rng = np.random.default_rng(seed)
    length = torch.from_numpy(rng.integers(200, 5000, n).astype(np.int32)).to(gpu)
    eff = torch.from_numpy(rng.uniform(100, 4000, n)).to(gpu)
    tpm = torch.from_numpy(rng.uniform(0, 50, n) * (rng.random(n) < 0.8)).to(gpu)
    nr = torch.from_numpy(rng.uniform(0, 900, n) * (rng.random(n) < 0.8)).to(gpu)
    return length, eff, tpm, nr


def _pair(names, gpu):
    from sailfish_amd import quantfile
    b, o = quantfile.names_blob(names)
    return (torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(gpu), torch.from_numpy(o.view(np.int64).copy()).to(gpu))


@pytest.mark.gpu
def test_lookup_and_aggregate_columns(built, gpu, tmp_path):
    from sailfish_amd import genes
    p = tmp_path / "m.tsv"
    p.write_text("".join(f"{t} {g}\n" for t, g in [("bb", "g1"), ("dd", "g2"), ("dd2", "g1"), ("ff", "g3"), ("mm", "zz9"), ("mm", "g2")]))
    host = host_map(p)
    with genes.DeviceGeneMap.from_path(str(p), device=gpu) as d:
        inside = ["a", "", "aa", "bb", "dd", "dd2", "mm", "bc", "c", "dd1", "e", "ff", "bb", "k", "ddd"]      # below, equal, between
        ids, n_past = d.lookup(_pair(inside, gpu))
        want, table = host.gene_ids_of(inside)
        assert n_past == 0 and table == host.gene_names
        assert ids.cpu().numpy().view(np.uint32).tolist() == want.tolist()
        past = inside + ["zz9", "zz", "zz", "q", "zz9", "n", "mn"]             # past the last: a map gene's name, new names, duplicates
        ids, n_past = d.lookup(_pair(past, gpu))
        got = ids.cpu().numpy().view(np.uint32)
        assert n_past == 7 and got[:len(inside)].tolist() == want.tolist() and (got[len(inside):] == 0xFFFFFFFF).all()
        for names in (inside, past):
            cols = _columns(len(names), gpu, seed=len(names))
            a, b, c = str(tmp_path / "dev.sf"), str(tmp_path / "host.sf"), str(tmp_path / "blob.sf")
            genes.aggregate_columns(d, names, *cols, a)
            genes.aggregate_columns(host, names, *cols, b)
            genes.aggregate_columns(d, _pair(names, gpu), *cols, c)
            assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
            assert open(a, "rb").read().count(b"\n") > 4
    # an empty map: every transcript is its own gene
    e = tmp_path / "empty.tsv"
    e.write_text("\n")
    with genes.DeviceGeneMap.from_path(str(e), device=gpu) as d:
        assert d.num_transcripts() == 0 and d.lookup(_pair(["x", "y"], gpu))[1] == 2
        cols = _columns(2, gpu)
        genes.aggregate_columns(d, ["x", "y"], *cols, str(tmp_path / "e1.sf"))
        genes.aggregate_columns(host_map(e), ["x", "y"], *cols, str(tmp_path / "e2.sf"))
        assert open(tmp_path / "e1.sf", "rb").read() == open(tmp_path / "e2.sf", "rb").read()


@pytest.mark.gpu
def test_lookup_on_the_corpus_equals_gene_ids_of(built, gpu, files):
    from sailfish_amd import genes
    host = host_map(files["corner.gtf"])
    rng = np.random.default_rng(9)
    names = [n for n in host.transcript_names] + [n[:-1] for n in host.transcript_names if len(n) > 1] + [n + "x" for n in host.transcript_names[:-1]]
    names = [n for n in names if n < host.transcript_names[-1] or n == host.transcript_names[-1]]
    names = [names[i] for i in rng.permutation(len(names))]
    with genes.DeviceGeneMap.from_path(str(files["corner.gtf"]), device=gpu) as d:
        ids, n_past = d.lookup(_pair(names, gpu))
    assert n_past == 0 and ids.cpu().numpy().view(np.uint32).tolist() == host.gene_ids_of(names)[0].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["gtf", "gtf.gz", "gtf.bgzf", "gtf.gz_device", "tsv"])
def test_quantify_end_to_end(built, gpu, tmp_path, form):
    """quantify(..., gene_map=...) on the small workload of tests/test_gpu_genes.py with a shuffled GTF that carries exon records:
    quant.genes.sf is byte for byte what the host reader and the host aggregation give"""
    import sailfish_amd as sf
    from sailfish_amd import genes, gzfile
    from test_filter import _txome
    from test_gpu_genes import _toy_batches
    rng = np.random.default_rng(41)
    M, R = 300, 60_000
    seq, so, rl = _txome(rng, M, lo=400, hi=3000)
    names = [f"tx{i:04d}" for i in range(M)]
    if form == "tsv":
        plain = tmp_path / "map.tsv"
        plain.write_text("".join(f"{n} g{i // 3}\n" for i, n in enumerate(names[:-4])))          # the last four: their own genes
    else:
        lines = []
        for i, n in enumerate(names):
            if i % 3 == 0:
                lines.append(corpus.gtf_line(f'gene_id "G{i // 3}"; gene_name "N{i // 3}";', feature="gene"))
            lines.append(corpus.gtf_line(f'gene_id "G{i // 3}"; transcript_id "{n}"; gene_name "N{i // 3}";', feature="transcript"))
            lines += [corpus.gtf_line(f'transcript_id "{n}"; exon_number {e}; gene_id "G{i // 3}";', feature="exon") for e in range(i % 4)]
        lines = [lines[i] for i in rng.permutation(len(lines))]
        plain = tmp_path / "map.gtf"
        plain.write_text("".join(lines))
    gm = plain
    if form in ("gtf.gz", "gtf.gz_device"):
        gm = tmp_path / "map.gtf.gz"
        gm.write_bytes(gzip.compress(plain.read_bytes()))
    elif form == "gtf.bgzf":
        gm = tmp_path / "mapb.gtf.gz"
        gzfile.write_bgzf(str(gm), plain.read_bytes())
    sopt = sf.SailfishOpts(numFragSamples=2000)
    out = str(tmp_path / "out")
    if form == "gtf.gz_device":                  # "auto" keeps ordinary gzip on the host; the device route is asked for by name
        _, stats = check_gz(gm, plain, gpu, inflate="device")
        assert stats["inflate"] == "device" and stats["reader"] == "device"
        return
    rc, exp = sf.quant.quantify(names, rl, _toy_batches(rng, rl, M, R), "IU", out, sopt, seq=seq, seq_off=so, allow_orphans=True,
                                gene_map=str(gm), seed=3, device=gpu)
    assert rc == 0
    got = open(os.path.join(out, "quant.genes.sf"), "rb").read()
    os.rename(os.path.join(out, "quant.genes.sf"), os.path.join(out, "device.genes.sf"))
    want = open(genes.aggregate_estimates_to_gene_level(host_map(plain), os.path.join(out, "quant.sf")), "rb").read()
    assert got == want
    assert got.count(b"\n") == 1 + {"tsv": (M - 4 + 2) // 3 + 4}.get(form, M // 3)
    if form != "tsv":
        _, stats = check_gz(gm, plain, gpu)
        assert stats["inflate"] == {"gtf": None, "gtf.gz": "host", "gtf.bgzf": "device"}[form]


def check_gz(path, plain, gpu, **kw):
    got, stats = device_map(path, "gene_id", gpu, **kw)
    assert got == lists(host_map(plain)) and stats["reader"] == "device"
    return got, stats


@pytest.mark.gpu
def test_compressed_maps_in_small_blocks(built, gpu, files, tmp_path):
    """BGZF members and gzip chunks that end inside lines: the device carriers keep the tail of the inflated text"""
    from sailfish_amd import gzfile
    text = files["random1.gtf"].read_bytes()
    b = tmp_path / "r.gtf.gz"
    gzfile.write_bgzf(str(b), text, member_bytes=700)
    check_gz(b, files["random1.gtf"], gpu, block_bytes=4096)
    z = tmp_path / "z.gtf.gz"
    z.write_bytes(gzip.compress(text))
    check_gz(z, files["random1.gtf"], gpu, inflate="device", block_bytes=8192)
    check_gz(z, files["random1.gtf"], gpu, block_bytes=100)
    t = tmp_path / "t.tsv.gz"
    t.write_bytes(gzip.compress(files["corner.tsv"].read_bytes()))
    got, _ = device_map(t, "gene_id", gpu)
    assert got == lists(host_map(files["corner.tsv"]))


@pytest.mark.gpu
def test_handle_states_and_limits(built, gpu):
    import ctypes as C
    from sailfish_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    with torch.cuda.device(gpu):
        assert L.sfgpu_gmap_open(C.byref(h), 7, b"k", 1) == _lib.ERR_INVALID
        _lib.check(L.sfgpu_gmap_open(C.byref(h), 0, b"gene_id", 7))
        res, fin, past = _lib.GmapAddResult(), _lib.GmapResult(), C.c_uint64()
        text = np.frombuffer(b"no newline in this block", np.uint8)
        assert L.sfgpu_gmap_add_text_host(h, _lib.ptr(text), text.size, 0, C.byref(res), None) == _lib.ERR_RANGE and res.consumed == 0
        assert L.sfgpu_gmap_lookup(h, None, None, 0, None, C.byref(past), None) == _lib.ERR_STATE
        assert L.sfgpu_gmap_export(h, None, None, None, None, None, None) == _lib.ERR_STATE
        line = np.frombuffer(corpus.gtf_line('transcript_id "t"; gene_id "g";').encode() + b"tail", np.uint8)
        _lib.check(L.sfgpu_gmap_add_text_host(h, _lib.ptr(line), line.size, 0, C.byref(res), None))
        assert (res.n_lines, res.n_records, res.consumed, res.needs_host) == (1, 1, line.size - 4, 0)
        bad = np.frombuffer(b"x\0y\n", np.uint8)
        _lib.check(L.sfgpu_gmap_add_text_host(h, _lib.ptr(bad), bad.size, 1, C.byref(res), None))
        assert res.needs_host == 2 and L.sfgpu_gmap_finish(h, C.byref(fin), None) == _lib.ERR_STATE and fin.needs_host == 2
        L.sfgpu_gmap_close(h)
        _lib.check(L.sfgpu_gmap_open(C.byref(h), 1, None, 0))
        _lib.check(L.sfgpu_gmap_finish(h, C.byref(fin), None))
        assert (fin.n_transcripts, fin.n_genes) == (0, 0)
        assert L.sfgpu_gmap_add_text_host(h, _lib.ptr(line), line.size, 1, C.byref(res), None) == _lib.ERR_STATE
        L.sfgpu_gmap_close(h)


@pytest.mark.gpu
def test_cpp_adaptor(built, gpu, tmp_path, files):
    """readTranscriptToGeneMap and the handle overload of aggregateEstimatesToGeneLevel (include/sfgpu_sailfish.hpp), compiled with
    g++ and run: the file holds the bytes of the Python path, also when transcripts lie past the map's last name"""
    from sailfish_amd import _lib, genes
    host = host_map(files["corner.gtf"])
    names = [n for n in host.transcript_names if " " not in n and n][:40] + ["zzz_own_gene", "gp0", "zzz_own_gene2"]
    n = len(names)
    rng = np.random.default_rng(12)
    length = rng.integers(200, 5000, n).astype(np.uint32)
    eff = rng.uniform(100, 4000, n)
    cnt = rng.uniform(0, 900, n) * (rng.random(n) < 0.8)
    num_mapped = 1_234_567
    bits = lambda x: int(np.float64(x).view(np.uint64))
    with open(tmp_path / "columns.tsv", "w") as f:
        for i in range(n):
            f.write(f"{names[i]}\t{int(length[i])}\t{bits(eff[i]):016x}\t{bits(cnt[i]):016x}\n")
    exe = tmp_path / "gmap_host_test"
    csrc = os.path.join(ROOT, "sailfish_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"),
                           "-I", "/opt/rocm/include", os.path.join(ROOT, "tests", "gmap_host_test.cpp"), "-o", str(exe),
                           "-L", csrc, "-lsfgpu", "-L", "/opt/rocm/lib", "-lamdhip64", "-pthread",
                           "-Wl,-rpath," + csrc + ",-rpath,/opt/rocm/lib"])
    d_len = torch.from_numpy(length.view(np.int32).copy()).to(gpu)
    d_eff, d_cnt = torch.from_numpy(eff).to(gpu), torch.from_numpy(cnt).to(gpu)
    t = torch.zeros(n, dtype=torch.float64, device=gpu)
    with torch.cuda.device(gpu):
        _lib.check(_lib.lib().sfgpu_tpm(_lib.ptr(d_cnt), _lib.ptr(d_eff), n, float(num_mapped), _lib.ptr(t), _lib.current_stream_ptr()))
    for use, block in ((names, "100"), (names[:40], "33554432")):
        with open(tmp_path / "columns.tsv", "w") as f:
            for i in range(len(use)):
                f.write(f"{use[i]}\t{int(length[i])}\t{bits(eff[i]):016x}\t{bits(cnt[i]):016x}\n")
        p = tmp_path / "cpp.genes.sf"
        r = subprocess.run([str(exe), str(tmp_path / "columns.tsv"), str(num_mapped), str(files["corner.gtf"]), "gene_id", str(p), block],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"folded {len(use)} rows" in r.stdout and "refused:" in r.stdout, r.stdout + r.stderr
        assert f"mapped {len(host.transcript_names)} transcripts to {len(host.gene_names)} genes" in r.stdout
        k = len(use)
        if k < n:
            with torch.cuda.device(gpu):
                _lib.check(_lib.lib().sfgpu_tpm(_lib.ptr(d_cnt[:k].contiguous()), _lib.ptr(d_eff[:k].contiguous()), k, float(num_mapped), _lib.ptr(t), _lib.current_stream_ptr()))
        out = str(tmp_path / "py.genes.sf")
        genes.aggregate_columns(host, use, d_len[:k].contiguous(), d_eff[:k].contiguous(), t[:k].contiguous(), d_cnt[:k].contiguous(), out)
        assert p.read_bytes() == open(out, "rb").read()
