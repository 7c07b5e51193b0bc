"""Reads written as FASTA / FASTQ from the device (sfgpu_reads_write_text / _bgzf, sailfish_amd/csrc/readtext_write.hip with the
rules of csrc/readwfmt.h; readfile.ReadDeviceWriter; write_unmapped= of mapper.quantify_reads / quantify_files).  The expected
bytes are always readfile.reads_text_host's -- the per-record host loop -- over the host copy of the same batch.

Every input array is uploaded between 64 sentinel bytes on either side and compared with its upload after the call; the result
struct lies between sentinels too.  (The chunk buffers are the library's own: what the sink receives is checked byte for byte.)"""
import ctypes as C
import gzip
import os

import numpy as np
import pytest
import torch

import readwrite_corpus as corpus

PAD = 64
DEFAULT_CHUNK = 32 << 20


class Upload:
    """a corpus case on the device: every array between sentinels, off its 16-byte boundary when the case is misaligned"""

    def __init__(self, case, gpu):
        self.case, self.n = case, len(case["seqs"])
        self.host, self.dev, self.lead = {}, {}, {}
        for k, a in corpus.arrays(case).items():
            if k == "n" or a is None:
                continue
            raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            lead = PAD + ((3 if a.itemsize == 1 else 8) if case["misaligned"] else 0)
            buf = np.full(lead + raw.size + PAD, 0xA5, np.uint8)
            buf[lead:lead + raw.size] = raw
            self.host[k], self.lead[k], self.dev[k] = buf, lead, torch.from_numpy(buf).to(gpu)

    def ptr(self, k):
        return C.c_void_p(self.dev[k].data_ptr() + self.lead[k]) if k in self.dev else None

    def view(self, k, dtype=torch.uint8):
        """the array as a tensor (a view into the padded upload), or None"""
        if k not in self.dev:
            return None
        t = self.dev[k][self.lead[k]:self.dev[k].numel() - PAD]
        return t if dtype == torch.uint8 else t.view(dtype)

    def untouched(self):
        return all(np.array_equal(self.dev[k].cpu().numpy(), self.host[k]) for k in self.dev)


def _write(up, chunk_bytes=0, null_sink=False, refuse_at=None, n_reads=None):
    """sfgpu_reads_write_text over an upload with a sink that keeps every chunk -> (status, result dict, chunks)"""
    from sailfish_amd import _lib
    chunks = []

    def sink(addr, n, _user):
        chunks.append(C.string_at(addr, n))
        return 1 if refuse_at is not None and len(chunks) == refuse_at else 0

    size = C.sizeof(_lib.ReadWriteResult)
    frame = (C.c_uint8 * (size + 2 * PAD))(*([0xA5] * (size + 2 * PAD)))
    res = _lib.ReadWriteResult.from_buffer(frame, PAD)
    with torch.cuda.device(up.dev["off"].device):
        rc = _lib.lib().sfgpu_reads_write_text(up.ptr("bases"), up.ptr("off"), up.n if n_reads is None else n_reads, up.ptr("qual"), up.ptr("names"),
                                               up.ptr("name_off"), up.case["base"], up.ptr("select"), chunk_bytes,
                                               _lib.TEXT_SINK(0) if null_sink else _lib.TEXT_SINK(sink), None, C.byref(res), _lib.current_stream_ptr())
    assert bytes(frame[:PAD]) == b"\xa5" * PAD and bytes(frame[PAD + size:]) == b"\xa5" * PAD
    return rc, res.as_dict(), chunks


def _record_lengths(case):
    return [corpus.record_len(len(n), len(s), q is not None) for n, s, q in corpus.selected(case)]


def _greedy_chunks(unit_len, chunk_bytes):
    n, cur = 0, 0
    for L in unit_len:
        if cur and cur + L > chunk_bytes:
            n, cur = n + 1, 0
        cur += int(L)
    return n + (1 if cur else 0)


def _first_difference(got, want):
    n = min(len(got), len(want))
    d = np.flatnonzero(np.frombuffer(got, np.uint8, n) != np.frombuffer(want, np.uint8, n))
    i = int(d[0]) if len(d) else n
    return f"lengths {len(got)} / {len(want)}, first difference at byte {i}: got {got[max(i - 20, 0):i + 40]!r}, want {want[max(i - 20, 0):i + 40]!r}"


@pytest.fixture(scope="module")
def good():
    """[(case, expected text, record lengths)] of the corpus cases that can be written, computed once"""
    return [(c, corpus.expected(c), _record_lengths(c)) for c in corpus.cases() if c["error"] is None]


def _same_at(up, want, lens, chunk_bytes):
    case = up.case
    rc, res, chunks = _write(up, chunk_bytes)
    assert rc == 0, (case["label"], chunk_bytes)
    got = b"".join(chunks)
    assert got == want, (case["label"], chunk_bytes, _first_difference(got, want))
    assert (res["n_reads"], res["n_selected"], res["n_bytes"], res["max_record_bytes"], res["error_kind"]) == \
        (len(case["seqs"]), len(lens), len(want), max(lens, default=0), 0), case["label"]
    assert res["n_chunks"] == len(chunks) == _greedy_chunks(lens, chunk_bytes or DEFAULT_CHUNK), (case["label"], chunk_bytes)
    assert all(len(c) <= (chunk_bytes or DEFAULT_CHUNK) for c in chunks)
    assert set(np.cumsum([len(c) for c in chunks]).tolist()) <= set(np.cumsum(lens).tolist())      # chunks end between records


@pytest.mark.gpu
def test_corpus_text_is_the_statement_at_every_chunk_size(gpu, good):
    seen_none = 0
    for case, want, lens in good:
        up = Upload(case, gpu)
        for chunk_bytes in (max(max(lens, default=16), 16), 4096, 4097, 0):
            if chunk_bytes and chunk_bytes < max(lens, default=0):
                continue                                   # (a record longer than 4096: test_contract has that)
            _same_at(up, want, lens, chunk_bytes)
        assert up.untouched(), case["label"]
        if not lens:                                       # nothing selected: the sink is never called (n_chunks == len(chunks) == 0 above)
            assert want == b"" and case["seqs"]
            seen_none += 1
    assert seen_none >= 2


@pytest.mark.gpu
def test_random_batches(gpu):
    for i in range(corpus.N_RANDOM):
        case = corpus.random_case(i)
        want, lens = corpus.expected(case), _record_lengths(case)
        up = Upload(case, gpu)
        _same_at(up, want, lens, 0)
        if max(lens, default=0) <= 4096:
            _same_at(up, want, lens, 4096)
        assert up.untouched(), case["label"]


@pytest.mark.gpu
def test_records_that_cannot_be_written(gpu):
    from sailfish_amd import _lib
    bad = [c for c in corpus.cases() if c["error"] is not None]
    assert len(bad) >= 20
    for case in bad:
        up = Upload(case, gpu)
        for null_sink in (False, True):
            rc, res, chunks = _write(up, 0, null_sink=null_sink)
            assert rc == _lib.ERR_FORMAT and not chunks and res["n_chunks"] == 0, case["label"]
            assert (res["error_record"], res["error_kind"]) == case["error"], case["label"]
            assert f"record {case['error'][0]}:".encode() in _lib.lib().sfgpu_last_error()
        assert up.untouched()


@pytest.mark.gpu
def test_contract(gpu, good):
    from sailfish_amd import _lib
    by = {c["label"]: (c, w, l) for c, w, l in good}
    case, want, lens = by["runs.fastq"]
    up = Upload(case, gpu)
    # sizing only
    rc, res, chunks = _write(up, 0, null_sink=True)
    assert rc == 0 and not chunks and (res["n_bytes"], res["n_chunks"], res["max_record_bytes"]) == (len(want), 0, max(lens))
    # no reads
    rc, res, chunks = _write(up, 0, n_reads=0)
    assert rc == 0 and not chunks and (res["n_bytes"], res["n_selected"], res["n_chunks"]) == (0, 0, 0)
    # a record longer than chunk_bytes: nothing is delivered
    for chunk_bytes in (max(lens) - 1, 4096):
        rc, res, chunks = _write(up, chunk_bytes)
        assert rc == _lib.ERR_RANGE and not chunks and res["max_record_bytes"] == max(lens) and res["n_bytes"] == len(want)
    # chunk_bytes outside [16, 2^30]
    for chunk_bytes in (15, (1 << 30) + 1):
        assert _write(up, chunk_bytes)[0] == _lib.ERR_INVALID
    # a sink that refuses the second chunk
    rc, res, chunks = _write(up, max(lens), refuse_at=2)
    assert rc == _lib.ERR_IO and len(chunks) == 2 and b"".join(chunks) == want[:len(chunks[0]) + len(chunks[1])]
    # offsets that decrease; names without offsets; n_reads beyond the layout
    for key in ("off", "name_off"):
        broken = Upload(case, gpu)
        t = broken.view(key, torch.int64)
        t[3] = t[4] + 1
        rc, res, chunks = _write(broken, 0)
        assert rc == _lib.ERR_INVALID and not chunks
    orphan = Upload(case, gpu)
    del orphan.dev["name_off"]
    assert _write(orphan, 0)[0] == _lib.ERR_INVALID
    assert _write(up, 0, n_reads=2 ** 32 - 1)[0] == _lib.ERR_RANGE
    assert up.untouched()


def _cat(cases):
    """the concatenation of batches as one case for the statement: generated names count the records SEEN"""
    seen, parts, recs = 0, [], []
    for c in cases:
        d = dict(c, base=seen)
        parts.append(corpus.expected(d))
        recs += corpus.selected(d)
        seen += len(c["seqs"])
    return b"".join(parts), recs


def _read_back(path, gpu):
    from sailfish_amd import readfile
    with readfile.ReadFile(path, gpu, names="device", quals=True) as f:
        bases, off = f.read(1 << 40)
        nb, no = f.last_names
        b, o, nb, no = bases.cpu().numpy(), off.cpu().numpy(), nb.cpu().numpy(), no.cpu().numpy()
        q = None if f.last_quals is None else f.last_quals.cpu().numpy()
        recs = [(bytes(nb[no[r]:no[r + 1]]), bytes(b[o[r]:o[r + 1]]), None if q is None else bytes(q[o[r]:o[r + 1]])) for r in range(len(o) - 1)]
        return recs, f.inflate


@pytest.mark.gpu
@pytest.mark.parametrize("compress", [False, True], ids=["plain", "bgzf"])
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_writer_over_three_batches(gpu, tmp_path, fmt, compress):
    from sailfish_amd import readfile
    by = {c["label"]: c for c in corpus.cases()}
    batches = [by[f"runs.{fmt}"], by[f"generated_names_9.{fmt}"], by[f"select_sparse.{fmt}"], by[f"misaligned.{fmt}"]]
    want, recs = _cat(batches)
    path = tmp_path / ("u." + fmt + (".gz" if compress else ""))
    ups = [Upload(c, gpu) for c in batches]
    with readfile.ReadDeviceWriter(path, compress=compress, chunk_bytes=1 << 15) as w:
        for up in ups:
            sel = up.view("select")
            n = w.write((up.view("bases"), up.view("off", torch.int64)), quals=up.view("qual"),
                        names=None if up.case["names"] is None else (up.view("names"), up.view("name_off", torch.int64)),
                        select=None if sel is None else sel.view(torch.bool) if up.case["misaligned"] else sel)
            assert n == len(corpus.selected(up.case))
        other = Upload(by[f"select_first.{'fasta' if fmt == 'fastq' else 'fastq'}"], gpu)
        with pytest.raises(ValueError, match="first write fixed the format"):
            w.write((other.view("bases"), other.view("off", torch.int64)), quals=other.view("qual"))
        # a batch that cannot be written names the record counted from the first batch, and writes nothing
        bad = by[f"error_two_records.{fmt}"]
        up_bad = Upload(bad, gpu)
        seen = sum(len(c["seqs"]) for c in batches)
        with pytest.raises(ValueError, match=rf"^record {seen + bad['error'][0]}: the bases hold a line end \(kind 2\)$"):
            w.write((up_bad.view("bases"), up_bad.view("off", torch.int64)), quals=up_bad.view("qual"), names=(up_bad.view("names"), up_bad.view("name_off", torch.int64)))
        stats = w.stats
    assert all(up.untouched() for up in ups)
    raw = path.read_bytes()
    text = gzip.decompress(raw) if compress else raw
    assert text == want, _first_difference(text, want)
    assert (stats["batches"], stats["reads_in"], stats["reads_written"], stats["bytes"], stats["bytes_out"]) == \
        (len(batches), sum(len(c["seqs"]) for c in batches), len(recs), len(want), len(raw))
    assert stats["chunks"] >= len(batches) and set(stats) == {"batches", "reads_in", "reads_written", "bytes", "bytes_out", "chunks", "ms_format", "ms_copy",
                                                              "ms_sink", "ms_encode"}
    if compress:
        assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    back, inflate = _read_back(path, gpu)
    assert inflate == ("device" if compress else None)
    assert back == [(n, s, q) for n, s, q in recs]


@pytest.mark.gpu
def test_writer_without_a_batch(gpu, tmp_path):
    from sailfish_amd import readfile
    with readfile.ReadDeviceWriter(tmp_path / "none.fq") as w:
        pass
    assert (tmp_path / "none.fq").read_bytes() == b""
    with readfile.ReadDeviceWriter(tmp_path / "none.fq.gz", compress=True) as w:
        pass
    assert gzip.decompress((tmp_path / "none.fq.gz").read_bytes()) == b"" and w.stats["bytes_out"] == 28
    with pytest.raises(ValueError, match="closed"):
        w.write((torch.zeros(1, dtype=torch.uint8, device=gpu), torch.zeros(1, dtype=torch.int64, device=gpu)))


# ---- end to end: write_unmapped= ----------------------------------------------------------------------------------------------

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _revcomp(s):
    return s.translate(_COMP)[::-1]


def _mutated_pairs(rng, seqs, n, read_len=70, seed=19, rate=0.3):
    """pairs cut from a transcript, each mate with `rate` substitutions behind an intact seed of `seed` bases"""
    def spoil(read):
        v = bytearray(read)
        for i in rng.choice(np.arange(seed, len(v)), int(round(rate * (len(v) - seed))), replace=False):
            v[i] = rng.choice([c for c in b"ACGT" if c != v[i]])
        return bytes(v)
    out = []
    long = [s for s in seqs if len(s) >= 400]
    for _ in range(n):
        s = long[int(rng.integers(0, len(long)))]
        p = int(rng.integers(0, len(s) - 300))
        out.append((spoil(s[p:p + read_len]), spoil(_revcomp(s[p + 200 - read_len:p + 200]))))
    return out


def _write_fastq(path, mate, names, reads, rng):
    quals = [rng.integers(33, 127, len(r), dtype=np.uint8).tobytes() for r in reads]
    with open(path, "wb") as f:
        for nm, r, q in zip(names, reads, quals):
            f.write(b"@" + nm + b"/%d a comment:%d\n" % (mate, len(r)) + r + b"\n+\n" + q + b"\n")
    return {nm + b"/%d" % mate: (r, q) for nm, r, q in zip(names, reads, quals)}


def _records(path):
    lines = open(path, "rb").read().split(b"\n")
    assert lines[-1] == b"" and len(lines) % 4 == 1 and all(h.startswith(b"@") for h in lines[0:-1:4]) and all(p == b"+" for p in lines[2::4])
    return [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]


def _qnames(sam_path, flag):
    return [l.split(b"\t")[0] for l in open(sam_path, "rb").read().split(b"\n") if l and not l.startswith(b"@") and l.split(b"\t")[1] == flag]


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """the bundled sample's transcripts, its first 300 pairs, 100 pairs of random 70-mers, 4 pairs shorter than the seed and 20 pairs
    with 30 % substitutions behind an intact seed, shuffled -> dict(fa, kinds, files with and without the mutated pairs)"""
    import mapper_corpus
    from oracle import mapper_oracle as MO
    from test_gpu_readfile import _render, _sample
    tmp = tmp_path_factory.mktemp("unmapped")
    names, seqs, r1, r2 = _sample()
    fa = _render(tmp, names, seqs, r1, r2, n_reads=500)[0]          # (its read files are not used)
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda n: acgt[rng.integers(0, 4, n)].tobytes()
    pairs = [("true", a, b) for a, b in zip(r1[:300], r2[:300])] + [("random", rnd(70), rnd(70)) for _ in range(100)] + \
            [("short", rnd(n), rnd(n + 1)) for n in (1, 7, 17, 18)] + [("mutated", a, b) for a, b in _mutated_pairs(rng, seqs, 20)]
    # what the mapper's contract says of the pairs that are not the sample's own: the host statement of the scan mode
    sindex = (mapper_corpus.vec_table(seqs, 31), [MO._codes(s) for s in seqs], 31)
    extra = [p for p in pairs if p[0] != "true"]
    _, off = MO.scan_reads(sindex, [p[1] for p in extra], [p[2] for p in extra])
    placed = np.diff(off.astype(np.int64)) > 0
    assert not placed[:104].any()                          # the random and the short pairs: no record
    order = rng.permutation(len(pairs))
    pairs = [pairs[i] for i in order]
    qn = [b"frag%d_%s" % (i, k.encode()) for i, (k, _, _) in enumerate(pairs)]
    placed_names = {qn[j] for j, i in enumerate(order) if i >= 300 and placed[i - 300]}
    assert len(placed_names) >= 10 and all(n.endswith(b"mutated") for n in placed_names)
    out = dict(fa=fa, placed=placed_names)
    for tag, keep in (("all", lambda k: True), ("plain", lambda k: k != "mutated")):
        sub = [(n, p) for n, p in zip(qn, pairs) if keep(p[0])]
        p1, p2 = tmp / f"{tag}_1.fastq", tmp / f"{tag}_2.fastq"
        rec = _write_fastq(p1, 1, [n for n, _ in sub], [p[1] for _, p in sub], rng)
        rec.update(_write_fastq(p2, 2, [n for n, _ in sub], [p[2] for _, p in sub], rng))
        out[tag] = dict(p1=p1, p2=p2, records=rec, names=[n for n, _ in sub], kinds=[p[0] for _, p in sub])
    return out


def _run(library, tag, out, gpu, **kw):
    import sailfish_amd as sf
    lib = library[tag]
    rc, exp = sf.mapper.quantify_files(library["fa"], lib["p1"], lib["p2"], "IU", str(out), sf.SailfishOpts(numFragSamples=5000), batch_reads=128,
                                       cmd_options={"libType": "IU"}, device=gpu, write_mappings=str(out) + ".sam", **kw)
    return rc, exp


@pytest.mark.gpu
def test_unmapped_reads_of_a_paired_run(gpu, library, tmp_path):
    from sailfish_amd import readfile
    lib = library["plain"]
    u1, u2 = tmp_path / "u_1.fastq", tmp_path / "u_2.fastq"
    log = []
    import sailfish_amd as sf
    rc, exp = sf.mapper.quantify_files(library["fa"], lib["p1"], lib["p2"], "IU", str(tmp_path / "with"), sf.SailfishOpts(numFragSamples=5000, jointLog=lambda lvl, m: log.append(m)),
                                       batch_reads=128, cmd_options={"libType": "IU"}, device=gpu, write_mappings=str(tmp_path / "with.sam"), write_unmapped=(u1, u2))
    assert rc == 0
    rc0, exp0 = _run(library, "plain", tmp_path / "without", gpu)
    assert rc0 == 0
    # neither the estimates nor the mappings file depend on the option (QUAL stays '*': mappings_oriented is off)
    assert (tmp_path / "with" / "quant.sf").read_bytes() == (tmp_path / "without" / "quant.sf").read_bytes()
    sam = (tmp_path / "with.sam").read_bytes()
    assert sam == (tmp_path / "without.sam").read_bytes()
    assert all(l.split(b"\t")[10] == b"*" for l in sam.split(b"\n") if l and not l.startswith(b"@"))
    # the unmapped files: the reads of the 77 lines, in order, each the input record of that name
    rec1, rec2 = _records(u1), _records(u2)
    unmapped = _qnames(tmp_path / "with.sam", b"77")
    assert [n for n, _, _ in rec1] == unmapped and len(rec1) == len(rec2)
    stem = lambda n: n[:-2]
    kinds = dict(zip(lib["names"], lib["kinds"]))
    assert {n for n in lib["names"] if kinds[n] != "true"} <= {stem(n) for n in unmapped}          # the random and the short pairs
    batches = {lib["names"].index(stem(n)) // 128 for n in unmapped}
    assert len(rec1) >= 104 and len(batches) > 1
    for recs, mate in ((rec1, b"/1"), (rec2, b"/2")):
        for n, s, q in recs:
            assert n.endswith(mate) and (s, q) == lib["records"][n]
    assert [stem(n) for n, _, _ in rec1] == [stem(n) for n, _, _ in rec2]
    with readfile.ReadFile(u1, gpu, names="device") as a, readfile.ReadFile(u2, gpu, names="device") as b:
        a.read(1 << 40), b.read(1 << 40)
        assert readfile.mate_names_match(a.last_names, b.last_names) is None
    assert exp.unmapped_stats == dict(reads=len(lib["names"]), unmapped=len(rec1), bytes=[os.path.getsize(u1), os.path.getsize(u2)])
    assert sum("unmapped reads:" in m for m in log) == 1 and not hasattr(exp0, "unmapped_stats")
    # on their own the unmapped files map nothing: every read comes out again, and the mappings file holds 77 / 141 lines only
    v1, v2 = tmp_path / "v_1.fastq", tmp_path / "v_2.fastq"
    sf.mapper.quantify_files(library["fa"], u1, u2, "IU", str(tmp_path / "again"), sf.SailfishOpts(numFragSamples=5000), batch_reads=128,
                             cmd_options={"libType": "IU"}, device=gpu, write_mappings=str(tmp_path / "again.sam"), write_unmapped=(v1, v2))
    assert v1.read_bytes() == u1.read_bytes() and v2.read_bytes() == u2.read_bytes()
    flags = {l.split(b"\t")[1] for l in (tmp_path / "again.sam").read_bytes().split(b"\n") if l and not l.startswith(b"@")}
    assert flags == {b"77", b"141"}


@pytest.mark.gpu
def test_unmapped_reads_after_validation(gpu, library, tmp_path):
    """a read whose records the validation pass drops is unmapped: the selector is taken from the batch handed to quant.quantify"""
    lib = library["all"]
    placed = library["placed"]
    rc, _ = _run(library, "all", tmp_path / "loose", gpu, write_unmapped=(tmp_path / "l_1.fq", tmp_path / "l_2.fq"))
    assert rc == 0
    loose = {n[:-2] for n, _, _ in _records(tmp_path / "l_1.fq")}
    assert not placed & loose                              # without validation the seeds give them records
    u1, u2 = tmp_path / "s_1.fq.gz", tmp_path / "s_2.fq.gz"
    rc, exp = _run(library, "all", tmp_path / "strict", gpu, validate_mappings=True, min_identity=0.9, write_unmapped=(u1, u2), unmapped_compress=True)
    assert rc == 0
    rec1 = [l for l in gzip.decompress(u1.read_bytes()).split(b"\n")[0::4] if l]
    rec2 = [l for l in gzip.decompress(u2.read_bytes()).split(b"\n")[0::4] if l]
    strict = {l[1:-2] for l in rec1}
    assert placed <= strict and [l[:-2] for l in rec1] == [l[:-2] for l in rec2]
    assert [l[1:] for l in rec1] == _qnames(str(tmp_path / "strict") + ".sam", b"77")
    st = exp.verify_stats
    assert st["reads_in"] - st["reads_out"] >= len(placed) and st["failed_identity"] >= len(placed)
    assert exp.unmapped_stats["unmapped"] == len(rec1) >= len(loose) + len(placed)


@pytest.mark.gpu
def test_unmapped_reads_of_quantify_reads(gpu, library, tmp_path):
    """from the in-memory driver the names are r<index>, counted over the whole run; FASTA without qualities, single end"""
    import sailfish_amd as sf
    from test_gpu_readfile import _sample
    names, seqs, _, _ = _sample()
    lib = library["plain"]
    reads = [lib["records"][n + b"/1"][0] for n in lib["names"]]
    u = tmp_path / "u.fa"
    rc, exp = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "q"), sf.SailfishOpts(), batch_reads=100, device=gpu,
                                       cmd_options={"libType": "U"}, write_mappings=str(tmp_path / "q.sam"), write_unmapped=u)
    assert rc == 0
    lines = u.read_bytes().split(b"\n")
    got = list(zip(lines[0:-1:2], lines[1::2]))
    want = [b"r%d" % i for i, k in enumerate(lib["kinds"]) if k != "true"]
    assert [h[1:] for h, _ in got] == _qnames(tmp_path / "q.sam", b"4") and set(want) <= {h[1:] for h, _ in got}
    assert all(h.startswith(b">r") and s == reads[int(h[2:])] for h, s in got) and max(int(h[2:]) for h, _ in got) >= 100
    assert exp.unmapped_stats["unmapped"] == len(got) and exp.unmapped_stats["reads"] == len(reads)
    quals = [lib["records"][n + b"/1"][1] for n in lib["names"]]
    uq = tmp_path / "u.fq"
    rc, _ = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "qq"), sf.SailfishOpts(), batch_reads=100, device=gpu,
                                     cmd_options={"libType": "U"}, quals1=quals, write_unmapped=uq)
    assert rc == 0 and (tmp_path / "qq" / "quant.sf").read_bytes() == (tmp_path / "q" / "quant.sf").read_bytes()
    assert _records(uq) == [(h[1:], s, quals[int(h[2:])]) for h, s in got]


@pytest.mark.gpu
def test_option_checks_come_before_the_index(gpu, tmp_path, monkeypatch):
    import sailfish_amd as sf

    def no_index(*a, **k):
        raise AssertionError("an index was built")
    monkeypatch.setattr(sf.mapper, "QuasiIndex", no_index)
    fa = tmp_path / "missing.fa"                           # (never opened: the checks come first)
    for reads2, kw in (("b.fq", dict(write_unmapped="u.fq")), (None, dict(write_unmapped=("u1.fq", "u2.fq"))), ("b.fq", dict(write_unmapped=("u1.fq",))),
                       ("b.fq", dict(write_unmapped=("u1.fq", 3))), (None, dict(unmapped_compress=True)), ("b.fq", dict(unmapped_compress=True))):
        with pytest.raises(ValueError, match="write_unmapped"):
            sf.mapper.quantify_files(fa, "a.fq", reads2, "IU" if reads2 else "U", str(tmp_path / "o"), device=gpu, **kw)
        with pytest.raises(ValueError, match="write_unmapped"):
            sf.mapper.quantify_reads(["t"], [b"ACGT" * 20], [b"ACGT"], None if reads2 is None else [b"ACGT"], "IU" if reads2 else "U", str(tmp_path / "o"), device=gpu, **kw)
    assert not os.path.exists(tmp_path / "o") and not os.path.exists("u.fq") and not os.path.exists("u1.fq")
