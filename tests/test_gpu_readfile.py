"""The device FASTA / FASTQ parser (sfgpu_reads_parse_host, sailfish_amd/csrc/readtext.hip) against the serial run of the same
contract header (tests/readfile_harness.cpp) in everything it reports -- bases, offsets, name spans, consumed, n_lines, the
error triple -- then the file driver around it (sailfish_amd.readfile.ReadFile, mapper.quantify_files) against the in-memory
path on the bundled sample."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from test_readfile_cpu import (BAD_START, ERR_FORMAT, ERR_RANGE, FASTA, FASTQ, LENGTH_MISMATCH, MISSING_PLUS, OK, TRUNCATED, Harness,
                               build_harness, fasta_text, fastq_text, same, unpack)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return Harness(build_harness(tmp_path_factory.mktemp("rfh")))


def device_parse(gpu, text, final, max_reads=1 << 40, cap_bases=1 << 40, spans=True):
    import torch
    from sailfish_amd import _lib
    text = bytes(text)
    n = len(text)
    max_reads, cap_bases = min(max_reads, n + 1), min(cap_bases, n)
    bases = torch.zeros(max(cap_bases, 16), dtype=torch.uint8, device=gpu)
    off = torch.full((max_reads + 1,), -1, dtype=torch.int64, device=gpu)
    span = torch.zeros(2 * max_reads + 2, dtype=torch.int64, device=gpu) if spans else None
    res = _lib.ReadsResult()
    with torch.cuda.device(gpu):
        rc = _lib.lib().sfgpu_reads_parse_host(text, n, int(final), max_reads, _lib.ptr(bases), cap_bases, _lib.ptr(off), _lib.ptr(span),
                                               C.byref(res), _lib.current_stream_ptr())
    assert res.ms_copy >= 0 and res.ms_kernels >= 0
    sp = span.cpu().numpy().view(np.uint64) if spans else np.zeros(2 * max_reads + 2, np.uint64)
    return unpack(rc, res, text, bases.cpu().numpy(), off.cpu().numpy(), sp)


def check(gpu, harness, text, final, max_reads=1 << 40, cap_bases=1 << 40):
    n = len(text)
    want = harness.parse(text, final, min(max_reads, n + 1), min(cap_bases, n))
    got = device_parse(gpu, text, final, max_reads, cap_bases)
    same(got, want, (text[:200], final, max_reads, cap_bases))
    return got


def fastq_with_total(rng, total, **kw):
    """reads of the straddling lengths, the last one sized so that the bases sum to `total`"""
    lens = [0, 1, 15, 16, 17, 31, 33, 300] * 4
    lens = lens + [total - sum(lens) - 1000, 1000]
    assert min(lens) >= 0
    return fastq_text(rng, len(lens), lens=lens, **kw)


SHAPES = {
    "fastq_straddle": lambda rng: fastq_text(rng, 24, lens=[0, 1, 15, 16, 17, 31, 33, 300] * 3),
    "fastq_4095": lambda rng: fastq_with_total(rng, 4095),
    "fastq_4096": lambda rng: fastq_with_total(rng, 4096),
    "fastq_4097": lambda rng: fastq_with_total(rng, 4097),
    "fastq_10000": lambda rng: fastq_text(rng, 5, lens=[7, 10000, 0, 150, 33]),
    "fastq_crlf": lambda rng: fastq_text(rng, 24, lens=[0, 1, 15, 16, 17, 31, 33, 300] * 3, crlf=True),
    "fastq_no_final_newline": lambda rng: fastq_text(rng, 9, lens=[150] * 8 + [17], final_newline=False),
    "fastq_crlf_no_final_newline": lambda rng: fastq_text(rng, 9, lens=[16] * 9, crlf=True, final_newline=False),
    "fasta_wrap_1": lambda rng: fasta_text(rng, 6, lens=[0, 1, 33, 300, 16, 0], width=1, blanks=True),
    "fasta_wrap_60": lambda rng: fasta_text(rng, 7, lens=[59, 60, 61, 0, 4097, 120, 0], width=60, blanks=True),
    "fasta_wrap_61": lambda rng: fasta_text(rng, 6, lens=[61, 122, 10000, 0, 60, 0], width=61),
    "fasta_crlf": lambda rng: fasta_text(rng, 6, lens=[61, 122, 1000, 0, 60, 0], width=60, crlf=True, blanks=True),
    "fasta_no_final_newline": lambda rng: fasta_text(rng, 5, lens=[61, 0, 4096, 17, 31], width=60, final_newline=False),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_device_parse_equals_the_harness(gpu, harness, shape):
    """every shape whole and cut short, final and not, with and without the record and base limits; the whole final text gives
    the sequences it was rendered from (the last FASTA records of several shapes are empty: a header-only last record)"""
    rng = np.random.default_rng(sorted(SHAPES).index(shape))
    text, seqs, names = SHAPES[shape](rng)
    got = check(gpu, harness, text, 1)
    assert got["rc"] == OK and got["seqs"] == seqs and got["names"] == names and got["consumed"] == len(text)
    if shape.startswith("fastq"):
        assert any(ln[:1] == b"@" for ln in text.split(b"\n")[3::4]) and any(ln[:1] == b"+" for ln in text.split(b"\n")[3::4])
    check(gpu, harness, text, 0)
    for cut in (len(text) - 1, len(text) - 2, len(text) // 2, 5):
        for final in (0, 1):
            check(gpu, harness, text[:cut], final)
    total = sum(len(s) for s in seqs)
    for max_reads, cap in ((1, 1 << 40), (3, 1 << 40), (1 << 40, total - 1), (1 << 40, total // 2), (len(seqs) - 1, total // 2)):
        r = check(gpu, harness, text, 1, max_reads, cap)
        assert r["rc"] in (OK, ERR_RANGE) and len(r["seqs"]) <= max_reads and sum(len(s) for s in r["seqs"]) <= cap
    # without name spans the rest is the same
    r = device_parse(gpu, text, 1, spans=False)
    assert r["seqs"] == seqs and r["consumed"] == len(text)


@pytest.mark.gpu
def test_texts_without_records(gpu, harness):
    for text in (b"", b"\n", b"\r\n\n\n", b">", b">\n", b"@", b">t", b">\n>\n>"):
        for final in (0, 1):
            check(gpu, harness, text, final)


@pytest.mark.gpu
def test_capacity(gpu, harness):
    text, seqs, _ = fastq_text(np.random.default_rng(3), 6, lens=[40, 20, 0, 30, 16, 5])
    r = check(gpu, harness, text, 1, cap_bases=61)
    assert r["rc"] == OK and r["seqs"] == seqs[:3] and r["consumed"] == text.index(b"@r3")
    assert check(gpu, harness, text, 1, cap_bases=39)["rc"] == ERR_RANGE
    assert check(gpu, harness, text, 0, cap_bases=40)["seqs"] == seqs[:1]
    ftext, fseqs, _ = fasta_text(np.random.default_rng(4), 4, lens=[100, 0, 61, 7], width=60)
    assert check(gpu, harness, ftext, 1, cap_bases=100)["seqs"] == fseqs[:2]
    assert check(gpu, harness, ftext, 1, cap_bases=99)["rc"] == ERR_RANGE
    from sailfish_amd import _lib
    assert _lib.lib().sfgpu_reads_parse_host(b"x", (1 << 30) + 1, 1, 1, None, 0, None, None, C.byref(_lib.ReadsResult()), None) == ERR_RANGE


@pytest.mark.gpu
def test_errors_name_the_first_bad_record(gpu, harness):
    rng = np.random.default_rng(5)
    text, seqs, _ = fastq_text(rng, 1200, lens=rng.integers(1, 40, 1200))
    lines = text.split(b"\n")

    def broken(*edits):
        ls = list(lines)
        for i, new in edits:
            ls[i] = new
        return b"\n".join(ls)
    cases = [(b"ACGT\n@r\nA\n+\nI\n", (BAD_START, 0, 0)),
             (broken((2, b"-")), (MISSING_PLUS, 0, 2)),
             (broken((4 * 77 + 2, b"")), (MISSING_PLUS, 77, 4 * 77 + 2)),
             (broken((3, lines[3] + b"I")), (LENGTH_MISMATCH, 0, 3)),
             (broken((4 * 1000 + 3, lines[4 * 1000 + 3][:-1])), (LENGTH_MISMATCH, 1000, 4 * 1000 + 3)),
             (broken((4 * 500, b"r500")), (BAD_START, 500, 4 * 500)),
             (broken((4 * 1100 + 2, b"-"), (4 * 1000 + 1, lines[4 * 1000 + 1] + b"A"), (4 * 1150, b"x")), (LENGTH_MISMATCH, 1000, 4 * 1000 + 3)),
             (broken((4 * 9, b"x"), (4 * 9 + 2, b"x"), (4 * 9 + 3, b"")), (BAD_START, 9, 4 * 9))]
    for bad, err in cases:
        for final in (0, 1):
            for max_reads in (1 << 40, 1):
                r = check(gpu, harness, bad, final, max_reads)
                assert r["rc"] == ERR_FORMAT and r["error"] == err and r["seqs"] == [] and r["consumed"] == 0
    cut = b"\n".join(lines[:4 * 700 + 2])                 # the last record stops behind its sequence
    assert len(check(gpu, harness, cut, 0)["seqs"]) == 700
    r = check(gpu, harness, cut, 1)
    assert r["rc"] == ERR_FORMAT and r["error"] == (TRUNCATED, 700, 4 * 700 + 2) and r["seqs"] == []


@pytest.mark.gpu
def test_error_behind_reused_staging_slots(gpu, harness):
    """a text of three staged sub-chunks (4 MiB each: the first pinned slot is collected and taken again) whose last sub-chunk
    holds a record without its '+'; the same text unbroken parses whole"""
    rng = np.random.default_rng(6)
    rec, seq, name = fastq_text(rng, 1, lens=[1001])
    reps = (8 << 20) // len(rec) + 3                      # the last record lies wholly behind byte 8 MiB
    text = rec * reps
    assert 8 << 20 < len(text) - len(rec) and len(text) < (8 << 20) + (1 << 16)
    lines = text.split(b"\n")
    bad_line = 4 * (reps - 1) + 2
    assert lines[bad_line] == b"+" + name[0]
    lines[bad_line] = b""
    r = check(gpu, harness, b"\n".join(lines), 1)
    assert r["rc"] == ERR_FORMAT and r["error"] == (MISSING_PLUS, reps - 1, bad_line) and r["seqs"] == [] and r["consumed"] == 0
    r = check(gpu, harness, text, 1)
    assert r["rc"] == OK and r["seqs"] == seq * reps and r["names"] == name * reps and r["consumed"] == len(text)


def _texts_for_carry():
    rng = np.random.default_rng(8)
    yield fastq_text(rng, 40, lens=[0, 1, 15, 16, 17, 31, 33, 300, 150, 70] * 4)
    yield fastq_text(rng, 20, lens=[33, 300] * 10, crlf=True, final_newline=False)
    yield fasta_text(rng, 12, lens=[61, 0, 500, 17, 31, 0, 1, 120, 60, 59, 300, 0], width=60, blanks=True)
    yield fasta_text(rng, 5, lens=[10, 700, 0, 3, 0], width=61, final_newline=False)


@pytest.mark.gpu
def test_read_file_blocks_and_batches_equal_one_shot(gpu, tmp_path):
    """ReadFile with blocks far smaller than a record (a 300-base read against 64-byte blocks: "present more bytes") and batches
    of 1, 3 and 1000 records = the one-shot result = pack_sequences of the truth, byte for byte"""
    import torch
    from sailfish_amd import mapper, readfile
    for k, (text, seqs, names) in enumerate(_texts_for_carry()):
        path = tmp_path / f"t{k}.txt"
        path.write_bytes(text)
        want_b, want_o = mapper.pack_sequences(seqs)
        with readfile.ReadFile(path, gpu) as rf:
            b, o = rf.read(1 << 40)
            assert rf.stats["calls"] == 1 and rf.format == (FASTQ if text[:1] == b"@" else FASTA)
        assert torch.equal(b.cpu(), want_b) and torch.equal(o.cpu(), want_o)
        for block in (64, 100, 4096):
            for batch in (1, 3, 1000):
                got_b, got_o, got_names = [], [np.zeros(1, np.int64)], []
                with readfile.ReadFile(path, gpu, block_bytes=block, names=True) as rf:
                    while True:
                        b, o = rf.read(batch)
                        n = o.numel() - 1
                        if n == 0:
                            break
                        assert n == batch or len(got_names) + n == len(seqs)
                        o = o.cpu().numpy()
                        assert o[0] == 0 and b.numel() >= o[-1]
                        got_b.append(b.cpu().numpy()[: o[-1]]); got_o.append(o[1:] + got_o[-1][-1]); got_names += rf.last_names
                    if block == 64:
                        assert rf.stats["bytes_parsed"] > len(text) and rf._carry.buf.size > 64        # blocks were grown
                assert np.array_equal(np.concatenate(got_b), want_b.numpy()) and np.array_equal(np.concatenate(got_o), want_o.numpy())
                assert got_names == names
    names_t, (b, o) = readfile.read_transcripts(path, gpu, block_bytes=100)
    assert names_t == [nm.decode() for nm in names] and torch.equal(o.cpu(), want_o)


@pytest.mark.gpu
def test_read_file_reports_the_record_of_an_error(gpu, tmp_path):
    from sailfish_amd import readfile
    text, seqs, _ = fastq_text(np.random.default_rng(9), 50, lens=[30] * 50)
    lines = text.split(b"\n")
    lines[4 * 41 + 3] += b"I"
    path = tmp_path / "bad.fastq"
    path.write_bytes(b"\n".join(lines))
    with readfile.ReadFile(path, gpu, block_bytes=512) as rf:
        with pytest.raises(ValueError, match=r"bad\.fastq: record 41 .*differ in length"):
            for _ in range(50):
                rf.read(7)
    (tmp_path / "none.txt").write_bytes(b"hello\n")
    with pytest.raises(ValueError, match="record 0"):
        readfile.ReadFile(tmp_path / "none.txt", gpu).read(1)


# ---- end to end on the bundled sample ---------------------------------------------------------------------------------------

def _sample():
    d = np.load(os.path.join(GOLD, "sample_data_reads.npz"))
    n, L = len(d["truth"]), int(d["read_len"])

    def unpack2(p):
        b = np.unpackbits(p).reshape(-1, 2)
        return np.frombuffer(b"ACGT", np.uint8)[(b[:, 0] * 2 + b[:, 1])[: n * L]].reshape(n, L)
    seqs = [bytes(d["seq"][d["seq_off"][t]:d["seq_off"][t + 1]]) for t in range(len(d["names"]))]
    return [str(x) for x in d["names"]], seqs, [bytes(r) for r in unpack2(d["mate1_2bit"])], [bytes(r) for r in unpack2(d["mate2_2bit"])]


def _render(tmp_path, names, seqs, r1, r2, n_reads=None):
    rng = np.random.default_rng(21)
    fa = tmp_path / "transcripts.fasta"
    with open(fa, "wb") as f:
        for nm, s in zip(names, seqs):
            f.write(b">" + nm.encode() + b" len=%d\n" % len(s))
            for a in range(0, len(s), 60):
                f.write(s[a:a + 60] + b"\n")
    paths = [fa]
    led = 0
    for mate, reads in ((1, r1), (2, r2)):
        p = tmp_path / f"reads_{mate}.fastq"
        with open(p, "wb") as f:
            for i, r in enumerate(reads[:n_reads]):
                q = bytearray(rng.integers(33, 127, len(r), dtype=np.uint8).tobytes())
                if i % 97 == 0:
                    q[0] = ord("@"); led += 1
                f.write(b"@read%d/%d\n" % (i, mate) + r + b"\n+\n" + bytes(q) + b"\n")
        paths.append(p)
    assert led > 10
    return paths


@pytest.mark.gpu
def test_sample_files_give_the_committed_hit_records(gpu, tmp_path):
    import sailfish_amd as sf
    from sailfish_amd import readfile
    from oracle import oracle as O
    names, seqs, r1, r2 = _sample()
    fa, f1, f2 = _render(tmp_path, names, seqs, r1, r2)
    got_names, packed = readfile.read_transcripts(fa, gpu)
    assert got_names == names
    idx = sf.mapper.QuasiIndex(packed, device=gpu)
    assert idx.M == len(names) and np.array_equal(idx.ref_len.cpu().numpy(), [len(s) for s in seqs])
    with readfile.ReadFile(f1, gpu, block_bytes=1 << 18) as a, readfile.ReadFile(f2, gpu, block_bytes=1 << 18) as b:
        m1, m2 = a.read(1 << 40), b.read(1 << 40)
        assert a.stats["calls"] > 2
    for seed_len, fixture in ((None, "sample_data_hits_scan.npz"), (0, "sample_data_hits.npz")):
        gold = np.load(os.path.join(GOLD, fixture))
        if seed_len is not None:
            idx.set_scan(seed_len)
        hits, off = sf.mapper.hits_to_numpy(*idx.map_reads(m1, m2))
        assert np.array_equal(off, gold["offsets"]) and hits.tobytes() == gold["hits"].view(O.HIT_DTYPE).tobytes(), fixture


@pytest.mark.gpu
def test_quantify_files_writes_the_quant_sf_of_the_in_memory_path(gpu, tmp_path):
    import sailfish_amd as sf
    names, seqs, r1, r2 = _sample()
    fa, f1, f2 = _render(tmp_path, names, seqs, r1, r2)
    opts = dict(batch_reads=3000, cmd_options={"libType": "IU"}, device=gpu)
    rc, exp = sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / "mem"), sf.SailfishOpts(numFragSamples=5000), **opts)
    assert rc == 0 and exp.numMappedFragments() == 10000
    want = (tmp_path / "mem" / "quant.sf").read_bytes()
    rc, exp = sf.mapper.quantify_files(fa, f1, f2, "IU", str(tmp_path / "files"), sf.SailfishOpts(numFragSamples=5000), **opts)
    assert rc == 0 and exp.numMappedFragments() == 10000
    assert (tmp_path / "files" / "quant.sf").read_bytes() == want
    gz = []
    for p in (fa, f1, f2):
        gz.append(str(p) + ".gz")
        with gzip.open(gz[-1], "wb", compresslevel=1) as f:
            f.write(p.read_bytes())
    rc, exp = sf.mapper.quantify_files(*gz, "IU", str(tmp_path / "gz"), sf.SailfishOpts(numFragSamples=5000), **opts)
    assert rc == 0 and (tmp_path / "gz" / "quant.sf").read_bytes() == want
    # mate files of unequal length
    short = tmp_path / "short_2.fastq"
    short.write_bytes(b"\n".join(f2.read_bytes().split(b"\n")[:4 * 9000]) + b"\n")
    with pytest.raises(ValueError, match="same number of records"):
        sf.mapper.quantify_files(fa, f1, short, "IU", str(tmp_path / "short"), sf.SailfishOpts(numFragSamples=5000), **opts)
