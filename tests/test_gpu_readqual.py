"""The FASTQ parser with the qualities kept (sfgpu_reads_parse_host_q / _device_q, sailfish_amd/csrc/readtext.hip;
readfile.ReadFile(quals=True).last_quals): the qualities are the quality lines split out in Python, at the bases' offsets, through
every carrier; everything else is what the entries without d_qual give for the same bytes."""
import ctypes as C
import gzip

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENS = [0, 1, 15, 16, 17, 31, 33, 150, 151, 100, 0, 0, 75, 300, 48, 49] * 20         # 320 records; runs of empty reads; 16-byte edges
QUALS = np.arange(33, 127, dtype=np.uint8)


def fastq(seed=0, crlf=False, final_newline=True, lens=LENS):
    """-> (text, [bases], [qualities]); every fifth quality line begins with '@', every seventh with '+'"""
    rng = np.random.default_rng(300 + seed)
    eol = b"\r\n" if crlf else b"\n"
    seqs, quals, out = [], [], []
    for i, n in enumerate(lens):
        s = rng.choice(np.frombuffer(b"ACGTN", np.uint8), n).tobytes()
        q = bytearray(rng.choice(QUALS, n).tobytes())
        if n and i % 5 == 0:
            q[0] = ord("@")
        if n and i % 7 == 0:
            q[0] = ord("+")
        seqs.append(s); quals.append(bytes(q))
        out.append(b"@read.%d some comment" % i + eol + s + eol + b"+" + (b"read.%d" % i if i % 3 == 0 else b"") + eol + bytes(q) + eol)
    text = b"".join(out)
    return (text if final_newline else text[:-len(eol)]), seqs, quals


def split_quals(text):
    """the quality lines, as the issue states them: line 4r + 3 without its line end or the '\\r' of a CRLF end"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in lines[3::4]]


def parse(gpu, text, final, max_reads, cap_bases, entry, quals):
    """one call of `entry` ("host" / "device", with d_qual when quals) -> dict of every output"""
    from sailfish_amd import _lib
    L, n = _lib.lib(), len(text)
    bases = torch.zeros(max(cap_bases, 16), dtype=torch.uint8, device=gpu)
    qual = torch.full((max(cap_bases, 16),), 7, dtype=torch.uint8, device=gpu)
    off = torch.full((max_reads + 1,), -1, dtype=torch.int64, device=gpu)
    span = torch.zeros(2 * max_reads + 2, dtype=torch.int64, device=gpu)
    res = _lib.ReadsResult()
    with torch.cuda.device(gpu):
        if entry == "host":
            head = (text, n, int(final), max_reads, _lib.ptr(bases))
        else:
            cap_text = (n + 1 + 15) // 16 * 16 + 16
            d_text = torch.zeros(cap_text, dtype=torch.uint8, device=gpu)
            d_text[:n] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(gpu)
            head = (_lib.ptr(d_text), n, cap_text, int(final), max_reads, _lib.ptr(bases))
        tail = (cap_bases, _lib.ptr(off), _lib.ptr(span), C.byref(res), _lib.current_stream_ptr())
        fn = getattr(L, f"sfgpu_reads_parse_{entry}" + ("_q" if quals else ""))
        rc = fn(*head, *((_lib.ptr(qual),) if quals else ()), *tail)
    R, B = int(res.n_reads), int(res.n_bases)
    return dict(rc=rc, n_reads=R, n_bases=B, consumed=int(res.consumed), n_lines=int(res.n_lines), format=int(res.format),
                error=(int(res.error_kind), int(res.error_record), int(res.error_line)), bases=bases.cpu().numpy()[:B].tobytes(),
                off=off.cpu().numpy()[:R + 1].tolist(), span=span.cpu().numpy()[:2 * R].tolist(), qual=qual.cpu().numpy())


@pytest.mark.parametrize("entry", ["host", "device"])
def test_entries_with_and_without_qualities(gpu, entry):
    """whole texts and cuts at max_reads / cap_bases: the _q entry equals the old one in everything, and adds the qualities"""
    for crlf, final_newline in ((False, True), (True, True), (False, False), (True, False)):
        text, seqs, quals = fastq(1, crlf, final_newline)
        assert split_quals(text) == quals and any(q.startswith(b"@") for q in quals) and any(q.startswith(b"+") for q in quals)
        total = sum(len(s) for s in seqs)
        for final, max_reads, cap_bases in ((1, len(seqs) + 5, len(text)), (0, len(seqs) + 5, len(text)), (1, 37, len(text)), (1, len(seqs), total // 3),
                                            (1, 11, 16), (0, 3, 0)):
            old = parse(gpu, text, final, max_reads, cap_bases, entry, False)
            new = parse(gpu, text, final, max_reads, cap_bases, entry, True)
            for k in old:
                if k != "qual":
                    assert old[k] == new[k], (k, crlf, final_newline, final, max_reads, cap_bases)
            assert (old["qual"] == 7).all()                    # (the old entry has no d_qual to write)
            if new["rc"]:
                assert new["n_reads"] == 0
                continue
            R, B = new["n_reads"], new["n_bases"]
            assert new["bases"] == b"".join(seqs[:R]) and new["qual"][:B].tobytes() == b"".join(quals[:R])
            assert (new["qual"][B:] == 7).all()                # nothing behind the qualities
            if (final, max_reads) == (1, len(seqs) + 5):
                assert R == len(seqs)
            if max_reads == 37:
                assert R == 37
            if cap_bases == total // 3:
                assert 0 < R < len(seqs) and B <= cap_bases < B + len(seqs[R])


def test_errors_emit_nothing_and_fasta_writes_nothing(gpu):
    from sailfish_amd import _lib
    text, seqs, quals = fastq(2, lens=LENS[:40])
    lines = text.split(b"\n")
    lines[4 * 9 + 3] += b"I"                                   # record 9: quality and sequence differ in length
    bad = b"\n".join(lines)
    for entry in ("host", "device"):
        old, new = (parse(gpu, bad, 1, 100, len(bad), entry, q) for q in (False, True))
        assert new["rc"] == _lib.ERR_FORMAT and new["error"] == old["error"] == (3, 9, 39) and new["n_reads"] == 0
        assert (new["qual"] == 7).all()
        fa = b"".join(b">t%d\n%s\n" % (i, s) for i, s in enumerate(seqs) if s)
        old, new = (parse(gpu, fa, 1, 100, len(fa), entry, q) for q in (False, True))
        assert new["rc"] == 0 and new["format"] == 1 and new["bases"] == old["bases"] == b"".join(seqs) and new["off"] == old["off"]
        assert (new["qual"] == 7).all()
        assert parse(gpu, b"", 1, 4, 16, entry, True)["rc"] == 0


@pytest.mark.parametrize("carrier", ["plain", "bgzf", "gzip-device", "gzip-host"])
def test_read_file_keeps_the_qualities(gpu, tmp_path, carrier):
    """block ends inside quality lines (block_bytes far below the file), reads() that end inside blocks"""
    from sailfish_amd import gzfile, readfile
    for crlf, final_newline in ((False, True), (True, False)):
        text, seqs, quals = fastq(3, crlf, final_newline)
        path = tmp_path / f"reads.{carrier}.{int(crlf)}.fastq"
        if carrier == "plain":
            path.write_bytes(text)
        elif carrier == "bgzf":
            gzfile.write_bgzf(str(path), text, member_bytes=3000)
        else:
            path.write_bytes(gzip.compress(text))
        block = 1500 if carrier in ("plain", "gzip-host") else 20000      # (of the compressed bytes, where the device inflates)
        inflate = {"gzip-device": "device", "gzip-host": "host"}.get(carrier, "auto")
        plain = readfile.ReadFile(str(path), gpu, block_bytes=block, inflate=inflate)
        with readfile.ReadFile(str(path), gpu, block_bytes=block, names=True, inflate=inflate, quals=True) as f:
            assert f.inflate == {"plain": None, "bgzf": "device", "gzip-device": "device", "gzip-host": "host"}[carrier]
            r = 0
            for max_reads in (70, 1, 130, 1000):
                bases, off = f.read(max_reads)
                b0, o0 = plain.read(max_reads)
                n = off.numel() - 1
                assert n == min(max_reads, len(seqs) - r) and torch.equal(off, o0) and torch.equal(bases[:int(off[-1])], b0[:int(o0[-1])])
                assert off.cpu().tolist() == np.concatenate([[0], np.cumsum([len(s) for s in seqs[r:r + n]])]).tolist()
                assert f.last_quals.dtype == torch.uint8 and f.last_quals.device == bases.device
                assert f.last_quals.cpu().numpy().tobytes() == b"".join(quals[r:r + n])
                assert bases.cpu().numpy()[:int(off[-1])].tobytes() == b"".join(seqs[r:r + n])
                assert f.last_names == [b"read.%d" % i for i in range(r, r + n)]
                r += n
            assert r == len(seqs) and f.stats["calls"] > (4 if block == 1500 else 3)
            bases, off = f.read(10)
            assert off.numel() == 1 and f.last_quals is None
        assert plain.last_quals is None
        plain.close()


def test_fasta_file_has_no_qualities(gpu, tmp_path):
    from sailfish_amd import readfile
    _, seqs, _ = fastq(4, lens=LENS[:50])
    path = tmp_path / "reads.fasta"
    path.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
    with readfile.ReadFile(str(path), gpu, block_bytes=600, quals=True) as f:
        bases, off = f.read(30)
        assert off.numel() == 31 and f.last_quals is None
