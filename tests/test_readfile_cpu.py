"""The record contract of the device FASTA / FASTQ parser (sailfish_amd/csrc/readfmt.h, used by readtext.hip) compiled as plain
C++ with g++ (tests/readfile_harness.cpp, a shared object; nothing but libstdc++ is linked) and judged by a short pure-Python
restatement that works record by record where the harness and the kernels work line by line and with scans.  The carry-over
that sailfish_amd.readfile.BlockCarry keeps around the stateless parser is driven with the harness as its parser.  No GPU."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_RANGE, ERR_FORMAT = 0, 5, 8
FASTA, FASTQ = 1, 2
BAD_START, MISSING_PLUS, LENGTH_MISMATCH, TRUNCATED = 1, 2, 3, 4
NONE = 2 ** 64 - 1


# ---- the harness -----------------------------------------------------------------------------------------------------------

def build_harness(dirpath):
    so = os.path.join(str(dirpath), "libreadfile_harness.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(ROOT, "sailfish_amd", "csrc"), os.path.join(ROOT, "tests", "readfile_harness.cpp"), "-o", so])
    return so


class Result(C.Structure):             # sfgpu_reads_result
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("consumed", C.c_uint64), ("n_lines", C.c_uint64),
                ("error_record", C.c_uint64), ("error_line", C.c_uint64), ("format", C.c_int32), ("error_kind", C.c_int32),
                ("ms_copy", C.c_double), ("ms_kernels", C.c_double)]


class Harness:
    def __init__(self, so):
        self.fn = C.CDLL(so).readfile_harness_parse
        self.fn.restype = C.c_int
        self.fn.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(Result)]

    def parse(self, text, final, max_reads=1 << 40, cap_bases=1 << 40):
        """-> dict(rc, format, seqs, names, spans, consumed, n_lines, error=(kind, record, line))"""
        text = bytes(text)
        n = len(text)
        bases = np.zeros(n + 1, np.uint8); off = np.zeros(n + 2, np.int64); span = np.zeros(2 * n + 2, np.uint64)
        res = Result()
        rc = self.fn(text, n, int(final), max_reads, bases.ctypes.data, cap_bases, off.ctypes.data, span.ctypes.data, C.byref(res))
        return unpack(rc, res, text, bases, off, span)


def unpack(rc, res, text, bases, off, span):
    R = int(res.n_reads)
    o = [int(x) for x in off[: R + 1]]
    assert o[0] == 0 and o[-1] == res.n_bases
    sp = [(int(span[2 * r]), int(span[2 * r + 1])) for r in range(R)]
    return dict(rc=rc, format=res.format, seqs=[bytes(bases[o[r]:o[r + 1]]) for r in range(R)], spans=sp,
                names=[text[b:b + l] for b, l in sp], consumed=int(res.consumed), n_lines=int(res.n_lines),
                error=(res.error_kind, int(res.error_record), int(res.error_line)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return Harness(build_harness(tmp_path_factory.mktemp("rfh")))


# ---- the restatement: record by record --------------------------------------------------------------------------------------

def _strip(line):
    return line[:-1] if line.endswith(b"\r") else line


def _name(header):
    nm = header[1:]
    for sep in (b" ", b"\t"):
        nm = nm.split(sep)[0]
    return nm


def restate(text, final, max_reads=1 << 40, cap_bases=1 << 40):
    text = bytes(text)
    n = len(text)
    out = dict(rc=OK, format=0, seqs=[], names=[], spans=[], consumed=0, n_lines=0, error=(0, NONE, NONE))
    if n == 0:
        return out
    out["format"] = {b">": FASTA, b"@": FASTQ}.get(text[:1], 0)
    if not out["format"]:
        if text.strip(b"\r\n") == b"":
            out.update(n_lines=text.count(b"\n") + int(final), consumed=n if final else 0)
        else:
            out.update(rc=ERR_FORMAT, error=(BAD_START, 0, 0))
        return out
    parts = text.split(b"\n")                    # the last one is what follows the last '\n'
    begin = np.concatenate([[0], np.cumsum([len(p) + 1 for p in parts])]).tolist()
    out["n_lines"] = len(parts) - 1 + int(final)
    records = []                                 # (header line index, sequence, index of the first line behind the record)
    if out["format"] == FASTQ:
        lines = parts if final else parts[:-1]
        T = len(lines)
        while T and _strip(lines[T - 1]) == b"":
            T -= 1
        for r in range((T + 3) // 4 if final else T // 4):
            rec = lines[4 * r:4 * r + 4]
            if not rec[0].startswith(b"@"):
                out.update(rc=ERR_FORMAT, error=(BAD_START, r, 4 * r)); return out
            if len(rec) > 2 and not rec[2].startswith(b"+"):
                out.update(rc=ERR_FORMAT, error=(MISSING_PLUS, r, 4 * r + 2)); return out
            if len(rec) > 3 and len(_strip(rec[3])) != len(_strip(rec[1])):
                out.update(rc=ERR_FORMAT, error=(LENGTH_MISMATCH, r, 4 * r + 3)); return out
            if len(rec) < 4:
                out.update(rc=ERR_FORMAT, error=(TRUNCATED, r, len(lines))); return out
            records.append((4 * r, _strip(rec[1]), 4 * r + 4))
    else:
        heads = [i for i, p in enumerate(parts) if p.startswith(b">")]
        for j, h in enumerate(heads):
            nxt = heads[j + 1] if j + 1 < len(heads) else len(parts)
            if nxt == len(parts) and not final:
                break                                # still open
            records.append((h, b"".join(_strip(p) for p in parts[h + 1:nxt]), nxt))
    R, total = 0, 0
    while R < min(len(records), max_reads) and total + len(records[R][1]) <= cap_bases:
        total += len(records[R][1]); R += 1
    if R == 0 and records and max_reads > 0:
        out["rc"] = ERR_RANGE
        return out
    for h, seq, nxt in records[:R]:
        out["seqs"].append(seq)
        out["names"].append(_name(_strip(parts[h])))
        out["spans"].append((begin[h] + 1, len(out["names"][-1])))
    if R:
        out["consumed"] = n if (final and R == len(records)) else begin[records[R - 1][2]]
    return out


def same(a, b, what=""):
    for k in ("rc", "format", "seqs", "names", "spans", "consumed", "n_lines", "error"):
        assert a[k] == b[k], (k, a[k], b[k], what)


def pack(seqs):
    """mapper.pack_sequences without the tensors: the bytes back to back, and the offsets"""
    return b"".join(seqs), np.concatenate([[0], np.cumsum([len(s) for s in seqs], dtype=np.int64)]).astype(np.int64)


# ---- texts ------------------------------------------------------------------------------------------------------------------

def fastq_text(rng, n, max_len=40, crlf=False, final_newline=True, lens=None):
    """-> (text, truth sequences, truth names); qualities are drawn from all printable bytes, so '@' and '+' lead quality lines"""
    eol = b"\r\n" if crlf else b"\n"
    out, seqs, names = [], [], []
    for r in range(n):
        ln = int(lens[r]) if lens is not None else int(rng.integers(0, max_len + 1))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), ln))
        qual = bytearray(rng.integers(33, 127, ln, dtype=np.uint8).tobytes())
        if ln and r % 3 == 0:
            qual[0] = ord("@") if r % 2 else ord("+")
        name = b"r%d" % r
        out += [b"@" + name + (b" extra words" if r % 4 == 1 else b"\tx" if r % 4 == 2 else b""), seq, b"+" + (name if r % 5 == 0 else b""), bytes(qual)]
        seqs.append(seq); names.append(name)
    text = eol.join(out) + eol if out else b""
    if not final_newline and text:
        text = text[:-len(eol)]
    return text, seqs, names


def fasta_text(rng, n, max_len=40, width=60, crlf=False, final_newline=True, blanks=False, lens=None):
    eol = b"\r\n" if crlf else b"\n"
    out, seqs, names = [], [], []
    for r in range(n):
        ln = int(lens[r]) if lens is not None else int(rng.integers(0, max_len + 1))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), ln))
        name = b"t%d.%d" % (r, ln)
        out.append(b">" + name + (b" gene=g%d" % r if r % 2 else b""))
        for a in range(0, ln, width):
            out.append(seq[a:a + width])
            if blanks and (r + a) % 3 == 0:
                out.append(b"")
        seqs.append(seq); names.append(name)
    text = eol.join(out) + eol if out else b""
    if not final_newline and text:
        text = text[:-len(eol)]
    return text, seqs, names


def random_texts(fmt, count=200, seed=0):
    rng = np.random.default_rng(seed + fmt)
    for c in range(count):
        n = int(rng.integers(1, 9))
        crlf, nl = bool(c % 4 == 1), bool(c % 3 != 2)
        if fmt == FASTQ:
            yield fastq_text(rng, n, crlf=crlf, final_newline=nl)
        else:
            yield fasta_text(rng, n, width=int(rng.integers(1, 18)), crlf=crlf, final_newline=nl, blanks=bool(c % 5 == 0))


HAND_MADE = [
    b"", b"\n", b"\r\n\n", b"x", b"\n@r\nA\n+\nI\n",
    b"@r\nACGT\n+\nIIII\n", b"@r\nACGT\n+\nIIII", b"@r\nACGT\n+\nIIII\n\n\n", b"@r\nACGT\n+\nIIII\n\n\n\n\n\n",
    b"@r\n\n+\n\n", b"@r\n\n+\n", b"@r\n\n+", b"@r\n\n", b"@r\nAC\n+\n", b"@r\nAC\n+", b"@r\nAC\n", b"@r\nAC", b"@r", b"@",
    b"@r\nAC\n+\n@+\n@s\nGG\n+s\n+@\n", b"@r\nAC\n+\nII\n@s\nGGG\n+\nII\n", b"@r\nAC\nII\n@s\n", b"@r\nAC\n+\nII\nr2\nAC\n+\nII\n",
    b"@r\r\nAC\r\n+\r\nII\r\n@s x\r\nG\r\n+\r\nI", b"@a b\tc\nA\n+\nI\n@\tb\nA\n+\nI\n@\nA\n+\nI\n",
    b">t\nACGT\n", b">t\nACGT", b">t\n", b">t", b">", b">\n>\n>", b">t\n\n\nAC\n\nGT\n\n", b">t x\nAC\n>u\ty\n>v\nGG\nTT\n>w",
    b">t\r\nAC\r\nGT\r\n>u\r\n\r\nA", b">t\nAC\n>", b">t\nAC\n>u", b">t\nAC\n@x\n+\n",
]


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_harness_links_nothing_else(harness, tmp_path):
    import re
    so = build_harness(tmp_path)
    needed = re.findall(r"NEEDED.*\[(.*?)\]", subprocess.check_output(["readelf", "-d", so], text=True))
    assert needed and all(n.startswith(("libstdc++", "libm.", "libgcc_s", "libc.")) for n in needed), needed


def test_hand_made_cases(harness):
    for text in HAND_MADE:
        for final in (0, 1):
            for max_reads, cap in ((1 << 40, 1 << 40), (1, 1 << 40), (1 << 40, 3), (0, 0)):
                same(harness.parse(text, final, max_reads, cap), restate(text, final, max_reads, cap), (text, final, max_reads, cap))
    # a few of them spelled out, so that the restatement is not the only witness
    r = harness.parse(b"@r\nAC\n+\n@+\n@s\nGG\n+s\n+@\n", 0)
    assert r["rc"] == OK and r["seqs"] == [b"AC", b"GG"] and r["names"] == [b"r", b"s"] and r["consumed"] == 23
    r = harness.parse(b"@r\nACGT\n+\nIIII", 0)
    assert r["rc"] == OK and r["seqs"] == [] and r["consumed"] == 0                    # the fourth line has no '\n' yet
    assert harness.parse(b"@r\nACGT\n+\nIIII", 1)["seqs"] == [b"ACGT"]
    r = harness.parse(b">t x\nAC\n>u\ty\n>v\nGG\nTT\n>w", 0)
    assert r["seqs"] == [b"AC", b"", b"GGTT"] and r["names"] == [b"t", b"u", b"v"] and r["consumed"] == 22
    r = harness.parse(b">t x\nAC\n>u\ty\n>v\nGG\nTT\n>w", 1)
    assert r["seqs"] == [b"AC", b"", b"GGTT", b""] and r["names"][-1] == b"w" and r["consumed"] == 24
    assert harness.parse(b">t\nAC\n>u\nGGG\n", 1, cap_bases=2)["seqs"] == [b"AC"]
    assert harness.parse(b">t\nAC\n>u\nGGG\n", 1, cap_bases=1)["rc"] == ERR_RANGE


@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_random_texts_match_the_restatement(harness, fmt):
    led = 0
    for text, seqs, names in random_texts(fmt):
        got = harness.parse(text, 1)
        same(got, restate(text, 1), text)
        assert got["rc"] == OK and got["seqs"] == seqs and got["names"] == names and got["consumed"] == len(text)
        for final in (0, 1):
            for cut in (len(text) // 3, len(text) - 1):
                for max_reads, cap in ((1 << 40, 1 << 40), (2, 1 << 40), (1 << 40, 50)):
                    same(harness.parse(text[:cut], final, max_reads, cap), restate(text[:cut], final, max_reads, cap), (text[:cut], final))
        if fmt == FASTQ:
            led += sum(1 for ln in text.split(b"\n")[3::4] if ln[:1] in (b"@", b"+"))
    assert fmt == FASTA or led > 50                  # quality lines that begin with '@' / '+' were there


def drive(parse, data, block, max_reads):
    """the whole stream through readfile.BlockCarry in read() calls of max_reads records -> all sequences, in order"""
    from sailfish_amd.readfile import BlockCarry, Parsed
    calls = []

    def one(text, final, want):
        r = parse(text.tobytes(), final, want)
        assert r["rc"] == OK, r
        calls.append((len(text), final, len(r["seqs"])))
        return Parsed(len(r["seqs"]), r["consumed"], r)
    carry = BlockCarry(io.BytesIO(data), block)
    seqs, names = [], []
    while True:
        left, got = max_reads, 0
        while left > 0:
            res = carry.next(one, left)
            if res is None:
                break
            assert 0 < res.n_reads <= left
            seqs += res.payload["seqs"]; names += res.payload["names"]
            left -= res.n_reads; got += res.n_reads
        if got < max_reads:
            break
    assert carry.lo == carry.hi and carry.records == len(seqs)
    return seqs, names, calls


@pytest.mark.parametrize("fmt", [FASTA, FASTQ])
def test_blocks_reassemble_to_the_packed_truth(harness, fmt):
    grew = 0
    for k, (text, seqs, names) in enumerate(random_texts(fmt, count=40, seed=7)):
        want_bases, want_off = pack(seqs)
        for block in (1, 7, 64, max(len(text), 1)):
            for max_reads in (1, 3, 1000):
                got, got_names, calls = drive(harness.parse, text, block, max_reads)
                b, o = pack(got)
                assert b == want_bases and np.array_equal(o, want_off) and got_names == names, (text, block, max_reads)
                grew += any(n > block for n, _, _ in calls)
    assert grew > 40                                 # "present more bytes" was exercised


def test_every_error_kind_at_its_record(harness):
    rng = np.random.default_rng(11)
    text, seqs, _ = fastq_text(rng, 6, lens=[5, 0, 7, 16, 3, 9])
    lines = text.split(b"\n")

    def broken(i, new):
        ls = list(lines); ls[i] = new
        return b"\n".join(ls)
    cases = [(b"ACGT\n", (BAD_START, 0, 0)), (broken(0, b"r0"), (BAD_START, 0, 0)), (broken(8, b">r2"), (BAD_START, 2, 8)),
             (broken(14, b"-"), (MISSING_PLUS, 3, 14)), (broken(14, b""), (MISSING_PLUS, 3, 14)),
             (broken(11, lines[11] + b"I"), (LENGTH_MISMATCH, 2, 11)), (broken(9, lines[9][:-1]), (LENGTH_MISMATCH, 2, 9 + 2)),
             (broken(18, b"-"), (MISSING_PLUS, 4, 18))]
    for bad, err in cases:
        for final in (0, 1):
            r = harness.parse(bad, final)
            assert r["rc"] == ERR_FORMAT and r["error"] == err and r["seqs"] == [] and r["consumed"] == 0, (bad, r)
            same(r, restate(bad, final))
            assert harness.parse(bad, final, max_reads=1)["error"] == err      # an error behind the cut is an error of the call
    # two bad records: the smaller index; two failed checks in one record: the first
    two = broken(14, b"-").split(b"\n"); two[7] = two[7] + b"II"
    assert harness.parse(b"\n".join(two), 1)["error"] == (LENGTH_MISMATCH, 1, 7)
    one = list(lines); one[8] = b"r2"; one[10] = b"-"; one[11] = b""
    assert harness.parse(b"\n".join(one), 1)["error"] == (BAD_START, 2, 8)
    # truncated: only a final text has a last record
    cut = b"\n".join(lines[:22])                        # record 5 without its '+' and quality lines
    assert harness.parse(cut, 0)["rc"] == OK and len(harness.parse(cut, 0)["seqs"]) == 5
    r = harness.parse(cut, 1)
    assert r["rc"] == ERR_FORMAT and r["error"] == (TRUNCATED, 5, 22) and r["seqs"] == []
    same(r, restate(cut, 1))
    # a record not yet complete is not checked
    assert harness.parse(b"@r\nAC\n+\nII\n@s\nAC\nxx\n", 0)["seqs"] == [b"AC"]
    assert harness.parse(b"@r\nAC\n+\nII\n@s\nAC\nxx\n", 1)["error"] == (MISSING_PLUS, 1, 6)


def test_dollar_separated_transcripts_equal_the_list_form():
    """what quantify_files hands the bias models from the packed pair = what quantify_reads builds from the lists"""
    from sailfish_amd import mapper
    seqs = [b"ACGT", b"", b"N", b"GATTACA" * 9]
    want_s, want_o = mapper.pack_sequences([s + b"$" for s in seqs])
    got_s, got_o = mapper._dollar_separated(*mapper.pack_sequences(seqs))
    assert got_s == want_s.numpy().tobytes() and np.array_equal(got_o, want_o[:-1].numpy())
