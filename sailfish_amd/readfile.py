"""Transcript and read files in, packed sequences on the device out: the file side of sfgpu_reads_parse_host
(csrc/readtext.hip; the record rules are csrc/readfmt.h).

`ReadFile` reads a FASTA or FASTQ file in blocks, keeps the bytes the parser has not consumed, and hands out batches of records
as the `(uint8 bases, int64 offsets)` pairs that `QuasiIndex` and `QuasiIndex.map_reads` take.  Nothing is parsed on the host:
the host reads the file, the device finds the records.

A gzip file (detected by its magic bytes) is inflated on the host with Python's `gzip` module and fed through the same path;
that path is bound by the host's inflate, not by the device."""
import ctypes as C
import gzip

import numpy as np
import torch

from . import _lib

MAX_TEXT = 1 << 30            # one parse call (sfgpu_reads_parse_host)
KINDS = {1: "a record does not begin with '@' (or the file with neither '>' nor '@')",
         2: "the third line of the record does not begin with '+'",
         3: "quality and sequence differ in length",
         4: "the last record has fewer than four lines"}


class Parsed:
    """what one parse call emitted: n_reads records, `consumed` bytes of the text, and the parser's payload"""

    def __init__(self, n_reads, consumed, payload=None):
        self.n_reads, self.consumed, self.payload = n_reads, consumed, payload


class BlockCarry:
    """The carry-over around a stateless record parser: blocks of a byte stream, the unconsumed tail in front of the next block.

    parse(text: uint8 array, final: bool, max_reads: int) -> Parsed.  n_reads == 0 on a text that is not final means "no complete
    record yet": the text is grown (doubled, up to 1 GiB) and presented again."""

    def __init__(self, stream, block_bytes, name="<stream>"):
        assert block_bytes >= 1
        self.stream, self.block_bytes, self.name = stream, int(block_bytes), name
        self.buf = np.empty(max(self.block_bytes, 64), np.uint8)
        self.lo = self.hi = 0                 # buf[lo:hi] = bytes read and not consumed
        self.eof = False
        self.records = 0                      # records handed out so far

    def _fill(self, want):
        """read until `want` bytes are at hand or the stream ends"""
        want = min(want, MAX_TEXT)
        if self.lo and self.lo + want > self.buf.size:
            self.buf[: self.hi - self.lo] = self.buf[self.lo:self.hi].copy()
            self.hi -= self.lo; self.lo = 0
        if want > self.buf.size:
            grown = np.empty(max(want, 2 * self.buf.size), np.uint8)
            grown[: self.hi] = self.buf[: self.hi]
            self.buf = grown
        while not self.eof and self.hi - self.lo < want:
            got = self.stream.readinto(memoryview(self.buf)[self.hi:self.lo + want])
            if not got:
                self.eof = True
            else:
                self.hi += got

    def next(self, parse, max_reads):
        """the next parse call that emits records (at most max_reads) -> Parsed, or None at the end of the stream"""
        want = self.block_bytes
        while max_reads > 0:
            self._fill(want)
            text = self.buf[self.lo:self.hi]
            if text.size == 0 and self.eof:
                return None
            res = parse(text, self.eof, max_reads)
            if res.n_reads or self.eof:
                self.lo += res.consumed
                self.records += res.n_reads
                return res if res.n_reads else None
            if text.size >= MAX_TEXT:
                raise ValueError(f"{self.name}: record {self.records} does not end within 1 GiB")
            want = max(want, text.size) * 2
        return None


class ReadFile:
    """A FASTA / FASTQ file (plain or gzip) read through the device parser.

    read(max_reads) -> (bases: uint8 device tensor, offsets: int64 device tensor [n + 1]) holding exactly max_reads records unless
    the file ends first (n == 0 at the end).  With names=True the record names (bytes) of the last read() are in `last_names`.
    The gzip path inflates on the host and is bound by it."""

    def __init__(self, path, device="cuda", block_bytes=32 << 20, names=False):
        self.path = str(path)
        self.device = torch.device(device)
        self._L = _lib.lib()
        with open(self.path, "rb") as f:
            magic = f.read(2)
        self.gzipped = magic == b"\x1f\x8b"
        self._f = gzip.open(self.path, "rb") if self.gzipped else open(self.path, "rb", buffering=0)
        self._carry = BlockCarry(self._f, block_bytes, self.path)
        self._names = bool(names)
        self.last_names = []
        self.format = 0
        self.stats = dict(calls=0, bytes_parsed=0, ms_copy=0.0, ms_kernels=0.0)

    def _parse(self, text, final, max_reads):
        n = int(text.size)
        max_reads = int(min(max_reads, n // 2 + 1))          # a record has at least two bytes (the last of a file: one)
        bases = torch.empty(max(n, 16), dtype=torch.uint8, device=self.device)
        off = torch.empty(max_reads + 1, dtype=torch.int64, device=self.device)
        span = torch.empty(2 * max_reads, dtype=torch.int64, device=self.device) if self._names else None
        res = _lib.ReadsResult()
        with torch.cuda.device(self.device):
            rc = self._L.sfgpu_reads_parse_host(_lib.ptr(text), n, int(final), max_reads, _lib.ptr(bases), n, _lib.ptr(off), _lib.ptr(span),
                                                C.byref(res), _lib.current_stream_ptr())
        if rc == _lib.ERR_FORMAT:
            raise ValueError(f"{self.path}: record {self._carry.records + res.error_record} is malformed: "
                             f"{KINDS.get(res.error_kind, 'malformed')} (kind {res.error_kind})")
        _lib.check(rc)
        self.format = res.format or self.format
        for k, v in (("calls", 1), ("bytes_parsed", n), ("ms_copy", res.ms_copy), ("ms_kernels", res.ms_kernels)):
            self.stats[k] += v
        names = None
        if self._names and res.n_reads:
            sp = span[: 2 * res.n_reads].cpu().numpy().reshape(-1, 2)
            raw = text.tobytes()
            names = [raw[b:b + l] for b, l in sp.tolist()]
        off = off[: res.n_reads + 1]
        if 2 * off.numel() < max_reads:                        # a batch must not pin an array sized for the records that might have been
            off = off.clone()
        return Parsed(int(res.n_reads), int(res.consumed), (bases[: res.n_bases], off, names))

    def read(self, max_reads):
        parts, left = [], int(max_reads)
        while left > 0:
            res = self._carry.next(self._parse, left)
            if res is None:
                break
            parts.append(res.payload)
            left -= res.n_reads
        self.last_names = [nm for p in parts for nm in (p[2] or [])]
        if not parts:
            return torch.zeros(1, dtype=torch.uint8, device=self.device), torch.zeros(1, dtype=torch.int64, device=self.device)
        if len(parts) == 1:
            return parts[0][0], parts[0][1]
        acc = parts[0][1][-1]                                  # the rebasing stays on the device
        offs = [parts[0][1]]
        for b, o, _ in parts[1:]:
            offs.append(o[1:] + acc)
            acc = acc + o[-1]
        return torch.cat([p[0] for p in parts]), torch.cat(offs)

    def close(self):
        if self._f is not None:
            self._f.close(); self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_transcripts(path, device="cuda", block_bytes=32 << 20):
    """a transcript FASTA (or FASTQ) whole -> (names: list of str, (bases, offsets) on the device); the names are sliced on the
    host from the name spans the parser reports"""
    with ReadFile(path, device, block_bytes, names=True) as rf:
        bases, off = rf.read(1 << 62)
        names = [nm.decode("utf-8", "replace") for nm in rf.last_names]
    if off.numel() <= 1:
        raise ValueError(f"{path}: no records")
    return names, (bases, off)
