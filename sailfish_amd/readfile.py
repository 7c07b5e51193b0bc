"""Transcript and read files in, packed sequences on the device out: the file side of sfgpu_reads_parse_host
(csrc/readtext.hip; the record rules are csrc/readfmt.h).

`ReadDeviceWriter` is the way back: batches of records that lie on the device become a FASTA / FASTQ file (plain or BGZF), formatted
there (sfgpu_reads_write_text / _bgzf, csrc/readtext_write.hip; the rules are csrc/readwfmt.h, and `reads_text_host` states them).

`ReadFile` reads a FASTA or FASTQ file in blocks, keeps the bytes the parser has not consumed, and hands out batches of records
as the `(uint8 bases, int64 offsets)` pairs that `QuasiIndex` and `QuasiIndex.map_reads` take.  Nothing is parsed on the host:
the host reads the file, the device finds the records.

A gzip file is detected by its magic bytes.  The blocked form (BGZF: what bgzip and the Illumina converters write, and
`gzfile.write_bgzf`) is inflated on the device, one wavefront per member (sfgpu_bgzf_inflate_host, csrc/bgzf_read.hip), and parsed
where it lands (sfgpu_reads_parse_device): the host reads the compressed file and hops over the member sizes, nothing else.
Any other gzip file is one serial bit stream per member.  By default it is inflated on the host with Python's `gzip` module and
fed through the plain-text path, which is then bound by the host's inflate; with inflate="device" it is inflated on the device
chunk by chunk (sfgpu_gzrd_*, csrc/gz_read.hip: block starts are found speculatively, the chunks are decoded twice, the gzip
trailer's CRC-32 says whether the result is right) and parsed where it lands, like a BGZF file."""
import ctypes as C
import gzip
import os

import numpy as np
import torch

from . import _lib

MAX_TEXT = 1 << 30            # one parse call (sfgpu_reads_parse_host)
BGZF_KINDS = {1: "not a BGZF member header", 2: "the member ends before its last block does", 3: "block type 3",
              4: "a stored block's LEN and NLEN disagree", 5: "invalid code lengths", 6: "invalid literal/length or distance code",
              7: "a match reaches before the member's first byte", 8: "the payload is not ISIZE bytes", 9: "CRC-32 mismatch"}
GZ_KINDS = {**BGZF_KINDS, 1: "not a gzip member header", 2: "the file ends inside a member"}
KINDS = {1: "a record does not begin with '@' (or the file with neither '>' nor '@')",
         2: "the third line of the record does not begin with '+'",
         3: "quality and sequence differ in length",
         4: "the last record has fewer than four lines"}
WRITE_KINDS = {1: "the name holds a line end", 2: "the bases hold a line end", 3: "the qualities hold a line end",
               4: "the first base of a FASTA record is '>'"}


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


def bgzf_member_bytes(head):
    """bytes of the gzip member whose header begins `head` when it carries the BGZF 'BC' subfield (BSIZE + 1), else None"""
    if len(head) < 18 or head[:3] != b"\x1f\x8b\x08" or not head[3] & 4:
        return None
    xlen = head[10] | head[11] << 8
    p, end = 12, min(12 + xlen, len(head))
    while p + 4 <= end:
        slen = head[p + 2] | head[p + 3] << 8
        if head[p:p + 2] == b"BC" and slen == 2 and p + 6 <= end:
            return (head[p + 4] | head[p + 5] << 8) + 1
        p += 4 + slen
    return None


class DeviceCarry:
    """The carry-over around a device inflater and the device parser: compressed blocks in, the compressed bytes the inflater has
    not consumed in front of the next block; the inflated text stays in one device buffer, the parser's unconsumed tail is moved to
    its front (device to device) and the next text is inflated behind it.  next() is BlockCarry.next for this path; _more() is
    the inflater's."""

    def __init__(self, owner, stream, block_bytes):
        self.o, self.stream, self.block_bytes = owner, stream, int(block_bytes)
        self.cbuf = np.empty(max(self.block_bytes, 1 << 16), np.uint8)     # compressed bytes read and not inflated: cbuf[:chi]
        self.chi = 0
        self.file_off = 0                     # where cbuf[0] lies in the file
        self.members = 0                      # members inflated so far
        self.eof = False
        self.text = None                      # device buffer; text[lo:hi] = inflated and not consumed
        self.lo = self.hi = 0
        self.records = 0
        self.starved = True

    def _read(self, want):
        if want > self.cbuf.size:
            grown = np.empty(max(want, 2 * self.cbuf.size), np.uint8)
            grown[: self.chi] = self.cbuf[: self.chi]
            self.cbuf = grown
        while not self.eof and self.chi < want:
            got = self.stream.readinto(memoryview(self.cbuf)[self.chi:want])
            if not got:
                self.eof = True
            else:
                self.chi += got

    def _place(self, n_out):
        """room for n_out bytes behind the unconsumed text, which moves to the front of the (possibly grown) buffer -> its length"""
        o, tail = self.o, self.hi - self.lo
        need = ((tail + n_out + 1 + 15) & ~15) + 16       # what the parser asks for behind the text
        if self.text is None or self.text.numel() < need:
            grown = torch.empty(max(need, 0 if self.text is None else 2 * self.text.numel()), dtype=torch.uint8, device=o.device)
            if tail:
                grown[:tail] = self.text[self.lo:self.hi]
            self.text = grown
        elif self.lo and tail:
            self.text[:tail] = self.text[self.lo:self.hi].clone()
        self.lo, self.hi = 0, tail
        return tail

    def _drop(self, used):
        self.cbuf[: self.chi - used] = self.cbuf[used:self.chi].copy()
        self.chi -= used
        self.file_off += used

    def close(self):
        pass

    def next(self, max_reads):
        while max_reads > 0:
            if self.starved or self.hi == self.lo:
                more = self._more()
                self.starved = False
                if not more and self.hi == self.lo:
                    return None
            final = self.eof and self.chi == 0
            res = self.o._parse_device(self.text, self.lo, self.hi, final, max_reads, self.records)
            if res.n_reads or final:
                self.lo += res.consumed
                self.records += res.n_reads
                return res if res.n_reads else None
            if self.hi - self.lo >= MAX_TEXT - (1 << 17):
                raise ValueError(f"{self.o.path}: record {self.records} does not end within 1 GiB")
            self.starved = True
        return None


class DeviceInflate(DeviceCarry):
    """DeviceCarry for a BGZF file: the members that do not end in a block wait in front of the next one"""

    def _inflate_error(self, res):
        m, off = int(res.error_member), self.file_off
        for _ in range(m):                    # hop to the bad member for its offset (the error path only)
            off += bgzf_member_bytes(bytes(self.cbuf[off - self.file_off:off - self.file_off + 65536]))
        raise ValueError(f"{self.o.path}: gzip member {self.members + m} (byte {off} of the file) does not inflate: "
                         f"{BGZF_KINDS.get(res.error_kind, 'malformed')} (kind {res.error_kind})")

    def _more(self):
        """inflate the next block behind the unconsumed text; False at the end of the file"""
        o, L = self.o, self.o._L
        want = self.block_bytes
        while True:
            self._read(max(want, self.chi + 1) if self.chi >= want else want)
            if self.chi == 0 and self.eof:
                return False
            tail = self.hi - self.lo
            room = MAX_TEXT - 64 - tail
            res = _lib.BgzfResult()
            rc = L.sfgpu_bgzf_inflate_host(_lib.ptr(self.cbuf), self.chi, int(self.eof), None, room, C.byref(res), None)      # sizes only
            if rc == _lib.ERR_FORMAT and res.n_members == 0:
                self._inflate_error(res)
            if res.n_members:
                break
            if self.eof:
                return False
            if self.chi >= MAX_TEXT:
                raise ValueError(f"{o.path}: gzip member {self.members} does not end within 1 GiB")
            want = max(want, self.chi) * 2
        with torch.cuda.device(o.device):
            tail = self._place(int(res.n_bytes_out))
            res = _lib.BgzfResult()
            rc = L.sfgpu_bgzf_inflate_host(_lib.ptr(self.cbuf), self.chi, int(self.eof), _lib.ptr(self.text[tail:]), room, C.byref(res),
                                           _lib.current_stream_ptr())
        if rc == _lib.ERR_FORMAT:
            self._inflate_error(res)
        _lib.check(rc)
        n_out = int(res.n_bytes_out)
        self.hi = tail + n_out
        used = int(res.consumed)
        self._drop(used)
        self.members += int(res.n_members)
        for k, v in (("ms_inflate", res.ms_kernels), ("ms_copy", res.ms_copy), ("bytes_compressed", used), ("members", int(res.n_members))):
            o.stats[k] += v
        return True


class DeviceGunzip(DeviceCarry):
    """DeviceCarry for an ordinary gzip file: plan (finder, pass A, chain, propagation: sizes only) -> room in the text buffer ->
    emit (pass B) behind the unconsumed text.  One call ends with a member at the latest, so a file of many small members costs
    a call per member."""

    def __init__(self, owner, stream, block_bytes, chunk_bytes=0):
        super().__init__(owner, stream, block_bytes)
        self.z = C.c_void_p()
        self.failed = None                    # the error a plan found behind chunks that were still good (file offset in error_offset)
        with torch.cuda.device(owner.device):
            _lib.check(owner._L.sfgpu_gzrd_open(C.byref(self.z), chunk_bytes))

    def close(self):
        if self.z:
            self.o._L.sfgpu_gzrd_close(self.z); self.z = C.c_void_p()

    def _inflate_error(self, res):
        at = int(res.error_offset) if res is self.failed else self.file_off + int(res.error_offset)
        raise ValueError(f"{self.o.path}: gzip member {self.members} (byte {at} of the file) does not "
                         f"inflate: {GZ_KINDS.get(res.error_kind, 'malformed')} (kind {res.error_kind})")

    def _more(self):
        """inflate the next chunks behind the unconsumed text; False at the end of the file"""
        o, L = self.o, self.o._L
        if self.failed is not None:
            self._inflate_error(self.failed)
        want = self.block_bytes
        with torch.cuda.device(o.device):
            while True:
                self._read(max(want, self.chi + 1) if self.chi >= want else want)
                room = MAX_TEXT - 64 - (self.hi - self.lo)
                res = _lib.GzrdResult()
                rc = L.sfgpu_gzrd_plan_host(self.z, _lib.ptr(self.cbuf), self.chi, int(self.eof), room, C.byref(res), _lib.current_stream_ptr())
                if rc == _lib.ERR_FORMAT and res.n_chunks == 0:
                    self._inflate_error(res)
                if rc != _lib.ERR_FORMAT:              # (an error behind good chunks: they are emitted first, see below)
                    _lib.check(rc)
                for k, v in (("ms_copy", res.ms_copy), ("ms_find", res.ms_find), ("ms_decode", res.ms_decode), ("ms_inflate", res.ms_decode),
                             ("ms_propagate", res.ms_propagate)):
                    o.stats[k] += v
                if res.n_chunks:
                    break
                if res.need_cap:
                    raise ValueError(f"{o.path}: one chunk of gzip member {self.members} holds {int(res.need_cap)} bytes: more than a call takes")
                if res.consumed:                           # padding between members
                    self._drop(int(res.consumed)); o.stats["bytes_compressed"] += int(res.consumed)
                    continue
                if self.eof:
                    return False
                if self.chi >= MAX_TEXT:
                    raise ValueError(f"{o.path}: a block of gzip member {self.members} does not end within 1 GiB")
                want = min(max(want, self.chi) * 2, MAX_TEXT)
            tail = self._place(int(res.n_bytes_out))
            planned = (res.error_kind, int(res.error_offset))
            rc = L.sfgpu_gzrd_emit(self.z, _lib.ptr(self.text[tail:]), C.byref(res), _lib.current_stream_ptr())
        if rc == _lib.ERR_FORMAT:
            # Which error is it?  The emit returns the plan's own (kind, offset) only when every chunk in front of it decoded in
            # pass B: an error of pass B names an earlier chunk (another offset), and a trailer check cannot coincide with a plan
            # error, because the chain then ends in front of the final block.  Anything else means the text is not to be trusted.
            if (res.error_kind, int(res.error_offset)) != planned or not planned[0]:
                self._inflate_error(res)
            # the plan's error lies behind these chunks: their records are delivered, the next call raises (as the BGZF path does)
            self.failed = _lib.GzrdResult.from_buffer_copy(res)
            self.failed.error_offset = self.file_off + int(res.error_offset)
        else:
            _lib.check(rc)
        self.hi = tail + int(res.n_bytes_out)
        used = int(res.consumed)
        self._drop(used)
        self.members += int(res.member_end)
        for k, v in (("ms_emit", res.ms_emit), ("ms_inflate", res.ms_emit), ("bytes_compressed", used), ("members", int(res.member_end)), ("chunks", int(res.n_chunks)),
                     ("candidates", int(res.n_candidates)), ("false_starts", int(res.n_false_starts))):
            o.stats[k] += v
        return True


class ReadFile:
    """A FASTA / FASTQ file (plain or gzip) read through the device parser.

    read(max_reads) -> (bases: uint8 device tensor, offsets: int64 device tensor [n + 1]) holding exactly max_reads records unless
    the file ends first (n == 0 at the end).  With names=True the record names (bytes) of the last read() are in `last_names`,
    sliced on the host from the name spans the parser reports.  With names="device" they stay where the parser left them:
    `last_names` is then the (uint8 device tensor, int64 device tensor [n + 1]) pair of the names back to back and their offsets
    (sfgpu_reads_parse_*_n), the form SamDeviceWriter.write(read_names=) and mate_names_match take; nothing is copied back and no
    Python runs per record (no reads: an empty tensor and one zero).
    With quals=True the qualities of the last read() are in `last_quals`: a uint8 device tensor that shares the bases' offsets
    (record r's are last_quals[offsets[r]:offsets[r + 1]], the bytes of its quality line), or None for a FASTA file.
    `inflate` says where a gzip file is inflated: "auto" takes the device for a BGZF file (its first member carries the 'BC'
    subfield) and the host for any other gzip file, "host" forces Python's gzip, "device" takes the device for every gzip file
    (a BGZF file member by member, any other chunk by chunk: DeviceGunzip); the attribute `inflate` is "device", "host" or None (a
    plain file).  block_bytes counts bytes of the file as it is stored: compressed ones on the device path.  `stats` counts, for
    an ordinary gzip file on the device, the chunks decoded, the block starts the finder accepted (candidates) and those of them
    that the chain did not reach (false_starts); ms_inflate is there ms_decode (pass A) + ms_emit (pass B)."""

    def __init__(self, path, device="cuda", block_bytes=32 << 20, names=False, inflate="auto", quals=False):
        if inflate not in ("auto", "host", "device"):
            raise ValueError("inflate must be 'auto', 'host' or 'device'")
        self.path = str(path)
        self.device = torch.device(device)
        self._L = _lib.lib()
        with open(self.path, "rb") as f:
            head = f.read(4096)
        self.gzipped = head[:2] == b"\x1f\x8b"
        bgzf = self.gzipped and bgzf_member_bytes(head) is not None
        self.inflate = None if not self.gzipped else "device" if inflate == "device" or (inflate == "auto" and bgzf) else "host"
        if isinstance(names, str) and names != "device":
            raise ValueError("names must be True, False or 'device'")
        self._names_dev = isinstance(names, str)        # the device blob
        self._names = bool(names) and not self._names_dev      # the host list
        self.last_names = self._no_names() if self._names_dev else []
        self._quals = bool(quals)
        self.last_quals = None
        self.format = 0
        self.stats = dict(calls=0, bytes_parsed=0, ms_copy=0.0, ms_kernels=0.0, ms_inflate=0.0, bytes_compressed=0, members=0,
                          chunks=0, candidates=0, false_starts=0, ms_find=0.0, ms_decode=0.0, ms_propagate=0.0, ms_emit=0.0)
        if self.inflate == "device":
            self._f = open(self.path, "rb", buffering=0)
            self._carry = (DeviceInflate if bgzf else DeviceGunzip)(self, self._f, block_bytes)
        else:
            self._f = gzip.open(self.path, "rb") if self.gzipped else open(self.path, "rb", buffering=0)
            self._carry = BlockCarry(self._f, block_bytes, self.path)

    def _parse(self, text, final, max_reads):
        n = int(text.size)
        max_reads = int(min(max_reads, n // 2 + 1))          # a record has at least two bytes (the last of a file: one)
        bases = torch.empty(max(n, 16), dtype=torch.uint8, device=self.device)
        off = torch.empty(max_reads + 1, dtype=torch.int64, device=self.device)
        span = torch.empty(2 * max_reads, dtype=torch.int64, device=self.device) if self._names else None
        qual = torch.empty(max(n, 16), dtype=torch.uint8, device=self.device) if self._quals else None
        blob, blob_off, cap_names, n_name = self._name_room(n, max_reads)
        res = _lib.ReadsResult()
        with torch.cuda.device(self.device):
            rc = self._L.sfgpu_reads_parse_host_n(_lib.ptr(text), n, int(final), max_reads, _lib.ptr(bases), _lib.ptr(qual), n, _lib.ptr(off),
                                                  _lib.ptr(span), _lib.ptr(blob), cap_names, _lib.ptr(blob_off), C.byref(n_name), C.byref(res),
                                                  _lib.current_stream_ptr())
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
        elif self._names_dev:
            names = self._name_pair(blob, blob_off, int(n_name.value), int(res.n_reads), max_reads)
        off = off[: res.n_reads + 1]
        if 2 * off.numel() < max_reads:                        # a batch must not pin an array sized for the records that might have been
            off = off.clone()
        return Parsed(int(res.n_reads), int(res.consumed), (bases[: res.n_bases], off, names, qual[: res.n_bases] if self._kept(res, qual) else None))

    def _parse_device(self, text, lo, hi, final, max_reads, records):
        """_parse for text[lo:hi] of a device buffer (lo is a multiple of 16 or the text is moved there first by the caller)"""
        n = hi - lo
        max_reads = int(min(max_reads, n // 2 + 1))
        with torch.cuda.device(self.device):
            if lo % 16:                                         # the parser wants its text at a 16-byte boundary
                text[:n] = text[lo:hi].clone()
                self._carry.lo, self._carry.hi, lo, hi = 0, n, 0, n
            bases = torch.empty(max(n, 16), dtype=torch.uint8, device=self.device)
            off = torch.empty(max_reads + 1, dtype=torch.int64, device=self.device)
            span = torch.empty(2 * max_reads, dtype=torch.int64, device=self.device) if self._names else None
            qual = torch.empty(max(n, 16), dtype=torch.uint8, device=self.device) if self._quals else None
            blob, blob_off, cap_names, n_name = self._name_room(n, max_reads)
            res = _lib.ReadsResult()
            view = text[lo:]
            rc = self._L.sfgpu_reads_parse_device_n(_lib.ptr(view), n, view.numel(), int(final), max_reads, _lib.ptr(bases), _lib.ptr(qual), n,
                                                    _lib.ptr(off), _lib.ptr(span), _lib.ptr(blob), cap_names, _lib.ptr(blob_off), C.byref(n_name),
                                                    C.byref(res), _lib.current_stream_ptr())
        if rc == _lib.ERR_FORMAT:
            raise ValueError(f"{self.path}: record {records + res.error_record} is malformed: "
                             f"{KINDS.get(res.error_kind, 'malformed')} (kind {res.error_kind})")
        _lib.check(rc)
        self.format = res.format or self.format
        for k, v in (("calls", 1), ("bytes_parsed", n), ("ms_kernels", res.ms_kernels)):
            self.stats[k] += v
        names = None
        if self._names and res.n_reads:                         # the bytes of the spans only come back
            sp = span[: 2 * res.n_reads].view(-1, 2)
            lens = sp[:, 1]
            ends = torch.cumsum(lens, 0)
            idx = torch.arange(int(ends[-1]), device=self.device) + torch.repeat_interleave(sp[:, 0] - (ends - lens), lens)
            raw = view[idx].cpu().numpy().tobytes()
            cuts = np.concatenate([[0], ends.cpu().numpy()]).tolist()
            names = [raw[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        elif self._names_dev:
            names = self._name_pair(blob, blob_off, int(n_name.value), int(res.n_reads), max_reads)
        off = off[: res.n_reads + 1]
        if 2 * off.numel() < max_reads:
            off = off.clone()
        return Parsed(int(res.n_reads), int(res.consumed), (bases[: res.n_bases], off, names, qual[: res.n_bases] if self._kept(res, qual) else None))

    def _no_names(self):
        return torch.zeros(0, dtype=torch.uint8, device=self.device), torch.zeros(1, dtype=torch.int64, device=self.device)

    def _name_room(self, n, max_reads):
        """what a parse call of n bytes needs for its name blob -> (blob, offsets, cap_names, n_name_bytes); Nones and 0 without one"""
        if not self._names_dev:
            return None, None, 0, C.c_uint64(0)
        cap = max((n + 15) & ~15, 16)                        # the names of a text are never more than its bytes
        return (torch.empty(cap, dtype=torch.uint8, device=self.device), torch.empty(max_reads + 1, dtype=torch.int64, device=self.device),
                cap, C.c_uint64(0))

    @staticmethod
    def _name_pair(blob, blob_off, n_name, n_reads, max_reads):
        """the pair of one parse call; like the offsets of the bases, it must not pin arrays sized for what might have been"""
        b, o = blob[:n_name], blob_off[: n_reads + 1]
        if 2 * n_name < blob.numel():
            b = b.clone()
        if 2 * o.numel() < max_reads:
            o = o.clone()
        return b, o

    @staticmethod
    def _kept(res, qual):
        """the parse wrote the qualities: they were asked for and the text is FASTQ"""
        return qual is not None and res.format == 2            # SFGPU_READS_FASTQ

    def read(self, max_reads):
        parts, left = [], int(max_reads)
        while left > 0:
            res = self._carry.next(left) if self.inflate == "device" else self._carry.next(self._parse, left)
            if res is None:
                break
            parts.append(res.payload)
            left -= res.n_reads
        if self._names_dev:
            pairs = [p[2] for p in parts]
            if len(pairs) <= 1:
                self.last_names = pairs[0] if pairs else self._no_names()
            else:                                              # rebased on the device, as the bases are below
                acc, offs = pairs[0][1][-1], [pairs[0][1]]
                for _, o in pairs[1:]:
                    offs.append(o[1:] + acc)
                    acc = acc + o[-1]
                self.last_names = torch.cat([b for b, _ in pairs]), torch.cat(offs)
        else:
            self.last_names = [nm for p in parts for nm in (p[2] or [])]
        kept = [p[3] for p in parts if p[3] is not None]
        self.last_quals = (kept[0] if len(kept) == 1 else torch.cat(kept)) if kept and len(kept) == len(parts) else None
        if not parts:
            return torch.zeros(1, dtype=torch.uint8, device=self.device), torch.zeros(1, dtype=torch.int64, device=self.device)
        if len(parts) == 1:
            return parts[0][0], parts[0][1]
        acc = parts[0][1][-1]                                  # the rebasing stays on the device
        offs = [parts[0][1]]
        for b, o, _, _ in parts[1:]:
            offs.append(o[1:] + acc)
            acc = acc + o[-1]
        return torch.cat([p[0] for p in parts]), torch.cat(offs)

    def close(self):
        if self._f is not None:
            self._f.close(); self._f = None
            if self.inflate == "device":
                self._carry.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def mate_stem(name):
    """the name without a trailing b"/1" or b"/2" (whichever digit it is), any other name whole: what the names of two mates have
    to share.  The Python statement of csrc/readfmt.h's rf_mate_stem_len."""
    name = bytes(name)
    return name[:-2] if len(name) >= 2 and name[-2:] in (b"/1", b"/2") else name


def mate_names_match(pair1, pair2):
    """Do two batches of read names run in step?  pair1, pair2: (uint8 device tensor, int64 device tensor [n + 1]) as
    ReadFile(names="device") leaves them in `last_names`.  -> None when every read's two names have the same mate_stem, else the
    lowest read whose names disagree.  Compared on the device (sfgpu_reads_names_match); one integer comes back.  The offsets are
    trusted as the parser's are (never decreasing, the last one within the bytes): only shapes and types are looked at here."""
    (b1, o1), (b2, o2) = pair1, pair2
    n = int(o1.numel()) - 1
    if int(o2.numel()) - 1 != n or n < 0:
        raise ValueError(f"{n} names against {int(o2.numel()) - 1}")
    for b, o in ((b1, o1), (b2, o2)):
        if b.dtype != torch.uint8 or o.dtype != torch.int64 or not b.is_cuda or o.device != b.device or b.device != b1.device:
            raise TypeError("expected (uint8, int64) tensors on one device")
    b1, o1, b2, o2 = (t.contiguous() for t in (b1, o1, b2, o2))
    first = C.c_uint64(0)
    with torch.cuda.device(b1.device):
        _lib.check(_lib.lib().sfgpu_reads_names_match(_lib.ptr(b1), _lib.ptr(o1), _lib.ptr(b2), _lib.ptr(o2), n, C.byref(first),
                                                      _lib.current_stream_ptr()))
    return None if first.value == 2 ** 64 - 1 else int(first.value)


def read_transcripts(path, device="cuda", block_bytes=32 << 20, inflate="auto"):
    """a transcript FASTA (or FASTQ) whole -> (names: list of str, (bases, offsets) on the device); the names are sliced on the
    host from the name spans the parser reports"""
    with ReadFile(path, device, block_bytes, names=True, inflate=inflate) as rf:
        bases, off = rf.read(1 << 62)
        names = [nm.decode("utf-8", "replace") for nm in rf.last_names]
    if off.numel() <= 1:
        raise ValueError(f"{path}: no records")
    return names, (bases, off)


# ---- the way back: records on the device -> a read file --------------------------------------------------------------------

def reads_text_host(seqs, quals=None, names=None, select=None, index_base=0):
    """The text sfgpu_reads_write_text writes, stated on the host over lists of bytes (csrc/readwfmt.h): the records r with
    select[r] (all of them without `select`) in input order, FASTQ '@' name \\n bases \\n + \\n qualities \\n when `quals` is given,
    else FASTA '>' name \\n bases \\n, never wrapped; without `names` record r is called r<index_base + r>.  A selected record that
    cannot be written raises ValueError naming the lowest such record and the lowest WRITE_KINDS kind it breaks."""
    out = []
    for r, seq in enumerate(seqs):
        if select is not None and not select[r]:
            continue
        seq = bytes(seq)
        name = bytes(names[r]) if names is not None else b"r%d" % (index_base + r)
        qual = None if quals is None else bytes(quals[r])
        kind = (1 if b"\n" in name else 2 if b"\n" in seq else 3 if qual is not None and b"\n" in qual else
                4 if qual is None and seq[:1] == b">" else 0)
        if kind:
            raise ValueError(f"record {r}: {WRITE_KINDS[kind]} (kind {kind})")
        if qual is None:
            out.append(b">" + name + b"\n" + seq + b"\n")
        else:
            if len(qual) != len(seq):
                raise ValueError(f"record {r}: {len(qual)} quality bytes for {len(seq)} bases")
            out.append(b"@" + name + b"\n" + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out)


class ReadDeviceWriter:
    """A FASTA / FASTQ file written from batches of records that lie on the device: the mirror of ReadFile.

    `path_or_file`: a path, or a binary file object (left open by close()).  write((bases, offsets), quals=, names=, select=) takes
    one batch as ReadFile.read returns it -- a uint8 device tensor of the bases and the int64 device tensor of their offsets --
    with, optionally, the qualities (a uint8 device tensor that shares the offsets: ReadFile's last_quals), the names (the
    (uint8, 64-bit offsets) pair of ReadFile(names="device").last_names) and a selector (one uint8 or bool a record: nonzero =
    write it; default all), and appends the selected records in input order; -> the number of records written.  No name, base or
    offset visits the host.  The first write fixes the format: FASTQ iff `quals` is given; a later batch of the other kind is a
    ValueError.  Without `names` a record is called r<index>, the index counted over all records SEEN so far, written or not: the
    name says where the read stood in the input.  A selected record that cannot be written (WRITE_KINDS) raises ValueError naming
    the record, counted from the first batch, and the kind; nothing of that batch is written.
    compress=True writes a BGZF file whose members are encoded on the device (gzfile.BgzfDeviceWriter): the formatted chunks go
    from the formatter to the encoder on the device, only compressed bytes are copied, and close() writes the EOF member; the
    format is never inferred from the path.  chunk_bytes: 0 (the library's 32 MiB) or 16 .. 2^30; no record may be longer.
    `stats` sums batches, reads_in, reads_written, bytes (of text), bytes_out (of the file: known at close() when compressed),
    chunks and the device / copy / sink / encode times."""

    def __init__(self, path_or_file, *, compress=False, chunk_bytes=0):
        self._L = _lib.lib()
        self.compress, self.chunk_bytes = bool(compress), int(chunk_bytes)
        self._own = isinstance(path_or_file, (str, bytes, os.PathLike))
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        self.format = 0                                    # 1 FASTA, 2 FASTQ (SFGPU_READS_*), fixed by the first write
        self.n_seen = 0                                    # the running record index
        self.stats = dict(batches=0, reads_in=0, reads_written=0, bytes=0, bytes_out=0, chunks=0, ms_format=0.0, ms_copy=0.0, ms_sink=0.0,
                          ms_encode=0.0)
        self._z = None
        if self.compress:
            from . import gzfile
            self._z = gzfile.BgzfDeviceWriter(self._f, chunk_bytes=self.chunk_bytes)

    def write(self, reads, *, quals=None, names=None, select=None):
        if self._f is None:
            raise ValueError("the read writer is closed")
        bases, off = reads
        dev = off.device
        if bases.dtype != torch.uint8 or off.dtype != torch.int64 or not off.is_cuda or bases.device != dev:
            raise TypeError("expected (uint8 bases, int64 offsets) on one device")
        n = int(off.numel()) - 1
        if n < 0:
            raise ValueError("the offsets of a batch have at least one entry")
        fmt = 1 if quals is None else 2
        if self.format and fmt != self.format:
            raise ValueError("a {} batch for a {} file: the first write fixed the format".format(*(("FASTA", "FASTQ") if fmt == 1 else ("FASTQ", "FASTA"))))
        one = lambda: torch.zeros(1, dtype=torch.uint8, device=dev)        # nothing at all: still "given"
        bases, off = bases.contiguous(), off.contiguous()
        if quals is not None:
            if quals.dtype != torch.uint8 or quals.device != dev:
                raise TypeError("quals: expected a uint8 tensor on the bases' device")
            if quals.numel() != bases.numel():
                raise ValueError(f"{quals.numel()} quality bytes for {bases.numel()} bases")
            quals = quals.contiguous() if quals.numel() else one()
        nb = no = None
        if names is not None:
            nb, no = names
            if nb.element_size() != 1 or no.is_floating_point() or no.element_size() != 8 or nb.device != dev or no.device != dev:
                raise TypeError("names: expected (bytes, 64-bit integer offsets) on the bases' device")
            if no.numel() != n + 1:
                raise ValueError(f"{no.numel() - 1} names for {n} reads")
            nb, no = nb.contiguous() if nb.numel() else one(), no.contiguous()
        if select is not None:
            if select.element_size() != 1 or select.is_floating_point() or select.device != dev:
                raise TypeError("select: expected one uint8 or bool a record on the bases' device")
            if select.numel() != n:
                raise ValueError(f"a selector of {select.numel()} entries for {n} reads")
            select = select.contiguous().view(torch.uint8) if n else None
        raised = []

        def sink(addr, nbytes, _user):
            try:                                   # nothing may unwind through the C frame
                self._f.write(memoryview((C.c_char * nbytes).from_address(addr)))
                return 0
            except BaseException as e:             # noqa: BLE001  (re-raised below)
                raised.append(e)
                return 1

        res = _lib.ReadWriteResult()
        batch = (_lib.ptr(bases if bases.numel() else one()), _lib.ptr(off), n, _lib.ptr(quals), _lib.ptr(nb), _lib.ptr(no), self.n_seen,
                 _lib.ptr(select), self.chunk_bytes)
        with torch.cuda.device(dev):
            if self._z is None:
                rc = self._L.sfgpu_reads_write_text(*batch, _lib.TEXT_SINK(sink), None, C.byref(res), _lib.current_stream_ptr())
            else:
                self._z._open(dev)
                rc = self._L.sfgpu_reads_write_bgzf(*batch, self._z._h, C.byref(res), _lib.current_stream_ptr())
        sunk = raised if self._z is None else self._z._raised      # what this call's sink raised: the encoder's, when it does the sinking
        if sunk:
            raise sunk.pop(0)
        if rc == _lib.ERR_FORMAT and res.error_kind:
            raise ValueError(f"record {self.n_seen + int(res.error_record)}: {WRITE_KINDS.get(res.error_kind, 'cannot be written')} (kind {res.error_kind})")
        _lib.check(rc)
        self.format = fmt
        self.n_seen += n
        st = self.stats
        for k, v in (("batches", 1), ("reads_in", n), ("reads_written", res.n_selected), ("bytes", res.n_bytes), ("chunks", res.n_chunks)):
            st[k] += int(v)
        if self._z is None:
            st["bytes_out"] += int(res.n_bytes)
        st["ms_format"] += res.format_ms; st["ms_copy"] += res.d2h_ms; st["ms_sink"] += res.sink_ms
        return int(res.n_selected)

    def close(self):
        if self._f is None:
            return
        try:
            if self._z is not None:
                try:
                    res = self._z.close()              # the EOF member
                finally:
                    self._z = None
                st = self.stats
                st["bytes_out"], st["ms_encode"] = res["n_bytes_out"], res["encode_ms"]
                st["ms_copy"] += res["d2h_ms"]; st["ms_sink"] += res["sink_ms"]
        finally:                                       # the file is released also when the encoder's close raises
            f, self._f = self._f, None
            if self._own:
                f.close()
            else:
                f.flush()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
