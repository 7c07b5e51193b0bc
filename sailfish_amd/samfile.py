"""A mapper's SAM file in, hit records on the device out: the file side of sfgpu_sam_parse_host / _device (csrc/samtext.hip; what a
SAM file says to this library is csrc/samfmt.h, and `read_sam_host` below is the contract both are judged by).

`SamFile` reads the file in blocks through the carriers of `readfile` (plain text and host-inflated gzip through pinned blocks,
BGZF and -- with inflate="device" -- ordinary gzip inflated on the device and parsed where they land) and iterates the
`(hits, offsets)` batches that `hits.filter_hits` and `quant.quantify` take.  Nothing of the alignment lines is parsed on the host.
The header is: `read_header` reads the @SQ lines with Python, they are a thousandth of a real file.

The file must be grouped by read name, as mappers write it (all lines of a fragment follow each other); a position-sorted file
is not.  `write_sam` is the way back: hit records as SAM text, for the device mapper's output and for tests."""
import ctypes as C
import gzip
import re

import numpy as np

from .hits import HIT_DTYPE

BAD_FIELDS, BAD_NUMBER, BAD_FLAG, BAD_RNAME, BAD_CIGAR, BAD_LENGTH = 1, 2, 4, 8, 16, 32
KINDS = {BAD_FIELDS: "fewer than 11 tab-separated fields",
         BAD_NUMBER: "FLAG is not a number up to 65535, or POS of a mapped line is not a number in 1 .. 2^31 - 1",
         BAD_FLAG: "the FLAG does not fit the library: a paired call needs 0x1 and exactly one of 0x40 / 0x80, a single-end call no 0x1",
         BAD_RNAME: "RNAME is not one of the transcript names",
         BAD_CIGAR: "CIGAR is neither '*' nor a run of (1-9 digits, one of MIDNSHP=X)",
         BAD_LENGTH: "the read is longer than 65535 bases, or SEQ and CIGAR disagree about its length"}
_CIGAR = re.compile(rb"(?:[0-9]{1,9}[MIDNSHP=X])+")
_CIGAR_OP = re.compile(rb"([0-9]+)([MIDNSHP=X])")
_LEAD = re.compile(rb"(?:[0-9]+H)*((?:[0-9]+S)*)")


def _malformed(path, line, kind):
    return ValueError(f"{path}: line {line} is malformed: {KINDS[kind]} (kind {kind})")


def _open_text(path):
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rb") if gz else open(path, "rb")


def read_header(path):
    """(names, lengths) of the @SQ lines (SN:, LN:) in front of the first alignment line, in file order; plain or gzip"""
    names, lengths = [], []
    with _open_text(path) as f:
        for n, line in enumerate(f, 1):
            if not line.startswith(b"@"):
                break
            fields = line.rstrip(b"\r\n").split(b"\t")
            if fields[0] != b"@SQ":
                continue
            tags = {x[:2]: x[3:] for x in fields[1:] if x[2:3] == b":"}
            if b"SN" not in tags or not tags.get(b"LN", b"").isdigit():
                raise ValueError(f"{path}: line {n}: an @SQ line without SN: and a numeric LN:")
            names.append(tags[b"SN"].decode("utf-8", "surrogateescape"))
            lengths.append(int(tags[b"LN"]))
    return names, lengths


def _name_bytes(names):
    return [nm if isinstance(nm, bytes) else nm.encode("utf-8", "surrogateescape") for nm in names]


# ---- the contract ---------------------------------------------------------------------------------------------------------

def _parse_line(line, tid_of, paired):
    """one non-header line -> (kind, None) or (0, (qname, mapped, side, tid, pos, read_len, fwd))"""
    f = line.split(b"\t")
    if len(f) < 11:
        return BAD_FIELDS, None
    if not (f[1].isdigit() and len(f[1]) <= 5 and int(f[1]) <= 65535):
        return BAD_NUMBER, None
    flag, bad = int(f[1]), 0
    first, second = bool(flag & 0x40), bool(flag & 0x80)
    if (not flag & 0x1 or first == second) if paired else flag & 0x1:
        bad |= BAD_FLAG
    side = (1 if first else 2) if paired else 0
    if flag & (0x4 | 0x800):
        return bad, (f[0], False, side, 0, 0, 0, not flag & 0x10)
    if not (f[3].isdigit() and len(f[3]) <= 10 and 1 <= int(f[3]) <= 2 ** 31 - 1):
        bad |= BAD_NUMBER
    if f[2] not in tid_of:
        bad |= BAD_RNAME
    lead = qlen = read_len = 0
    cigar, seq = f[5], f[9]
    if cigar != b"*" and not _CIGAR.fullmatch(cigar):
        bad |= BAD_CIGAR
    else:
        if cigar != b"*":
            qlen = sum(int(n) for n, op in _CIGAR_OP.findall(cigar) if op in b"MIS=X")
            lead = sum(int(n) for n, _ in _CIGAR_OP.findall(_LEAD.match(cigar).group(1)))
        read_len = len(seq) if seq != b"*" else qlen
        if read_len > 65535 or (seq != b"*" and cigar != b"*" and len(seq) != qlen):
            bad |= BAD_LENGTH
    if bad:
        return bad & -bad, None                       # the first rule in the order FIELDS, NUMBER, FLAG, RNAME, CIGAR, LENGTH
    return 0, (f[0], True, side, tid_of[f[2]], int(f[3]) - 1 - lead, read_len, not flag & 0x10)


def _group_records(lines, paired):
    """the records of one group, in order: lines = [(qname, mapped, side, tid, pos, read_len, fwd)]"""
    pairs = []
    if paired:
        for a, b in zip(lines[:-1], lines[1:]):
            if a[1] and b[1] and a[2] == 1 and b[2] == 2 and a[3] == b[3]:
                frag = max(a[4] + a[5], b[4] + b[5]) - min(a[4], b[4])
                pairs.append((a[3], a[4], b[4], frag, a[5], b[5], a[6], b[6], 3, 0))
    if pairs:
        return sorted(pairs, key=lambda r: r[0])      # (sorted is stable: ties keep file order)
    singles = [(l[3], l[4], 0, 0, l[5], 0, l[6], 0, l[2], 0) for l in lines if l[1]]
    return sorted(singles, key=lambda r: (r[8] == 2, r[0]))


def read_sam_host(data, names, paired, path="<sam>", counts=None):
    """The rules, on the host, written to be read: `data` (bytes: a whole SAM text) -> (HIT_DTYPE array, uint32 offsets [reads + 1]).
    Raises the ValueError SamFile raises (lowest malformed line, 1-based; first broken rule).  `counts`, when a dict, receives
    lines / header / reads / hits / pairs."""
    tid_of = {nm: i for i, nm in enumerate(_name_bytes(names))}
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()                                   # (the text ended in '\n', or is empty)
    groups, n_header = [], 0
    for n, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if line.startswith(b"@"):
            n_header += 1
            continue
        kind, rec = _parse_line(line, tid_of, paired)
        if kind:
            raise _malformed(path, n, kind)
        if groups and groups[-1][-1][0] == rec[0]:
            groups[-1].append(rec)
        else:
            groups.append([rec])
    recs, off = [], [0]
    for g in groups:
        recs.extend(_group_records(g, paired))
        off.append(len(recs))
    if counts is not None:
        counts.update(lines=len(lines), header=n_header, reads=len(groups), hits=len(recs), pairs=sum(r[8] == 3 for r in recs))
    return np.array(recs, dtype=HIT_DTYPE), np.array(off, np.uint32)


# ---- the way back ---------------------------------------------------------------------------------------------------------

def _aligned(pos, length, what):
    """(POS, CIGAR) of a read of `length` bases whose first base stands at `pos`: bases in front of the transcript are soft-clipped"""
    if pos >= 0:
        return pos + 1, b"%dM" % length
    if -pos >= length:
        raise ValueError(f"{what}: a read of {length} bases at position {pos} has no base on the transcript: SAM cannot say that")
    return 1, b"%dS%dM" % (-pos, length + pos)


def write_sam(path, names, ref_len, hits, offsets, *, read_names=None, seqs=None, bgzf=False):
    """Hit records as SAM text at `path` (host side): @HD and @SQ lines, then per read mate 1 and mate 2 of every pair record, one
    line per orphan or single-end record (0x100 from the read's second record on), and 77 / 141 lines (single end: one 4 line) for
    a read with no record.  CIGAR is <len>M (<clip>S<rest>M where the read begins in front of the transcript), SEQ is '*' unless
    `seqs` gives, per read, the bases (single end) or a (mate 1, mate 2) pair, written as given.  `read_names`: per read, default
    r<index>.  The library is taken as paired when any record is, or, without records, when seqs holds pairs.  bgzf=True writes
    blocked gzip (gzfile.write_bgzf).  What SAM does not carry is lost: mate_len of an orphan."""
    hits = np.asarray(hits).view(HIT_DTYPE).reshape(-1)
    off = np.asarray(offsets).astype(np.int64)
    paired = bool((hits["mate_status"] != 0).any()) if len(hits) else bool(seqs and isinstance(seqs[0], tuple))
    nm = _name_bytes(names)
    out = [b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n"]
    out += [b"@SQ\tSN:%s\tLN:%d\n" % (n, int(l)) for n, l in zip(nm, ref_len)]
    line = b"%s\t%d\t%s\t%d\t255\t%s\t%s\t%d\t%d\t%s\t*\n"
    for r in range(len(off) - 1):
        q = _name_bytes([read_names[r]])[0] if read_names is not None else b"r%d" % r
        s = seqs[r] if seqs is not None else (b"*", b"*") if paired else b"*"
        s1, s2 = s if paired else (s, None)
        recs = hits[off[r]:off[r + 1]].tolist()
        if not recs:
            out.append(line % (q, 77, b"*", 0, b"*", b"*", 0, 0, s1) + line % (q, 141, b"*", 0, b"*", b"*", 0, 0, s2) if paired
                       else line % (q, 4, b"*", 0, b"*", b"*", 0, 0, s1))
        for i, (tid, pos, mpos, frag, rlen, mlen, fwd, mfwd, status, _) in enumerate(recs):
            sec = 0x100 if i else 0
            what = f"read {r}, record {i}"
            p1, c1 = _aligned(pos, rlen, what)
            if status == 3:
                p2, c2 = _aligned(mpos, mlen, what)
                tlen = frag if pos <= mpos else -frag
                out.append(line % (q, 0x1 | 0x2 | 0x40 | sec | (0 if fwd else 0x10) | (0 if mfwd else 0x20), nm[tid], p1, c1, b"=", p2, tlen, s1))
                out.append(line % (q, 0x1 | 0x2 | 0x80 | sec | (0 if mfwd else 0x10) | (0 if fwd else 0x20), nm[tid], p2, c2, b"=", p1, -tlen, s2))
            elif status:
                out.append(line % (q, 0x1 | 0x8 | (0x40 if status == 1 else 0x80) | sec | (0 if fwd else 0x10), nm[tid], p1, c1, b"*", 0, 0,
                                   s1 if status == 1 else s2))
            else:
                out.append(line % (q, sec | (0 if fwd else 0x10), nm[tid], p1, c1, b"*", 0, 0, s1))
    data = b"".join(out)
    if bgzf:
        from . import gzfile
        gzfile.write_bgzf(path, data)
    else:
        with open(path, "wb") as f:
            f.write(data)


# ---- the device reader ----------------------------------------------------------------------------------------------------

class SamFile:
    """A SAM file (plain, BGZF or gzip) read through the device parser: iterating yields (hits: uint8 device tensor [n_hits * 24] of
    HIT_DTYPE records, offsets: int32 device tensor [n_reads + 1], starting at 0 in every batch), one batch per block of the file.

    `names`: the transcript names in index order; default: the file's @SQ lines (read_header).  `paired`: the library's rules
    (csrc/samfmt.h).  `inflate` and block_bytes as readfile.ReadFile takes them.  `stats` counts lines, header lines, reads, hits,
    pairs and blocks (parse calls that emitted a batch or ended the file) and sums the device times.  A malformed line raises
    ValueError naming the path, the 1-based line number in the file and the kind; the batch that holds it is not emitted."""

    def __init__(self, path, device="cuda", paired=True, names=None, block_bytes=32 << 20, inflate="auto"):
        import torch

        from . import _lib, readfile
        if inflate not in ("auto", "host", "device"):
            raise ValueError("inflate must be 'auto', 'host' or 'device'")
        self.path, self.device, self.paired = str(path), torch.device(device), bool(paired)
        if names is None:
            names, _ = read_header(self.path)
            if not names:
                raise ValueError(f"{self.path}: no @SQ lines: give the transcript names (names=)")
        self._L = _lib.lib()
        with open(self.path, "rb") as f:
            head = f.read(4096)
        gzipped = head[:2] == b"\x1f\x8b"
        bgzf = gzipped and readfile.bgzf_member_bytes(head) is not None
        self.inflate = None if not gzipped else "device" if inflate == "device" or (inflate == "auto" and bgzf) else "host"
        self.stats = dict(lines=0, header_lines=0, reads=0, hits=0, pairs=0, blocks=0, calls=0, bytes_parsed=0, ms_copy=0.0, ms_kernels=0.0,
                          ms_inflate=0.0, bytes_compressed=0, members=0, chunks=0, candidates=0, false_starts=0, ms_find=0.0, ms_decode=0.0,
                          ms_propagate=0.0, ms_emit=0.0)
        nb = _name_bytes(names)
        blob = np.frombuffer(b"".join(nb), np.uint8)
        off = np.concatenate([[0], np.cumsum([len(x) for x in nb], dtype=np.int64)]).astype(np.int64)
        d_blob = torch.from_numpy(blob.copy()).to(self.device) if blob.size else None
        d_off = torch.from_numpy(off).to(self.device)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._L.sfgpu_sam_open(C.byref(self._h), _lib.ptr(d_blob), _lib.ptr(d_off), len(nb), int(self.paired), _lib.current_stream_ptr())
        if rc == _lib.ERR_INVALID:
            raise ValueError(f"{self.path}: {self._L.sfgpu_last_error().decode('utf-8', 'replace')}")
        _lib.check(rc)
        if self.inflate == "device":
            self._f = open(self.path, "rb", buffering=0)
            self._carry = (readfile.DeviceInflate if bgzf else readfile.DeviceGunzip)(self, self._f, block_bytes)
        else:
            self._f = gzip.open(self.path, "rb") if gzipped else open(self.path, "rb", buffering=0)
            self._carry = readfile.BlockCarry(self._f, block_bytes, self.path)

    def _call(self, n, final, call):
        """one parse call over n bytes -> readfile.Parsed; call(hits, cap_hits, off, cap_reads, res) -> rc"""
        import torch

        from . import _lib, readfile
        cap_reads = n // 11 + 1                            # a read has a line, a line ten tabs and (but for the last) a '\n'
        cap_hits = n // 64 + 1024                          # a guess: the call says what it needs
        off = torch.empty(cap_reads + 1, dtype=torch.int32, device=self.device)
        res = _lib.SamResult()
        with torch.cuda.device(self.device):
            for _ in range(2):
                hits = torch.empty(cap_hits * 24, dtype=torch.uint8, device=self.device)
                rc = call(hits, cap_hits, off, cap_reads, res)
                if rc != _lib.ERR_CAPACITY or res.need_reads > cap_reads:
                    break
                cap_hits = int(res.need_hits)
        if rc == _lib.ERR_FORMAT and res.bad:
            raise _malformed(self.path, self.stats["lines"] + int(res.bad_line) + 1, int(res.bad))
        _lib.check(rc)
        st = self.stats
        st["calls"] += 1; st["ms_copy"] += res.ms_copy; st["ms_kernels"] += res.ms_kernels
        if not (res.n_reads or final):
            return readfile.Parsed(0, 0)                   # no whole group yet: the carrier presents more
        for k, v in (("lines", res.n_lines), ("header_lines", res.n_header), ("reads", res.n_reads), ("hits", res.n_hits), ("pairs", res.n_pairs),
                     ("blocks", 1), ("bytes_parsed", res.consumed)):
            st[k] += int(v)
        return readfile.Parsed(int(res.n_reads), int(res.consumed), (hits[: int(res.n_hits) * 24].clone(), off[: int(res.n_reads) + 1].clone()))

    def _parse_host(self, text, final, _max_reads):
        from . import _lib
        n = int(text.size)
        return self._call(n, final, lambda hits, ch, off, cr, res: self._L.sfgpu_sam_parse_host(
            self._h, _lib.ptr(text), n, int(final), _lib.ptr(hits), ch, _lib.ptr(off), cr, C.byref(res), _lib.current_stream_ptr()))

    def _parse_device(self, text, lo, hi, final, _max_reads, _records):
        from . import _lib
        n = hi - lo
        if lo % 16:                                        # the parser wants its text at a 16-byte boundary
            text[:n] = text[lo:hi].clone()
            self._carry.lo, self._carry.hi, lo, hi = 0, n, 0, n
        view = text[lo:]
        out = self._call(n, final, lambda hits, ch, off, cr, res: self._L.sfgpu_sam_parse_device(
            self._h, _lib.ptr(view), n, view.numel(), int(final), _lib.ptr(hits), ch, _lib.ptr(off), cr, C.byref(res), _lib.current_stream_ptr()))
        if out.n_reads and not final:
            self._carry.starved = True                     # what is left is one group that has not ended: inflate before the next call
        return out

    def __iter__(self):
        if self._h is None:
            raise ValueError("the SAM file is closed")
        try:
            while True:
                res = self._carry.next(1 << 62) if self.inflate == "device" else self._carry.next(self._parse_host, 1 << 62)
                if res is None:
                    break
                yield res.payload
        finally:
            self.close()

    def close(self):
        if self._h is not None:
            import torch
            with torch.cuda.device(self.device):
                self._L.sfgpu_sam_close(self._h)
            self._h = None
            self._f.close()
            if self.inflate == "device":
                self._carry.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001  (interpreter shutdown)
            pass
