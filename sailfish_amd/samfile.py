"""A mapper's SAM file in, hit records on the device out: the file side of sfgpu_sam_parse_host / _device (csrc/samtext.hip; what a
SAM file says to this library is csrc/samfmt.h, and `read_sam_host` below is the contract both are judged by).

`SamFile` reads the file in blocks through the carriers of `readfile` (plain text and host-inflated gzip through pinned blocks,
BGZF and -- with inflate="device" -- ordinary gzip inflated on the device and parsed where they land) and iterates the
`(hits, offsets)` batches that `hits.filter_hits` and `quant.quantify` take.  Nothing of the alignment lines is parsed on the host.
The header is: `read_header` reads the @SQ lines with Python, they are a thousandth of a real file.

The file must be grouped by read name, as mappers write it (all lines of a fragment follow each other), unless it is read with
`collate=True`: then the lines may stand in any order -- a position-sorted file, what `samtools sort` leaves -- and the whole file
is collected on the device, grouped by QNAME exactly and paired through the mate fields (csrc/samcfmt.h, csrc/samcollate.hip;
`read_sam_collated_host` / `read_bam_collated_host` are the contract).  `write_sam` is the way back: hit records as SAM text, the host statement (`_sam_text`); `SamDeviceWriter` writes the same
file from the device mapper's batches where they lie (sfgpu_sam_write_text, csrc/samtext_write.hip, rules in csrc/samwfmt.h).

BAM (what `samtools view -b` makes of the same alignments) is read too: a BGZF file whose first member inflates to "BAM\1".  What
its record stream says is csrc/bamfmt.h, `read_bam_host` is the contract, the device side is csrc/bamtext.hip behind
sfgpu_bam_parse_host / _device, and `SamFile` picks the format by itself (`SamFile.format`).  `sam_to_bam`, `bam_to_sam` and
`write_bam` are host-side converters, for tests and for the way back."""
import ctypes as C
import gzip
import os
import re
import struct

import numpy as np

from .hits import HIT_DTYPE

BAD_FIELDS, BAD_NUMBER, BAD_FLAG, BAD_RNAME, BAD_CIGAR, BAD_LENGTH = 1, 2, 4, 8, 16, 32
BAD_QNAME = 64                                         # the collated reading only (COLLATED_KINDS)
KINDS = {BAD_FIELDS: "fewer than 11 tab-separated fields",
         BAD_NUMBER: "FLAG is not a number up to 65535, or POS of a mapped line is not a number in 1 .. 2^31 - 1",
         BAD_FLAG: "the FLAG does not fit the library: a paired call needs 0x1 and exactly one of 0x40 / 0x80, a single-end call no 0x1",
         BAD_RNAME: "RNAME is not one of the transcript names",
         BAD_CIGAR: "CIGAR is neither '*' nor a run of (1-9 digits, one of MIDNSHP=X)",
         BAD_LENGTH: "the read is longer than 65535 bases, or SEQ and CIGAR disagree about its length"}
BAM_KINDS = {BAD_FIELDS: "block_size is below 32 or below what l_read_name, n_cigar_op and l_seq need, the name is empty or lacks its NUL, "
                         "or the file ends inside the record",
             BAD_NUMBER: "pos of a mapped record is not in 0 .. 2^31 - 2",
             BAD_FLAG: KINDS[BAD_FLAG],
             BAD_RNAME: "refID of a mapped record is not in 0 .. n_ref - 1, or its reference is not one of the transcript names",
             BAD_CIGAR: "a CIGAR op code above 8",
             BAD_LENGTH: "the read is longer than 65535 bases, or l_seq and the CIGAR disagree about its length"}
# what the collated reading (collate=True) adds to KINDS: PNEXT is read, QNAME is bounded
COLLATED_KINDS = {**KINDS,
                  BAD_NUMBER: KINDS[BAD_NUMBER] + ", or (collated, paired) PNEXT of a mapped line is not a number in 0 .. 2^31 - 1",
                  BAD_QNAME: "QNAME is longer than 254 bytes"}
BAM_MAGIC = b"BAM\x01"
_CIGAR = re.compile(rb"(?:[0-9]{1,9}[MIDNSHP=X])+")
_CIGAR_OP = re.compile(rb"([0-9]+)([MIDNSHP=X])")
_LEAD = re.compile(rb"(?:[0-9]+H)*((?:[0-9]+S)*)")


def _malformed(path, line, kind):
    return ValueError(f"{path}: line {line} is malformed: {KINDS[kind]} (kind {kind})")


def _malformed_collated(path, line, kind):
    return ValueError(f"{path}: line {line} is malformed: {COLLATED_KINDS[kind]} (kind {kind})")


def _malformed_bam(path, record, kind):
    return ValueError(f"{path}: record {record} is malformed: {BAM_KINDS[kind]} (kind {kind})")


def is_bam(path):
    """a gzip (BGZF, as a rule) file whose first bytes inflate to the BAM magic"""
    with open(path, "rb") as f:
        if f.read(2) != b"\x1f\x8b":
            return False
    try:
        with gzip.open(path, "rb") as f:
            return f.read(4) == BAM_MAGIC
    except (OSError, EOFError):
        return False


def _open_text(path):
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(path, "rb") if gz else open(path, "rb")


def read_header(path):
    """(names, lengths) of the @SQ lines (SN:, LN:) in front of the first alignment line, in file order; plain or gzip.  Of a BAM
    file: its binary reference list (read_bam_header)."""
    if is_bam(path):
        return read_bam_header(path)[:2]
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


# ---- the BAM contract -------------------------------------------------------------------------------------------------------

def _bam_header(data):
    """the header of an inflated BAM stream -> (names, lengths, header_bytes, text), or None when `data` ends inside it"""
    if len(data) < 4:
        return None
    if data[:4] != BAM_MAGIC:
        raise ValueError("not a BAM stream: it does not begin with 'BAM\\1'")
    if len(data) < 12:
        return None
    p = 8 + struct.unpack_from("<I", data, 4)[0]
    if len(data) < p + 4:
        return None
    text, n_ref = bytes(data[8:p]), struct.unpack_from("<I", data, p)[0]
    p += 4
    names, lengths = [], []
    for _ in range(n_ref):
        if len(data) < p + 4:
            return None
        l_name = struct.unpack_from("<I", data, p)[0]
        if len(data) < p + 4 + l_name + 4:
            return None
        if l_name == 0:
            raise ValueError("a BAM reference without a name")
        names.append(bytes(data[p + 4:p + 4 + l_name - 1]).decode("utf-8", "surrogateescape"))
        lengths.append(struct.unpack_from("<I", data, p + 4 + l_name)[0])
        p += 4 + l_name + 4
    return names, lengths, p, text


def read_bam_header(path):
    """(names, lengths, header_bytes, text) of a BAM file: the reference list in file order, the length of the binary header in
    the inflated stream, and the SAM header text it carries.  Members are inflated on the host (zlib, through gzip) until the
    header is whole: it is a thousandth of the file, like the @SQ lines."""
    with gzip.open(path, "rb") as f:
        data, want = b"", 1 << 16
        while True:
            more = f.read(want - len(data))
            data += more
            try:
                head = _bam_header(data)
            except ValueError as e:
                raise ValueError(f"{path}: {e}") from None
            if head is not None:
                return head
            if not more:
                raise ValueError(f"{path}: the file ends inside the BAM header")
            want *= 2


def _parse_record(data, p, ref_tid, paired):
    """the record at p, whole in data -> (kind, None) or (0, (qname, mapped, side, tid, pos, read_len, fwd)): csrc/bamfmt.h"""
    block_size, ref, pos, l_name, _mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiiBBHHHI", data, p)
    if block_size < 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq or l_name == 0 or data[p + 36 + l_name - 1] != 0:
        return BAD_FIELDS, None
    qname, bad = bytes(data[p + 36:p + 36 + l_name - 1]), 0
    first, second = bool(flag & 0x40), bool(flag & 0x80)
    if (not flag & 0x1 or first == second) if paired else flag & 0x1:
        bad |= BAD_FLAG
    side = (1 if first else 2) if paired else 0
    if flag & (0x4 | 0x800):
        return bad, (qname, False, side, 0, 0, 0, not flag & 0x10)
    if not 0 <= pos <= 2 ** 31 - 2:
        bad |= BAD_NUMBER
    tid = ref_tid[ref] if 0 <= ref < len(ref_tid) else None
    if tid is None:
        bad |= BAD_RNAME
    ops = [(w >> 4, w & 15) for w in struct.unpack_from("<%dI" % n_cigar, data, p + 36 + l_name)]
    read_len = lead = 0
    if any(op > 8 for _, op in ops):
        bad |= BAD_CIGAR
    else:
        qlen = sum(n for n, op in ops if op in (0, 1, 4, 7, 8))            # M I S = X
        k = 0
        while k < len(ops) and ops[k][1] == 5:                             # the leading H ...
            k += 1
        while k < len(ops) and ops[k][1] == 4:                             # ... and the S behind them
            lead += ops[k][0]
            k += 1
        read_len = l_seq if l_seq else qlen
        if read_len > 65535 or (l_seq and n_cigar and l_seq != qlen):
            bad |= BAD_LENGTH
    if bad:
        return bad & -bad, None
    return 0, (qname, True, side, tid, pos - lead, read_len, not flag & 0x10)


def read_bam_host(data, names, paired, path="<bam>", counts=None):
    """The rules for BAM, on the host, written to be read: `data` (bytes: a whole inflated BAM stream, header included) -> what
    read_sam_host returns.  The record chain is walked from the header's end; a record whose block_size is below 32, or that the
    stream ends in, is BAD_FIELDS.  Raises the ValueError SamFile raises (lowest malformed record, 1-based; first broken rule).
    `counts` receives lines (= records) / header (0) / reads / hits / pairs."""
    data = bytes(data)
    head = _bam_header(data)
    if head is None:
        raise ValueError(f"{path}: the file ends inside the BAM header")
    refs, _, p, _ = head
    tid_of = {nm: i for i, nm in enumerate(_name_bytes(names))}
    ref_tid = [tid_of.get(r) for r in _name_bytes(refs)]
    groups, n = [], 0
    while p < len(data):
        n += 1
        if len(data) - p < 4:
            raise _malformed_bam(path, n, BAD_FIELDS)
        block_size = struct.unpack_from("<i", data, p)[0]
        if block_size < 32 or p + 4 + block_size > len(data):
            raise _malformed_bam(path, n, BAD_FIELDS)
        kind, rec = _parse_record(data, p, ref_tid, paired)
        if kind:
            raise _malformed_bam(path, n, kind)
        if groups and groups[-1][-1][0] == rec[0]:
            groups[-1].append(rec)
        else:
            groups.append([rec])
        p += 4 + block_size
    recs, off = [], [0]
    for g in groups:
        recs.extend(_group_records(g, paired))
        off.append(len(recs))
    if counts is not None:
        counts.update(lines=n, header=0, reads=len(groups), hits=len(recs), pairs=sum(r[8] == 3 for r in recs))
    return np.array(recs, dtype=HIT_DTYPE), np.array(off, np.uint32)


# ---- the collated contract (csrc/samcfmt.h) -----------------------------------------------------------------------------------

def _line_mate(line, paired):
    """what the collated reading adds to _parse_line for one non-header line -> (kinds, POS, PNEXT): the BAD_* bits it adds, the
    written POS of a mapped line, and PNEXT when the line names a mate (else 0).  A line that is BAD_FIELDS or whose FLAG is no
    number is not looked at (it is malformed already, by an earlier rule)."""
    f = line.split(b"\t")
    if len(f) < 11 or not (f[1].isdigit() and len(f[1]) <= 5 and int(f[1]) <= 65535):
        return 0, 0, 0
    flag, bad = int(f[1]), 0
    if len(f[0]) > 254:
        bad |= BAD_QNAME
    if flag & (0x4 | 0x800):
        return bad, 0, 0
    pos = int(f[3]) if f[3].isdigit() and len(f[3]) <= 10 and 1 <= int(f[3]) <= 2 ** 31 - 1 else 0      # (else BAD_NUMBER already)
    if not paired:
        return bad, pos, 0
    if not (f[7].isdigit() and len(f[7]) <= 10 and int(f[7]) <= 2 ** 31 - 1):
        return bad | BAD_NUMBER, pos, 0
    names_mate = not flag & 0x8 and f[6] in (b"=", f[2]) and int(f[7]) >= 1
    return bad, pos, int(f[7]) if names_mate else 0


def _record_mate(data, p, paired):
    """the same for the BAM record at p (mapped, well-formed) -> (POS, PNEXT or 0)"""
    _bs, ref, pos, _l, _mq, _bin, _nc, flag, _ls, nref, npos = struct.unpack_from("<iiiBBHHHIii", data, p)
    names_mate = paired and not flag & 0x8 and nref == ref and npos >= 0
    return pos + 1, npos + 1 if names_mate else 0


def _collated_records(lines, paired):
    """the records of one fragment: lines = [(rec, POS, PNEXT)] in file order, rec as _parse_line returns it"""
    pairs = []
    if paired:
        by_key = {}                                   # (tid, POS of mate 1, POS of mate 2) -> (side-1 lines, side-2 lines), file order
        for n, (l, pos, pnext) in enumerate(lines):
            if l[1] and pnext:
                key = (l[3], pos, pnext) if l[2] == 1 else (l[3], pnext, pos)
                by_key.setdefault(key, ([], []))[l[2] - 1].append(n)
        for ones, twos in by_key.values():
            for na, nb in zip(ones, twos):            # the i-th with the i-th; what is left over pairs with nothing
                a, b = lines[na][0], lines[nb][0]
                frag = max(a[4] + a[5], b[4] + b[5]) - min(a[4], b[4])
                pairs.append((na, (a[3], a[4], b[4], frag, a[5], b[5], a[6], b[6], 3, 0)))
    if pairs:
        return [r for _, r in sorted(pairs, key=lambda x: (x[1][0], x[0]))]      # tid, then the side-1 line's place in the file
    singles = [(l[3], l[4], 0, 0, l[5], 0, l[6], 0, l[2], 0) for l, _, _ in lines if l[1]]
    return sorted(singles, key=lambda r: (r[8] == 2, r[0]))


def _collated_result(frags, paired, counts, n_lines, n_header):
    recs, off = [], [0]
    for g in frags.values():                          # (a dict keeps the order of first insertion: of the fragments' first lines)
        recs.extend(_collated_records(g, paired))
        off.append(len(recs))
    if counts is not None:
        counts.update(lines=n_lines, header=n_header, reads=len(frags), hits=len(recs), pairs=sum(r[8] == 3 for r in recs))
    return np.array(recs, dtype=HIT_DTYPE), np.array(off, np.uint32)


def read_sam_collated_host(data, names, paired, path="<sam>", counts=None):
    """The rules of the collated reading (csrc/samcfmt.h), on the host, written to be read: what read_sam_host returns, for a text
    whose lines may stand in any order.  ALL non-header lines with byte-equal QNAME are one fragment, numbered by their first
    lines; a mapped line of a paired call NAMES A MATE iff FLAG lacks 0x8, RNEXT is "=" or its RNAME, and PNEXT >= 1; a side-1 line a
    and a side-2 line b of a fragment pair when both are mapped on one transcript, both name a mate, a.PNEXT == b.POS and
    b.PNEXT == a.POS (the written POS), the i-th such a with the i-th such b in file order.  What a fragment yields, and in which
    order, is read_sam_host's.  Raises the ValueError SamFile(collate=True) raises."""
    tid_of = {nm: i for i, nm in enumerate(_name_bytes(names))}
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    frags, n_header = {}, 0
    for n, line in enumerate(lines, 1):
        if line.endswith(b"\r"):
            line = line[:-1]
        if line.startswith(b"@"):
            n_header += 1
            continue
        kind, rec = _parse_line(line, tid_of, paired)
        more, pos, pnext = _line_mate(line, paired)
        kind |= more
        if kind:
            raise _malformed_collated(path, n, kind & -kind)
        frags.setdefault(rec[0], []).append((rec, pos, pnext))
    return _collated_result(frags, paired, counts, len(lines), n_header)


def read_bam_collated_host(data, names, paired, path="<bam>", counts=None):
    """The same for an inflated BAM stream: read_bam_host's walk of the record chain, read_sam_collated_host's fragments and pairs.
    A record names a mate iff FLAG lacks 0x8, next_refID == refID and next_pos >= 0; POS and PNEXT are pos + 1 and next_pos + 1."""
    data = bytes(data)
    head = _bam_header(data)
    if head is None:
        raise ValueError(f"{path}: the file ends inside the BAM header")
    refs, _, p, _ = head
    tid_of = {nm: i for i, nm in enumerate(_name_bytes(names))}
    ref_tid = [tid_of.get(r) for r in _name_bytes(refs)]
    frags, n = {}, 0
    while p < len(data):
        n += 1
        if len(data) - p < 4:
            raise _malformed_bam(path, n, BAD_FIELDS)
        block_size = struct.unpack_from("<i", data, p)[0]
        if block_size < 32 or p + 4 + block_size > len(data):
            raise _malformed_bam(path, n, BAD_FIELDS)
        kind, rec = _parse_record(data, p, ref_tid, paired)
        if kind:
            raise _malformed_bam(path, n, kind)
        pos, pnext = _record_mate(data, p, paired) if rec[1] else (0, 0)
        frags.setdefault(rec[0], []).append((rec, pos, pnext))
        p += 4 + block_size
    return _collated_result(frags, paired, counts, n, 0)


def header_sort_order(path):
    """the SO: tag of the @HD line of a SAM file (plain or gzip) or of the header text a BAM file carries, e.g. "coordinate",
    "queryname", "unsorted"; None without an @HD line or without the tag"""
    if is_bam(path):
        lines = read_bam_header(path)[3].split(b"\n")
    else:
        lines = []
        with _open_text(path) as f:
            for line in f:
                if not line.startswith(b"@"):
                    break
                lines.append(line)
    for line in lines:
        fields = line.rstrip(b"\r\n").split(b"\t")
        if fields[0] == b"@HD":
            for x in fields[1:]:
                if x.startswith(b"SO:"):
                    return x[3:].decode("utf-8", "surrogateescape")
            return None
    return None


# ---- SAM text <-> BAM stream (host) ------------------------------------------------------------------------------------------

_OPS = b"MIDNSHP=X"
_BASES = b"=ACMGRSVTWYHKDBN"
_BASE_CODE = {c: i for i, c in enumerate(_BASES)}
_TAG_INT = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}


def _reg2bin(beg, end):
    """the SAM specification's bin of the zero-based half-open interval [beg, end)"""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def sam_to_bam(text):
    """SAM text -> the uncompressed BAM stream of the same alignments.  The references are the @SQ lines, every '@' line goes into
    the header text; bin is the specification's reg2bin, SEQ is 4-bit packed, QUAL '*' becomes 0xFF bytes.  Optional fields of the
    types A, i, f and Z are converted; any other, a QNAME above 254 bytes, or a line the SAM rules reject is a ValueError."""
    lines = bytes(text).split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    lines = [l[:-1] if l.endswith(b"\r") else l for l in lines]
    head = [l for l in lines if l.startswith(b"@")]
    refs = []
    for l in head:
        if l.startswith(b"@SQ\t"):
            tags = {x[:2]: x[3:] for x in l.split(b"\t")[1:] if x[2:3] == b":"}
            if b"SN" not in tags or not tags.get(b"LN", b"").isdigit():
                raise ValueError("an @SQ line without SN: and a numeric LN:")
            refs.append((tags[b"SN"], int(tags[b"LN"])))
    tid_of = {nm: i for i, (nm, _) in enumerate(refs)}
    htext = b"".join(l + b"\n" for l in head)
    out = [BAM_MAGIC, struct.pack("<I", len(htext)), htext, struct.pack("<I", len(refs))]
    out += [struct.pack("<I", len(nm) + 1) + nm + b"\0" + struct.pack("<I", ln) for nm, ln in refs]
    for n, l in enumerate(lines, 1):
        if l.startswith(b"@"):
            continue
        f = l.split(b"\t")
        flag = int(f[1]) if len(f) > 1 and f[1].isdigit() and len(f[1]) <= 5 else 0
        kind, _ = _parse_line(l, tid_of, bool(flag & 0x1))
        if kind:
            raise ValueError(f"line {n} is malformed: {KINDS[kind]} (kind {kind})")
        qname, rname, cigar, rnext, seq, qual = f[0], f[2], f[5], f[6], f[9], f[10]
        if not 1 <= len(qname) <= 254:
            raise ValueError(f"line {n}: a QNAME of {len(qname)} bytes does not fit BAM")
        try:
            pos, mapq, pnext, tlen = int(f[3]) - 1, int(f[4]), int(f[7]) - 1, int(f[8])
            ref = -1 if rname == b"*" else tid_of[rname]
            nref = -1 if rnext == b"*" else ref if rnext == b"=" else tid_of[rnext]
        except (ValueError, KeyError):
            raise ValueError(f"line {n}: POS, MAPQ, PNEXT or TLEN is no number, or RNAME / RNEXT is no @SQ name") from None
        ops = [] if cigar == b"*" else [(int(c), _OPS.index(op)) for c, op in _CIGAR_OP.findall(cigar)]
        if cigar != b"*" and (not _CIGAR.fullmatch(cigar) or len(ops) > 65535 or any(c >= 1 << 28 for c, _ in ops)):
            raise ValueError(f"line {n}: the CIGAR does not fit BAM")
        ref_len = sum(c for c, op in ops if op in (0, 2, 3, 7, 8))
        bases = b"" if seq == b"*" else seq
        if qual != b"*" and len(qual) != len(bases):
            raise ValueError(f"line {n}: SEQ and QUAL differ in length")
        packed = bytearray((len(bases) + 1) // 2)
        for i, c in enumerate(bases.upper()):
            packed[i >> 1] |= _BASE_CODE.get(c, 15) << (0 if i & 1 else 4)
        tags = []
        for t in f[11:]:
            if len(t) < 5 or t[2:3] != b":" or t[4:5] != b":" or t[3:4] not in b"AifZ":
                raise ValueError(f"line {n}: the optional field {t!r} is not of type A, i, f or Z")
            ty, v = t[3:4], t[5:]
            try:
                if ty == b"A" and len(v) == 1:
                    tags.append(t[:2] + b"A" + v)
                elif ty == b"i":
                    x = int(v)
                    code = next(c for c, (lo, hi) in ((b"c", (-128, 127)), (b"C", (0, 255)), (b"s", (-32768, 32767)), (b"S", (0, 65535)),
                                                      (b"i", (-2 ** 31, 2 ** 31 - 1)), (b"I", (0, 2 ** 32 - 1))) if lo <= x <= hi)
                    tags.append(t[:2] + code + struct.pack(_TAG_INT[code], x))
                elif ty == b"f":
                    tags.append(t[:2] + b"f" + struct.pack("<f", float(v)))
                elif ty == b"Z":
                    tags.append(t[:2] + b"Z" + v + b"\0")
                else:
                    raise ValueError
            except (ValueError, StopIteration):
                raise ValueError(f"line {n}: the optional field {t!r} is ill-formed") from None
        body = b"".join([struct.pack("<iiBBHHHIiii", ref, pos, len(qname) + 1, mapq & 255,
                                     _reg2bin(pos, pos + max(ref_len, 1)) if pos >= 0 else 4680, len(ops), flag, len(bases), nref, pnext, tlen),
                         qname, b"\0", struct.pack("<%dI" % len(ops), *[c << 4 | op for c, op in ops]), bytes(packed),
                         b"\xff" * len(bases) if qual == b"*" else bytes(q - 33 for q in qual)] + tags)
        out += [struct.pack("<i", len(body)), body]
    return b"".join(out)


def _tag_text(data, p, end):
    """the optional fields in data[p:end] as SAM text fields"""
    out = []
    while p < end:
        tag, ty = bytes(data[p:p + 2]), bytes(data[p + 2:p + 3])
        p += 3
        if ty == b"A":
            out.append(tag + b":A:" + bytes(data[p:p + 1])); p += 1
        elif ty in _TAG_INT:
            out.append(tag + b":i:%d" % struct.unpack_from(_TAG_INT[ty], data, p)[0]); p += struct.calcsize(_TAG_INT[ty])
        elif ty == b"f":
            out.append(tag + b":f:" + repr(struct.unpack_from("<f", data, p)[0]).encode()); p += 4
        elif ty in (b"Z", b"H"):
            e = data.index(b"\0", p)
            out.append(tag + b":" + ty + b":" + bytes(data[p:e])); p = e + 1
        elif ty == b"B":
            sub, count = bytes(data[p:p + 1]), struct.unpack_from("<I", data, p + 1)[0]
            fmt = "<f" if sub == b"f" else _TAG_INT[sub]
            vals = struct.unpack_from("<%d%s" % (count, fmt[1]), data, p + 5)
            out.append(tag + b":B:" + sub + b"".join(b",%s" % repr(v).encode() for v in vals)); p += 5 + count * struct.calcsize(fmt)
        else:
            raise ValueError(f"an optional field of the unknown type {ty!r}")
    return out


def bam_to_sam(data):
    """an inflated BAM stream -> SAM text (host): the header text, then one line per record"""
    data = bytes(data)
    head = _bam_header(data)
    if head is None:
        raise ValueError("the stream ends inside the BAM header")
    refs, _, p, text = head
    refs = _name_bytes(refs)
    out = [text if not text or text.endswith(b"\n") else text + b"\n"]
    while p < len(data):
        block_size, ref, pos, l_name, mapq, _bin, n_cigar, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiiBBHHHIiii", data, p)
        end = p + 4 + block_size
        if block_size < 32 or end > len(data):
            raise ValueError(f"the record at byte {p} of the stream is broken")
        q = p + 36
        qname = data[q:q + l_name - 1]; q += l_name
        cigar = b"".join(b"%d%c" % (w >> 4, _OPS[w & 15]) for w in struct.unpack_from("<%dI" % n_cigar, data, q)) or b"*"; q += 4 * n_cigar
        seq = bytes(_BASES[data[q + (i >> 1)] >> (0 if i & 1 else 4) & 15] for i in range(l_seq)) or b"*"; q += (l_seq + 1) // 2
        qual = b"*" if l_seq == 0 or data[q] == 0xff else bytes(x + 33 for x in data[q:q + l_seq]); q += l_seq
        rname = refs[ref] if ref >= 0 else b"*"
        rnext = b"*" if nref < 0 else b"=" if nref == ref else refs[nref]
        out.append(b"\t".join([qname, b"%d" % flag, rname, b"%d" % (pos + 1), b"%d" % mapq, cigar, rnext, b"%d" % (npos + 1), b"%d" % tlen, seq, qual]
                              + _tag_text(data, q, end)) + b"\n")
        p = end
    return b"".join(out)


# ---- the way back ---------------------------------------------------------------------------------------------------------

def _aligned(pos, length, what):
    """(POS, CIGAR) of a read of `length` bases whose first base stands at `pos`: bases in front of the transcript are soft-clipped"""
    if pos >= 0:
        return pos + 1, b"%dM" % length
    if -pos >= length:
        raise ValueError(f"{what}: a read of {length} bases at position {pos} has no base on the transcript: SAM cannot say that")
    return 1, b"%dS%dM" % (-pos, length + pos)


# the complement of csrc/samwfmt.h's samw_comp: the bytes named change, in either case; S, W, N and every other byte stay
_COMP = bytes.maketrans(b"ACGTURYKMBDHVacgturykmbdhv", b"TGCAAYRMKVHDBtgcaayrmkvhdb")


def _alignment_arrays(alignments, n_records):
    """(pos, op_off, ops) as numpy arrays from what hits.align_hits / hits.align_hits_host return -- (pos, nm, op_off, ops, ...),
    device tensors or arrays, two slots per record"""
    def host(a, dtype):
        return (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)).view(dtype).reshape(-1)
    pos, op_off, ops = host(alignments[0], np.int32), host(alignments[2], np.uint64), host(alignments[3], np.uint32)
    if len(pos) != 2 * n_records or len(op_off) != 2 * n_records + 1:
        raise ValueError(f"an alignment of {len(pos)} slots for {n_records} records (two slots a record)")
    return pos, op_off, ops


def _cigar_text(words):
    return b"".join(b"%d%c" % (int(w) >> 4, _OPS[int(w) & 15]) for w in words)


def _tag_arrays(tags, n_records):
    """(nm, md_off, md) as numpy arrays from what hits.md_tags / hits.md_tags_host return, device tensors or arrays, two slots per record"""
    def host(a, dtype):
        return (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)).view(dtype).reshape(-1)
    nm, md_off, md = host(tags[0], np.uint32), host(tags[1], np.uint64), host(tags[2], np.uint8)
    if len(nm) != 2 * n_records or len(md_off) != 2 * n_records + 1:
        raise ValueError(f"tags of {len(nm)} slots for {n_records} records (two slots a record)")
    return nm, md_off, md.tobytes()


def _posterior_values(posteriors, n_records):
    """the records' posterior probabilities as a float64 array, from what hits.posteriors / hits.posteriors_host return (p first), device
    tensors or arrays"""
    p = posteriors[0]
    p = (p.cpu().numpy() if hasattr(p, "cpu") else np.asarray(p)).astype(np.float64).reshape(-1)
    if len(p) != n_records:
        raise ValueError(f"posteriors of {len(p)} records for {n_records} records")
    return p


def _sam_text(names, ref_len, hits, offsets, read_names, seqs, *, quals=None, oriented=False, alignments=None, tags=None, posteriors=None):
    """the text write_sam writes.  quals: per read the quality bytes (single end) or a (mate 1, mate 2) pair, a mate's None for
    "not given" (QUAL '*'); they go with the mate's SEQ on every line.  oriented: a line with 0x10 carries SEQ reverse-complemented
    and QUAL reversed.  alignments: what hits.align_hits / align_hits_host returned for the same records -- a mapped line then takes
    POS and CIGAR from its slot (2 * record + line) and PNEXT from the other line's slot, and a slot without an operation is the
    "no base on the transcript" error.  tags: what hits.md_tags / md_tags_host returned for the same records and the same alignments --
    a mapped line then ends NM:i:<nm>, MD:Z:<md>, NH:i:<the read's records>; they describe the read on the transcript's strand, so the
    text must be oriented and the bases given.  posteriors: what hits.posteriors / posteriors_host returned for the same records (the
    values p first: (p,) will do) -- a mapped line then ends, behind the tags, ZW:f:<"%g" % p of its record>, both lines of a pair
    alike; the lines of a read without records carry nothing.  The rules are stated in csrc/samwfmt.h."""
    if quals is not None and seqs is None:
        raise ValueError("qualities of reads whose bases are not given")
    if tags is not None and (seqs is None or not oriented):
        raise ValueError("tags describe the read on the transcript's strand: they need seqs= and oriented=True")
    hits = np.asarray(hits).view(HIT_DTYPE).reshape(-1)
    off = np.asarray(offsets).astype(np.int64)
    paired = bool((hits["mate_status"] != 0).any()) if len(hits) else bool(seqs and isinstance(seqs[0], tuple))
    nm = _name_bytes(names)
    out = [b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n"]
    out += [b"@SQ\tSN:%s\tLN:%d\n" % (n, int(l)) for n, l in zip(nm, ref_len)]
    fmt = b"%s\t%d\t%s\t%d\t255\t%s\t%s\t%d\t%d\t%s\t%s\n"
    aln = _alignment_arrays(alignments, int(off[-1]) if len(off) else 0) if alignments is not None else None
    tg = _tag_arrays(tags, int(off[-1]) if len(off) else 0) if tags is not None else None
    zw = _posterior_values(posteriors, int(off[-1]) if len(off) else 0) if posteriors is not None else None

    def tagged(text, h, which, nh):
        """a mapped line with its slot's tags and its record's posterior"""
        if tg is not None:
            slot = 2 * h + which
            text = text[:-1] + b"\tNM:i:%d\tMD:Z:%s\tNH:i:%d\n" % (int(tg[0][slot]), tg[2][int(tg[1][slot]):int(tg[1][slot + 1])], nh)
        if zw is not None:
            text = text[:-1] + b"\tZW:f:%s\n" % (b"%g" % float(zw[h]))
        return text

    def placed(h, which, pos, length, what):
        """(POS, CIGAR) of line `which` of record h"""
        if aln is None:
            return _aligned(pos, length, what)
        slot = 2 * h + which
        words = aln[2][int(aln[1][slot]):int(aln[1][slot + 1])]
        if not len(words):
            raise ValueError(f"{what}: the alignment has no operation, so {WRITE_KINDS[1]}")
        return int(aln[0][slot]) + 1, _cigar_text(words)

    def line(q, flag, rname, p, cigar, rnext, pnext, tlen, sq):
        """sq: the mate's (SEQ, QUAL or None)"""
        s, ql = sq
        if ql is None:
            ql = b"*"
        if oriented and flag & 0x10:
            s, ql = (s if s == b"*" and seqs is None else s.translate(_COMP)[::-1]), (ql if sq[1] is None else ql[::-1])
        return fmt % (q, flag, rname, p, cigar, rnext, pnext, tlen, s, ql)

    def check_quals(r, mates):
        """QUAL_WRITE_KINDS 6, reported as record 0 of the read: behind a record 0 that breaks another rule, in front of any later record"""
        for _, ql in mates:
            if ql is not None and any(not 33 <= c <= 126 for c in ql):
                raise ValueError(f"read {r}, record 0: {QUAL_WRITE_KINDS[6]}")

    for r in range(len(off) - 1):
        q = _name_bytes([read_names[r]])[0] if read_names is not None else b"r%d" % r
        s = seqs[r] if seqs is not None else (b"*", b"*") if paired else b"*"
        s1, s2 = s if paired else (s, None)
        k = quals[r] if quals is not None else (None, None) if paired else None
        k1, k2 = k if paired else (k, None)
        for sq, ql in ((s1, k1), (s2, k2)):
            if ql is not None and len(ql) != len(sq):
                raise ValueError(f"read {r}: {len(ql)} qualities for {len(sq)} bases")
        s1, s2 = (s1, k1), (s2, k2)
        recs = hits[off[r]:off[r + 1]].tolist()
        if not recs:
            check_quals(r, (s1, s2))
            out.append(line(q, 77, b"*", 0, b"*", b"*", 0, 0, s1) + line(q, 141, b"*", 0, b"*", b"*", 0, 0, s2) if paired
                       else line(q, 4, b"*", 0, b"*", b"*", 0, 0, s1))
        for i, (tid, pos, mpos, frag, rlen, mlen, fwd, mfwd, status, _) in enumerate(recs):
            sec = 0x100 if i else 0
            what = f"read {r}, record {i}"
            hi, nh = int(off[r]) + i, len(recs)
            p1, c1 = placed(int(off[r]) + i, 0, pos, rlen, what)
            if status == 3:
                p2, c2 = placed(int(off[r]) + i, 1, mpos, mlen, what)
            rname = nm[tid]
            if i == 0:
                check_quals(r, (s1, s2))
            if status == 3:
                tlen = frag if pos <= mpos else -frag
                out.append(tagged(line(q, 0x1 | 0x2 | 0x40 | sec | (0 if fwd else 0x10) | (0 if mfwd else 0x20), rname, p1, c1, b"=", p2, tlen, s1), hi, 0, nh))
                out.append(tagged(line(q, 0x1 | 0x2 | 0x80 | sec | (0 if mfwd else 0x10) | (0 if fwd else 0x20), rname, p2, c2, b"=", p1, -tlen, s2), hi, 1, nh))
            elif status:
                out.append(tagged(line(q, 0x1 | 0x8 | (0x40 if status == 1 else 0x80) | sec | (0 if fwd else 0x10), rname, p1, c1, b"*", 0, 0,
                                       s1 if status == 1 else s2), hi, 0, nh))
            else:
                out.append(tagged(line(q, sec | (0 if fwd else 0x10), rname, p1, c1, b"*", 0, 0, s1), hi, 0, nh))
    return b"".join(out)


def write_sam(path, names, ref_len, hits, offsets, *, read_names=None, seqs=None, bgzf=False, quals=None, oriented=False, alignments=None, tags=None,
              posteriors=None):
    """Hit records as SAM text at `path` (host side): @HD and @SQ lines, then per read mate 1 and mate 2 of every pair record, one
    line per orphan or single-end record (0x100 from the read's second record on), and 77 / 141 lines (single end: one 4 line) for
    a read with no record.  CIGAR is <len>M (<clip>S<rest>M where the read begins in front of the transcript), SEQ is '*' unless
    `seqs` gives, per read, the bases (single end) or a (mate 1, mate 2) pair; QUAL is '*' unless `quals` gives the qualities the
    same way (a mate's None: not given).  Both are written as given unless `oriented`: then a line with 0x10 carries SEQ
    reverse-complemented and QUAL reversed, as the SAM specification stores them.  A quality byte outside '!' .. '~' is a ValueError
    (QUAL_WRITE_KINDS); a 1-base read whose quality is '*' reads as "no qualities", the format's ambiguity.  `read_names`: per read, default
    r<index>.  The library is taken as paired when any record is, or, without records, when seqs holds pairs.  bgzf=True writes
    blocked gzip (gzfile.write_bgzf).  What SAM does not carry is lost: mate_len of an orphan.  `alignments`: the gapped alignment
    of the same records (hits.align_hits / align_hits_host): POS, CIGAR and PNEXT are then the alignment's.  `tags`: the NM / MD tags
    of the same records and alignments (hits.md_tags / md_tags_host): a mapped line then ends NM:i:, MD:Z: and NH:i: (the read's record
    count); they need `seqs` and `oriented`.  `posteriors`: the records' posterior probabilities (hits.posteriors / posteriors_host): a
    mapped line then ends ZW:f:<"%g" of its record's value>."""
    data = _sam_text(names, ref_len, hits, offsets, read_names, seqs, quals=quals, oriented=oriented, alignments=alignments, tags=tags, posteriors=posteriors)
    if bgzf:
        from . import gzfile
        gzfile.write_bgzf(path, data)
    else:
        with open(path, "wb") as f:
            f.write(data)


def write_bam(path, names, ref_len, hits, offsets, *, read_names=None, seqs=None, member_bytes=65280, quals=None, oriented=False, sort=None,
              alignments=None, tags=None, posteriors=None):
    """Hit records as a BAM file at `path` (host side): sam_to_bam of the text write_sam writes for the same arguments, in BGZF
    members of member_bytes bytes with the EOF member behind them (gzfile.write_bgzf).  sort="coordinate": the same records in
    coordinate order under an @HD SO:coordinate header (sort_bam_stream; csrc/baifmt.h), the header in members of its own, so that
    the first record begins a member; `build_bai` gives its index."""
    from . import gzfile
    if sort not in SORT_ORDERS:
        raise ValueError(f"sort must be one of {SORT_ORDERS}, not {sort!r}")
    data = sam_to_bam(_sam_text(names, ref_len, hits, offsets, read_names, seqs, quals=quals, oriented=oriented, alignments=alignments, tags=tags,
                                posteriors=posteriors))
    if sort is None:
        gzfile.write_bgzf(path, data, member_bytes=member_bytes)
        return
    data = sort_bam_stream(data)
    p = _bam_header(data)[2]
    with open(path, "wb") as f:
        for part in (data[:p], data[p:]):
            for a in range(0, len(part), member_bytes):
                f.write(gzfile.bgzf_member(part[a:a + member_bytes]))
        f.write(gzfile.BGZF_EOF)


# ---- the coordinate-sorted file and its index (csrc/baifmt.h; host statements) ---------------------------------------------------

SORT_ORDERS = (None, "coordinate")
_HD_COORDINATE = b"@HD\tVN:1.6\tSO:coordinate\n"
BAI_MAGIC = b"BAI\x01"
_PSEUDO_BIN = 37450
_REF_OPS = (0, 2, 3, 7, 8)                              # M D N = X consume the reference


def _bam_records(data, p):
    """the offsets of the records of the inflated stream `data` from p on; ValueError where the chain breaks"""
    out = []
    while p < len(data):
        if len(data) - p < 36:
            raise ValueError(f"the stream ends inside the record at byte {p}")
        block_size = struct.unpack_from("<i", data, p)[0]
        if block_size < 32 or p + 4 + block_size > len(data):
            raise ValueError(f"the record at byte {p} of the stream is broken")
        out.append(p)
        p += 4 + block_size
    return out


def _sort_key(data, p):
    ref, pos = struct.unpack_from("<ii", data, p + 4)
    return (ref & 0xffffffff) << 32 | ((pos + 1) & 0xffffffff)


def sort_bam_stream(data):
    """an inflated BAM stream -> the coordinate-sorted stream of the same records: the header text begins with @HD VN:1.6
    SO:coordinate (in place of an @HD line, if there is one), the records stand in stable order of
    (uint32)refID << 32 | (uint32)(pos + 1) -- records without a reference last, ties in the order they had."""
    data = bytes(data)
    head = _bam_header(data)
    if head is None:
        raise ValueError("the stream ends inside the BAM header")
    _, _, p, text = head
    lines = [l for l in text.split(b"\n") if l]
    if lines and lines[0].startswith(b"@HD"):
        lines.pop(0)
    at = _bam_records(data, p)
    order = sorted(range(len(at)), key=lambda i: _sort_key(data, at[i]))       # (sorted is stable)
    ends = at[1:] + [len(data)]
    return sam_to_bam(_HD_COORDINATE + b"".join(l + b"\n" for l in lines)) + b"".join(data[at[i]:ends[i]] for i in order)


def _bgzf_member_at(blob, c):
    """the member at byte c of a BGZF file -> (its bytes, its payload)"""
    import zlib
    if len(blob) - c < 18 or bytes(blob[c:c + 4]) != b"\x1f\x8b\x08\x04":
        raise ValueError(f"no BGZF member at byte {c}")
    xlen = struct.unpack_from("<H", blob, c + 10)[0]
    q, size = c + 12, None
    while q + 4 <= c + 12 + xlen:
        si, slen = bytes(blob[q:q + 2]), struct.unpack_from("<H", blob, q + 2)[0]
        if si == b"BC" and slen == 2:
            size = struct.unpack_from("<H", blob, q + 4)[0] + 1
        q += 4 + slen
    if size is None or c + size > len(blob):
        raise ValueError(f"the member at byte {c} has no BSIZE, or the file ends inside it")
    return size, zlib.decompress(bytes(blob[c + 12 + xlen:c + size - 8]), -15)


def _bgzf_members(blob):
    """[(file offset, first payload byte in the stream)] of every member, the stream, and the offset of the EOF member (the file's
    last empty member; the file's length without one)"""
    members, parts, c, n = [], [], 0, 0
    while c < len(blob):
        size, payload = _bgzf_member_at(blob, c)
        members.append((c, n, len(payload)))
        parts.append(payload)
        c += size
        n += len(payload)
    eof = members[-1][0] if members and members[-1][2] == 0 else len(blob)
    return members, b"".join(parts), eof


def _ref_end(data, p):
    """(beg, end) of the record at p: end = pos + the reference-consuming CIGAR lengths, at least beg + 1"""
    pos, l_name, _mq, _bin, n_cigar = struct.unpack_from("<iBBHH", data, p + 8)
    span = sum(w >> 4 for w in struct.unpack_from("<%dI" % n_cigar, data, p + 36 + l_name) if w & 15 in _REF_OPS)
    return pos, pos + max(span, 1)


def build_bai(bam_path_or_bytes):
    """The BAI index (bytes) of a coordinate-sorted BAM file, given as a path or as the file's bytes: the SAM specification's index
    with every choice fixed (csrc/baifmt.h), the statement the device index is judged by.  The members are inflated with zlib and
    walked with the records.  V(x) of stream byte x is coffset(member holding x) << 16 | offset in its payload, V(end of the stream)
    = coffset(EOF member) << 16.  A record with refID >= 0 spans [pos, pos + reference-consuming CIGAR lengths) (at least one base)
    and lies in bin reg2bin of that; a maximal run of records consecutive in the file with the same (refID, bin) is one chunk, and
    nothing else is merged.  Per reference: the bins ascending with their chunks in file order, pseudo-bin 37450 with (V(first
    record), V(end of the last)) and (mapped, unmapped by FLAG 0x4), then the linear index of ((max end - 1) >> 14) + 1 windows:
    the smallest vbeg of the records touching the window, an untouched window taking the next touched one to its right.  Then
    n_no_coor.  Raises ValueError if the keys (uint32)refID << 32 | (uint32)(pos + 1) ever descend."""
    import bisect
    blob = bam_path_or_bytes
    if not isinstance(blob, (bytes, bytearray, memoryview)):
        with open(blob, "rb") as f:
            blob = f.read()
    members, data, eof = _bgzf_members(blob)
    head = _bam_header(data)
    if head is None:
        raise ValueError("the file ends inside the BAM header")
    refs, _, p, _ = head
    starts = [m[1] for m in members]

    def v(x):
        if x >= len(data):
            return eof << 16
        m = bisect.bisect_right(starts, x) - 1           # the last member that starts at or before x: never an empty one
        return members[m][0] << 16 | (x - members[m][1])

    per = [dict(bins={}, lin=[], n=[0, 0], span=None) for _ in refs]
    no_coor, last, last_bin = 0, 0, None
    for n, q in enumerate(_bam_records(data, p)):
        ref, flag = struct.unpack_from("<i", data, q + 4)[0], struct.unpack_from("<H", data, q + 18)[0]
        key = _sort_key(data, q)
        if key < last:
            raise ValueError(f"record {n} stands behind a record of a higher (reference, position): the file is not coordinate-sorted")
        last = key
        if ref < 0:
            no_coor += 1
            continue
        if ref >= len(refs):
            raise ValueError(f"record {n}: refID {ref} is no reference")
        beg, end = _ref_end(data, q)
        vbeg, vend = v(q), v(q + 4 + struct.unpack_from("<i", data, q)[0])
        R, b = per[ref], _reg2bin(beg, end)
        chunks = R["bins"].setdefault(b, [])
        if last_bin == (ref, b):
            chunks[-1][1] = vend
        else:
            chunks.append([vbeg, vend])
        last_bin = (ref, b)
        R["span"] = [vbeg if R["span"] is None else R["span"][0], vend]
        R["n"][1 if flag & 0x4 else 0] += 1
        w1 = (end - 1) >> 14
        R["lin"] += [None] * (w1 + 1 - len(R["lin"]))
        for w in range(beg >> 14, w1 + 1):
            if R["lin"][w] is None or vbeg < R["lin"][w]:
                R["lin"][w] = vbeg
    out = [BAI_MAGIC, struct.pack("<I", len(refs))]
    for R in per:
        out.append(struct.pack("<I", len(R["bins"]) + 1 if R["span"] else 0))
        for b in sorted(R["bins"]):
            out.append(struct.pack("<II", b, len(R["bins"][b])) + b"".join(struct.pack("<QQ", *c) for c in R["bins"][b]))
        if R["span"]:
            out.append(struct.pack("<IIQQQQ", _PSEUDO_BIN, 2, *R["span"], *R["n"]))
        lin = R["lin"]
        for w in range(len(lin) - 2, -1, -1):
            if lin[w] is None:
                lin[w] = lin[w + 1]
        out.append(struct.pack("<I", len(lin)) + struct.pack("<%dQ" % len(lin), *lin))
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def reg2bins(beg, end):
    """the SAM specification's bins that may hold a record overlapping the zero-based half-open [beg, end)"""
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins += range(first + (beg >> shift), first + (end >> shift) + 1)
    return bins


def read_bai(bai):
    """BAI bytes -> per reference (bins {bin: [(vbeg, vend)]}, the pseudo-bin not among them; linear index; pseudo-bin chunks or
    None), and n_no_coor (None where the file ends without it)"""
    bai = bytes(bai)
    if bai[:4] != BAI_MAGIC:
        raise ValueError("not a BAI index: it does not begin with 'BAI\\1'")
    n_ref, p, refs = struct.unpack_from("<I", bai, 4)[0], 8, []
    for _ in range(n_ref):
        n_bin, bins, pseudo = struct.unpack_from("<I", bai, p)[0], {}, None
        p += 4
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<II", bai, p)
            chunks = [struct.unpack_from("<QQ", bai, p + 8 + 16 * k) for k in range(n_chunk)]
            p += 8 + 16 * n_chunk
            if b == _PSEUDO_BIN:
                pseudo = chunks
            else:
                bins[b] = chunks
        n_intv = struct.unpack_from("<I", bai, p)[0]
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, bai, p + 4)), pseudo))
        p += 4 + 8 * n_intv
    return refs, struct.unpack_from("<Q", bai, p)[0] if len(bai) >= p + 8 else None


def fetch(bam_path, name_or_tid, beg, end, bai=None):
    """The records (bytes each, block_size included, in file order) of the coordinate-sorted BAM file at bam_path that overlap the
    zero-based half-open region [beg, end) of a reference, named or numbered, found through the index: `bai` is the index's bytes or
    its path, default bam_path + ".bai".  The bins of reg2bins(beg, end) give the chunks, chunks that end at or before the linear
    index's entry for beg >> 14 are dropped, every other chunk is sought (the member at vbeg >> 16 is inflated, records are read
    from byte vbeg & 0xffff on, across members, until vend) and its records are kept when they lie on the reference, begin before
    `end` and end behind `beg`.  Host only: a convenience, and the check that an index can be used."""
    names = read_bam_header(bam_path)[0]
    tid = name_or_tid if isinstance(name_or_tid, int) else names.index(name_or_tid if isinstance(name_or_tid, str) else name_or_tid.decode("utf-8", "surrogateescape"))
    if not 0 <= tid < len(names):
        raise ValueError(f"reference {tid} of {len(names)}")
    if bai is None:
        bai = bam_path + ".bai"
    if not isinstance(bai, (bytes, bytearray, memoryview)):
        with open(bai, "rb") as f:
            bai = f.read()
    refs, _ = read_bai(bai)
    if len(refs) != len(names):
        raise ValueError(f"the index holds {len(refs)} references, the file {len(names)}")
    bins, lin, _ = refs[tid]
    beg = max(int(beg), 0)
    if beg >= end or (beg >> 14) >= len(lin):           # (a record that overlaps the region touches window beg >> 14 or a later one)
        return []
    min_off = lin[beg >> 14]
    chunks = sorted(c for b in reg2bins(beg, end) for c in bins.get(b, ()) if c[1] > min_off)
    out = []
    with open(bam_path, "rb") as f:
        size = f.seek(0, 2)

        def member(c):
            f.seek(c)
            head = f.read(18)
            if len(head) < 18:
                return 0, b""
            xlen = struct.unpack_from("<H", head, 10)[0]
            blob = head + f.read(12 + xlen - 18 + 65536)
            return _bgzf_member_at(blob, 0)

        for vbeg, vend in chunks:
            c, u = vbeg >> 16, vbeg & 0xffff
            msize, payload = member(c)
            while True:
                while u >= len(payload) and msize and c + msize < size:       # on to the member that holds the next byte
                    c, u = c + msize, u - len(payload)
                    msize, payload = member(c)
                if u >= len(payload) or (c << 16 | u) >= vend:
                    break
                rec = bytearray()
                need = 4
                while len(rec) < need:                  # the record may straddle members
                    take = payload[u:u + need - len(rec)]
                    rec += take
                    u += len(take)
                    if len(rec) == 4 and need == 4:
                        need = 4 + struct.unpack_from("<i", rec, 0)[0]
                    if len(rec) < need and u >= len(payload):
                        if not msize or c + msize >= size:
                            raise ValueError(f"{bam_path}: the file ends inside a record")
                        c, u = c + msize, 0
                        msize, payload = member(c)
                rec = bytes(rec)
                ref = struct.unpack_from("<i", rec, 4)[0]
                b0, b1 = _ref_end(rec, 0)
                if ref == tid and b0 < end and b1 > beg:
                    out.append(rec)
    return out


# ---- the way back, on the device ------------------------------------------------------------------------------------------

# SamDeviceWriter(format=): plain text; the same text in BGZF members encoded on the device; BAM records, likewise
WRITE_FORMATS = ("sam", "sam.gz", "bam")
_SAMW_FORMAT = {"sam.gz": 0, "bam": 1}                     # SFGPU_SAMW_TEXT, SFGPU_SAMW_BAM (include/sfgpu.h)
WRITE_KINDS = {1: "the read has no base on the transcript: SAM cannot say that", 2: "the transcript index is not below the number of names"}
# what qualities add (quals=; csrc/samwfmt.h), in either format: reported as record 0 of the lowest read that holds such a byte
QUAL_WRITE_KINDS = {6: "a quality byte is not in '!' .. '~': SAM cannot say that"}
# what format="bam" adds (csrc/bamwfmt.h), behind WRITE_KINDS where one record breaks several
BAM_WRITE_KINDS = {3: "the read name is not of 1 .. 254 bytes: BAM cannot say that",
                   4: "the bases given differ in number from the record's read length, or are more than 65535: BAM cannot say that",
                   5: "the alignment ends beyond 2^29: BAM cannot say that"}


def sam_header(names, ref_len, sort=None):
    """the @HD and @SQ lines _sam_text begins with; sort="coordinate": the @HD line of the sorted file (csrc/baifmt.h)"""
    return (_HD_COORDINATE if sort else b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n") + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, int(l)) for n, l in zip(_name_bytes(names), ref_len))


class SamDeviceWriter:
    """The SAM file write_sam writes, formatted on the device from the mapper's batches where they lie (sfgpu_sam_write_text,
    csrc/samtext_write.hip; what a line says is csrc/samwfmt.h, and `_sam_text` is the statement it is judged by).

    `path_or_file`: a path, or a binary file object (left open by close()).  `names`, `ref_len`: the transcripts in index order;
    the constructor writes the @HD / @SQ lines from the host.  `paired`: the library (decides what a read without records gives).
    `write(hits, offsets)` takes one batch as QuasiIndex.map_reads and SamFile return it (uint8 device tensor of HIT_DTYPE records,
    int32 device tensor [reads + 1]) and appends its lines, in whole-unit chunks of chunk_bytes (0: the library's 32 MiB).
      read_names  a (uint8 bytes, 64-bit offsets [reads + 1]) pair of device tensors, or a list of names (packed with
                  quantfile.names_blob and uploaded); default r<index>, the index counted over all batches written so far.
      seqs        the (bases, int64 offsets) device pair of readfile.ReadFile.read / mapper.pack_sequences, or (paired) a pair of such
                  pairs; default '*'.
      quals       the qualities that go with `seqs`: a device uint8 tensor that shares the bases' offsets (readfile.ReadFile's
                  last_quals), or (paired) a pair of them, either member None; default QUAL '*'.
      alignments  what hits.align_hits returned for the batch's records (pos, nm, op_off, ops, ...): a mapped line then takes POS
                  and CIGAR from its slot, PNEXT from the other line's; a slot without an operation is WRITE_KINDS[1]; default: the
                  recorded diagonal, <len>M at pos.
    Bases and qualities are written as given, also on 0x10 lines, unless `oriented=True`: then a 0x10 line carries SEQ
    reverse-complemented and QUAL reversed (the SAM specification's orientation, what other tools expect).
    A record SAM cannot express (WRITE_KINDS) raises ValueError naming the lowest such read -- counted over all batches, as
    write_sam counts it -- and record; nothing of that batch is written.
    `format`: "sam" (the default) writes the text as it is.  "sam.gz" writes the same text, @HD / @SQ lines included, as a BGZF
    file whose members are encoded on the device (gzfile.BgzfDeviceWriter; csrc/bgzf_write.hip): the formatted chunks go from
    the formatter to the encoder on the device, only compressed bytes are copied; close() writes the EOF member and adds
    bytes_out, members, stored_members, matches, literals, ms_encode and chunks_out to `stats`.  "bam" writes the BAM file
    write_bam writes (sam_to_bam of the same text: magic, header text, reference list, one record per line; csrc/bamwfmt.h) through
    the same encoder; BAM_WRITE_KINDS are then errors too, a read without records counting as record 0.  `stats` sums reads, hits, lines, bytes, chunks, batches and the device / copy / sink times.
    `sort`: None (the default) writes the records in read order, as above.  "coordinate" (format="bam" only, else ValueError) writes
    the file write_bam(sort="coordinate") writes (csrc/baifmt.h, csrc/bamsort.hip): write() has the same signature, checks and
    errors, but formats the batch's records and KEEPS them on the device (a failing batch keeps nothing); close() sorts them stably
    by (uint32)refID << 32 | (uint32)(pos + 1), gathers the sorted stream in pieces of chunk_bytes rounded down to a multiple of
    32 768 (the file does not depend on it), encodes them behind the @HD SO:coordinate header and builds the BAI index on the
    device.  `index`: a path or a binary file object (left open) for the index; None: path + ".bai" when path_or_file is a path, no
    index when it is a file object; False: no index.  The state is NOT spilled to the host: it takes the records' bytes plus 20
    bytes per record of device memory until close(), which adds 28 bytes per record, two pieces and, for the index, 40 bytes per
    record and 28 per chunk; fewer than 2^32 records.  `stats` gains records, state_bytes (peak device bytes held), no_coor,
    index_bytes, ms_sort, ms_gather and ms_index.
    write(tags=): the batch's NM / MD tags as hits.md_tags returns them (nm, md_off, md: device tensors, two slots per record, computed
    over the same `alignments`); a mapped line then ends NM:i:<nm>, MD:Z:<md>, NH:i:<the read's record count> (a BAM record: NM and NH
    in the smallest integer type that holds them, MD as a Z string), in every format, sorted or not.  The writer must be oriented and
    the bases given, else ValueError.  Without `tags` the bytes are what they were.
    write(posteriors=): what hits.posteriors returned for the batch's records (p, rec, f32, ...: device tensors, one entry per record);
    a mapped line then ends, behind the tags where there are any, ZW:f:<"%g" of its record's posterior probability> (a BAM record:
    ZW as a float), in every format, sorted or not.  Without `posteriors` the bytes are what they were."""

    def __init__(self, path_or_file, names, ref_len, paired, *, chunk_bytes=0, format="sam", oriented=False, sort=None, index=None):
        from . import _lib, quantfile
        if format not in WRITE_FORMATS:
            raise ValueError(f"format must be one of {WRITE_FORMATS}, not {format!r}")
        if sort not in SORT_ORDERS:
            raise ValueError(f"sort must be one of {SORT_ORDERS}, not {sort!r}")
        if sort is not None and format != "bam":
            raise ValueError(f'sort="coordinate" needs format="bam", not {format!r}')
        self._sort, self._b = sort is not None, None
        self._L = _lib.lib()
        self.paired, self.chunk_bytes, self.format, self.oriented = bool(paired), int(chunk_bytes), format, bool(oriented)
        self._names = quantfile.names_blob(_name_bytes(names))
        self._n_refs = len(self._names[1]) - 1
        self._d_names = None                               # uploaded to the device of the first batch
        self._own = not hasattr(path_or_file, "write")
        self._index = None                                 # where the BAI goes: a path, a file object or None
        if self._sort and index is not False:
            self._index = index if index is not None else (os.fsdecode(path_or_file) + ".bai" if self._own else None)
        self._f = open(path_or_file, "wb") if self._own else path_or_file
        self.n_reads = 0                                   # the running read index
        self.stats = dict(reads=0, hits=0, lines=0, bytes=0, chunks=0, batches=0, ms_format=0.0, ms_copy=0.0, ms_sink=0.0)
        head = sam_header(names, ref_len, sort)
        if format == "bam":
            head = sam_to_bam(head)                        # magic, header text and reference list
        self.stats["header_bytes"] = len(head)
        self._z = None
        if format == "sam":
            self._f.write(head)
        else:                                              # the header goes through the encoder as the first write, once the device is known
            from . import gzfile
            self._z, self._head = gzfile.BgzfDeviceWriter(self._f, chunk_bytes=self.chunk_bytes), head

    def _write_head(self, dev):
        import torch

        from . import _lib
        if self._head is not None:
            head, self._head = self._head, None
            if self._sort:                                 # the index is made of the members' sizes: kept from the first member on
                self._z._open(dev)
                _lib.check(self._L.sfgpu_bgzw_track_members(self._z._h))
            self._z.write(torch.from_numpy(np.frombuffer(head, np.uint8).copy()).to(dev))

    @staticmethod
    def _blob(pair, dev):
        """(bytes, 64-bit offsets), host (bytes / numpy) or device tensors -> contiguous (uint8, int64) tensors on dev"""
        import torch
        b, o = pair
        if not isinstance(b, torch.Tensor):
            b = torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy())
        if not isinstance(o, torch.Tensor):
            o = torch.from_numpy(np.ascontiguousarray(o).view(np.int64).copy())
        if b.element_size() != 1 or o.is_floating_point() or o.element_size() != 8:
            raise TypeError("expected (bytes, 64-bit integer offsets)")
        return b.to(dev).contiguous(), o.to(dev).contiguous()

    def _batch_args(self, hits, offsets, read_names, seqs, quals, alignments):
        """write()'s arguments as the entries take them: (batch, keepalive) -- the _lib.SamwBatch and the tensors whose addresses it
        holds: the caller keeps `keepalive` referenced until the entry has returned."""
        import torch

        from . import _lib, quantfile
        dev = hits.device
        d_hits, d_off = hits.contiguous(), offsets.contiguous()
        n = int(d_off.numel()) - 1
        if self._d_names is None or self._d_names[0].device != dev:
            b, o = self._names
            self._d_names = self._blob((b, o), dev)
        q = (None, None)
        if read_names is not None:
            pair = read_names if isinstance(read_names, tuple) else quantfile.names_blob(_name_bytes(read_names))
            q = self._blob(pair, dev)
            if q[1].numel() != n + 1:
                raise ValueError(f"{q[1].numel() - 1} read names for {n} reads")
        s = [(None, None), (None, None)]
        if seqs is not None:
            mates = seqs if isinstance(seqs[0], (tuple, list)) else (seqs,)
            if len(mates) != (2 if self.paired else 1):
                raise ValueError("seqs: one (bases, offsets) pair for a single-end library, a pair of them for a paired one")
            for m, pair in enumerate(mates):
                s[m] = self._blob(pair, dev)
                if s[m][1].numel() != n + 1:
                    raise ValueError(f"bases of {s[m][1].numel() - 1} reads for {n} reads")
        ql = [None, None]
        if quals is not None:
            mates = tuple(quals) if isinstance(quals, (tuple, list)) else (quals,)
            if len(mates) != (2 if self.paired else 1):
                raise ValueError("quals: one tensor of quality bytes for a single-end library, a pair of them (either may be None) for a paired one")
            for m, t in enumerate(mates):
                if t is None:
                    continue
                if s[m][1] is None:
                    raise ValueError("qualities of a mate whose bases are not given")
                if not isinstance(t, torch.Tensor):
                    t = torch.from_numpy(np.frombuffer(bytes(t), np.uint8).copy())
                if t.element_size() != 1:
                    raise TypeError("quals: expected quality bytes")
                t = t.to(dev).contiguous().reshape(-1)
                if t.numel() != s[m][0].numel():
                    raise ValueError(f"{t.numel()} quality bytes for {s[m][0].numel()} bases")
                ql[m] = t if t.numel() else torch.zeros(1, dtype=torch.uint8, device=dev)     # no base at all: still "given"
        p = lambda t: _lib.ptr(t) if t is not None and t.numel() else None
        batch = _lib.SamwBatch(p(d_hits), _lib.ptr(d_off), n, int(self.paired), p(self._d_names[0]), _lib.ptr(self._d_names[1]), self._n_refs,
                               p(q[0]), p(q[1]), p(s[0][0]), p(s[0][1]), p(s[1][0]), p(s[1][1]), self.n_reads,
                               None if ql[0] is None else _lib.ptr(ql[0]), None if ql[1] is None else _lib.ptr(ql[1]), int(self.oriented))
        aln_t = None
        if alignments is not None:
            a_pos, a_off, a_ops = (alignments[i].to(dev).contiguous() for i in (0, 2, 3))
            if a_pos.element_size() != 4 or a_off.element_size() != 8 or a_ops.element_size() != 4:
                raise TypeError("alignments: expected what hits.align_hits returns (32-bit positions, 64-bit offsets, 32-bit operations)")
            n_rec = d_hits.numel() // 24
            if a_pos.numel() != 2 * n_rec or a_off.numel() != 2 * n_rec + 1:
                raise ValueError(f"an alignment of {a_pos.numel()} slots for {n_rec} records (two slots a record)")
            if not a_ops.numel():
                a_ops = torch.zeros(1, dtype=torch.int32, device=dev)          # no operation at all: still "given"
            if not a_pos.numel():
                a_pos = torch.zeros(1, dtype=torch.int32, device=dev)
            batch.aln_pos, batch.aln_op_off, batch.aln_ops = _lib.ptr(a_pos), _lib.ptr(a_off), _lib.ptr(a_ops)
            aln_t = (a_pos, a_off, a_ops)
        return batch, (d_hits, d_off, self._d_names, q, s, ql, aln_t)

    def _tag_args(self, batch, tags, hits, seqs):
        """write()'s tags into the batch's tag fields; returns the tensors whose addresses they hold"""
        import torch

        from . import _lib
        if not self.oriented:
            raise ValueError("tags describe the read on the transcript's strand: the writer must be oriented=True")
        if seqs is None:
            raise ValueError("tags of reads whose bases are not given")
        dev = hits.device
        t_nm, t_off, t_md = (tags[i].to(dev).contiguous() for i in (0, 1, 2))
        if t_nm.element_size() != 4 or t_off.element_size() != 8 or t_md.element_size() != 1:
            raise TypeError("tags: expected what hits.md_tags returns (32-bit nm, 64-bit offsets, MD bytes)")
        n_rec = hits.numel() // 24
        if t_nm.numel() != 2 * n_rec or t_off.numel() != 2 * n_rec + 1:
            raise ValueError(f"tags of {t_nm.numel()} slots for {n_rec} records (two slots a record)")
        if not t_md.numel():
            t_md = torch.zeros(1, dtype=torch.uint8, device=dev)               # no MD byte at all: still "given"
        if not t_nm.numel():
            t_nm = torch.zeros(1, dtype=torch.int32, device=dev)
        batch.tag_nm, batch.tag_md_off, batch.tag_md = _lib.ptr(t_nm), _lib.ptr(t_off), _lib.ptr(t_md)
        return t_nm, t_off, t_md

    @staticmethod
    def _post_args(batch, posteriors, hits):
        """write()'s posteriors into the batch's ZW fields; returns the tensors whose addresses they hold"""
        import torch

        from . import _lib
        dev = hits.device
        if len(posteriors) < 3:
            raise TypeError("posteriors: expected what hits.posteriors returns (p, rec, f32, ...)")
        z_rec, z_f32 = (posteriors[i].to(dev).contiguous() for i in (1, 2))
        if z_rec.element_size() != 4 or z_rec.is_floating_point() or z_f32.dtype != torch.float32:
            raise TypeError("posteriors: expected what hits.posteriors returns (32-bit records, float32 values)")
        n_rec = hits.numel() // 24
        if z_rec.numel() != n_rec or z_f32.numel() != n_rec:
            raise ValueError(f"posteriors of {z_rec.numel()} records for {n_rec} records")
        if not n_rec:                                                                  # no record at all: still "given"
            z_rec, z_f32 = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev)
        batch.tag_zw_rec, batch.tag_zw_f32 = _lib.ptr(z_rec), _lib.ptr(z_f32)
        return z_rec, z_f32

    def write(self, hits, offsets, *, read_names=None, seqs=None, quals=None, alignments=None, tags=None, posteriors=None):
        import torch

        from . import _lib
        if self._f is None:
            raise ValueError("the SAM writer is closed")
        dev = hits.device
        batch, keepalive = self._batch_args(hits, offsets, read_names, seqs, quals, alignments)
        n = batch.n_reads
        if tags is not None:
            keepalive = (keepalive, self._tag_args(batch, tags, hits, seqs))
        if posteriors is not None:
            keepalive = (keepalive, self._post_args(batch, posteriors, hits))
        raised = []

        def sink(addr, nb, _user):
            try:                                   # nothing may unwind through the C frame
                self._f.write(memoryview((C.c_char * nb).from_address(addr)))
                return 0
            except BaseException as e:             # noqa: BLE001  (re-raised below)
                raised.append(e)
                return 1

        res = _lib.SamWriteResult()
        with torch.cuda.device(dev):
            if self._z is None:
                rc = self._L.sfgpu_sam_write_text(C.byref(batch), self.chunk_bytes, _lib.TEXT_SINK(sink), None, C.byref(res), _lib.current_stream_ptr())
            elif self._sort:
                self._write_head(dev)
                self._open_store()
                rc = self._L.sfgpu_bamsort_collect(self._b, C.byref(batch), C.byref(res), _lib.current_stream_ptr())
            else:
                self._write_head(dev)
                rc = self._L.sfgpu_sam_write_bgzf(C.byref(batch), self.chunk_bytes, self._z._h, _SAMW_FORMAT[self.format], C.byref(res),
                                                  _lib.current_stream_ptr())
        sunk = raised if self._z is None else self._z._raised      # what this call's sink raised: the encoder's, when it does the sinking
        if sunk:
            raise sunk.pop(0)
        if rc == _lib.ERR_INVALID and res.error_kind:
            what = {**WRITE_KINDS, **BAM_WRITE_KINDS, **QUAL_WRITE_KINDS}[int(res.error_kind)]
            raise ValueError(f"read {self.n_reads + int(res.error_read)}, record {int(res.error_record)}: {what}")
        _lib.check(rc)
        del keepalive                              # (referenced up to here: the entry has returned)
        self.n_reads += n
        st = self.stats
        for k, v in (("reads", n), ("hits", hits.numel() // 24), ("lines", res.n_lines), ("bytes", res.n_bytes), ("chunks", res.n_chunks), ("batches", 1)):
            st[k] += int(v)
        st["ms_format"] += res.format_ms; st["ms_copy"] += res.d2h_ms; st["ms_sink"] += res.sink_ms
        return res.as_dict()

    def _open_store(self):
        from . import _lib
        if self._b is None:
            b = C.c_void_p()
            _lib.check(self._L.sfgpu_bamsort_open(C.byref(b)))
            self._b = b

    def _finish_sorted(self):
        """sort, gather and encode the records kept, then the index: everything of close() that is the sorted file's own"""
        import torch

        from . import _lib
        dev = self._z._device
        raised, own, xf = [], isinstance(self._index, (str, bytes, os.PathLike)), None

        def sink(addr, nb, _user):
            try:                                   # nothing may unwind through the C frame
                xf.write(memoryview((C.c_char * nb).from_address(addr)))
                return 0
            except BaseException as e:             # noqa: BLE001  (re-raised below)
                raised.append(e)
                return 1

        if self._index is not None:
            xf = open(self._index, "wb") if own else self._index
        try:
            res = _lib.BamsortResult()
            with torch.cuda.device(dev):
                self._open_store()
                rc = self._L.sfgpu_bamsort_finish(self._b, self._z._h, self._n_refs, self.chunk_bytes,
                                                  _lib.TEXT_SINK(sink) if xf is not None else _lib.TEXT_SINK(0), None, C.byref(res),
                                                  _lib.current_stream_ptr())
            for sunk in (raised, self._z._raised):
                if sunk:
                    raise sunk.pop(0)
            _lib.check(rc)
        finally:
            if xf is not None:
                xf.close() if own else xf.flush()
        for k, v in (("records", res.n_records), ("state_bytes", res.state_bytes), ("no_coor", res.n_no_coor), ("index_bytes", res.index_bytes),
                     ("ms_sort", res.sort_ms), ("ms_gather", res.gather_ms), ("ms_index", res.index_ms)):
            self.stats[k] = v

    def close(self):
        if self._f is None:
            return
        try:
            if self._z is not None:
                try:
                    if not self._z._raised and self._z._h is None:
                        import torch
                        self._write_head(torch.device("cuda", torch.cuda.current_device()))
                    try:
                        if self._sort and not self._z._raised:
                            self._finish_sorted()
                    finally:
                        b, self._b = self._b, None
                        if b is not None:
                            self._L.sfgpu_bamsort_close(b)
                        res = self._z.close()          # the EOF member
                finally:
                    self._z = None
                for k, v in (("bytes_out", res["n_bytes_out"]), ("members", res["n_members"]), ("stored_members", res["n_stored_members"]),
                             ("matches", res["n_matches"]), ("literals", res["n_literals"]), ("ms_encode", res["encode_ms"])):
                    self.stats[k] = v
                self.stats["ms_copy"] += res["d2h_ms"]; self.stats["ms_sink"] += res["sink_ms"]; self.stats["chunks_out"] = res["n_chunks"]
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


# ---- the device reader ----------------------------------------------------------------------------------------------------

class SamFile:
    """A SAM file (plain, BGZF or gzip) or a BAM file read through the device parser: iterating yields (hits: uint8 device tensor [n_hits * 24] of
    HIT_DTYPE records, offsets: int32 device tensor [n_reads + 1], starting at 0 in every batch), one batch per block of the file.

    `names`: the transcript names in index order; default: the file's @SQ lines (read_header).  `paired`: the library's rules
    (csrc/samfmt.h).  `inflate` and block_bytes as readfile.ReadFile takes them.  `stats` counts lines, header lines, reads, hits,
    pairs and blocks (parse calls that emitted a batch or ended the file) and sums the device times.  A malformed line raises
    ValueError naming the path, the 1-based line number in the file and the kind; the batch that holds it is not emitted.

    `format` says what the file is: "sam" or "bam" (a gzip file whose first bytes inflate to "BAM\1").  A BAM file goes through
    readfile.DeviceInflate and sfgpu_bam_parse_device (inflate "auto" or "device") or gzip, BlockCarry and sfgpu_bam_parse_host
    ("host", and whenever the gzip file is not BGZF); its reference list is the default for `names`, `lines` counts its alignment
    records (`header_lines` stays 0) and a malformed record is named by its 1-based number among them (BAM_KINDS).

    `collate`: False (the default) reads a name-grouped file as described.  True reads a file whose lines stand in any order -- a
    position-sorted one -- by the rules of csrc/samcfmt.h (read_sam_collated_host / read_bam_collated_host): iterating first runs
    the whole file through sfgpu_sam_collect_* / sfgpu_bam_collect_* (the same carriers, one call per block), which keeps 32 bytes
    and the QNAME of every alignment line on the device; sfgpu_samc_finish then groups the lines by QNAME exactly and pairs them
    through their mate fields, and the batches are slices of `batch_reads` fragments (sfgpu_samc_emit), numbered by their first
    lines.  "auto" collates iff the header says SO:coordinate (header_sort_order).  `collated` says what was decided.  `stats` then
    also holds fragments, sort_rounds, state_bytes (device memory held while the batches are emitted), ms_collect, ms_finish and
    ms_emit; `blocks` counts the collect calls that consumed something.  A malformed line raises the same ValueError (COLLATED_KINDS
    for SAM text) before any batch is emitted."""

    def __init__(self, path, device="cuda", paired=True, names=None, block_bytes=32 << 20, inflate="auto", collate=False, batch_reads=1_000_000):
        import torch

        from . import _lib, readfile
        if inflate not in ("auto", "host", "device"):
            raise ValueError("inflate must be 'auto', 'host' or 'device'")
        if collate not in (False, True, "auto"):
            raise ValueError("collate must be False, True or 'auto'")
        if int(batch_reads) < 1:
            raise ValueError("batch_reads must be at least 1")
        self.collated = header_sort_order(str(path)) == "coordinate" if collate == "auto" else bool(collate)
        self.batch_reads = int(batch_reads)
        self._c = None
        self.path, self.device, self.paired = str(path), torch.device(device), bool(paired)
        self.format = "bam" if is_bam(self.path) else "sam"
        if self.format == "bam":
            refs, _, header_bytes, _ = read_bam_header(self.path)
            names = refs if names is None else names
        elif names is None:
            names, _ = read_header(self.path)
            if not names:
                raise ValueError(f"{self.path}: no @SQ lines: give the transcript names (names=)")
        self._L = _lib.lib()
        with open(self.path, "rb") as f:
            head = f.read(4096)
        gzipped = head[:2] == b"\x1f\x8b"
        bgzf = gzipped and readfile.bgzf_member_bytes(head) is not None
        self.inflate = None if not gzipped else "device" if inflate == "device" or (inflate == "auto" and bgzf) else "host"
        if self.format == "bam" and not bgzf:
            self.inflate = "host"
        self.stats = dict(lines=0, header_lines=0, reads=0, hits=0, pairs=0, blocks=0, calls=0, bytes_parsed=0, ms_copy=0.0, ms_kernels=0.0,
                          ms_inflate=0.0, bytes_compressed=0, members=0, chunks=0, candidates=0, false_starts=0, ms_find=0.0, ms_decode=0.0,
                          ms_propagate=0.0, ms_emit=0.0)
        if self.collated:
            self.stats.update(fragments=0, sort_rounds=0, state_bytes=0, ms_collect=0.0, ms_finish=0.0)

        def on_device(items):
            nb = _name_bytes(items)
            blob = np.frombuffer(b"".join(nb), np.uint8)
            off = np.concatenate([[0], np.cumsum([len(x) for x in nb], dtype=np.int64)]).astype(np.int64)
            return torch.from_numpy(blob.copy()).to(self.device) if blob.size else None, torch.from_numpy(off).to(self.device), len(nb)

        d_blob, d_off, n_names = on_device(names)
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            if self.format == "bam":
                d_rblob, d_roff, n_ref = on_device(refs)
                rc = self._L.sfgpu_bam_open(C.byref(self._h), _lib.ptr(d_blob), _lib.ptr(d_off), n_names, _lib.ptr(d_rblob), _lib.ptr(d_roff), n_ref,
                                            header_bytes, int(self.paired), _lib.current_stream_ptr())
            else:
                rc = self._L.sfgpu_sam_open(C.byref(self._h), _lib.ptr(d_blob), _lib.ptr(d_off), n_names, int(self.paired), _lib.current_stream_ptr())
        if rc == _lib.ERR_INVALID:
            raise ValueError(f"{self.path}: {self._L.sfgpu_last_error().decode('utf-8', 'replace')}")
        _lib.check(rc)
        if self.collated:
            self._c = C.c_void_p()
            with torch.cuda.device(self.device):
                _lib.check(self._L.sfgpu_samc_open(C.byref(self._c), int(self.paired), _lib.current_stream_ptr()))
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
        # a read has a line, a line ten tabs and (but for the last) a '\n'; a BAM record has 36 bytes or more
        cap_reads = n // 36 + 1 if self.format == "bam" else n // 11 + 1
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
            raise (_malformed_bam if self.format == "bam" else _malformed)(self.path, self.stats["lines"] + int(res.bad_line) + 1, int(res.bad))
        _lib.check(rc)
        st = self.stats
        st["calls"] += 1; st["ms_copy"] += res.ms_copy; st["ms_kernels"] += res.ms_kernels
        if not (res.n_reads or final):
            return readfile.Parsed(0, 0)                   # no whole group yet: the carrier presents more
        for k, v in (("lines", res.n_lines), ("header_lines", res.n_header), ("reads", res.n_reads), ("hits", res.n_hits), ("pairs", res.n_pairs),
                     ("blocks", 1), ("bytes_parsed", res.consumed)):
            st[k] += int(v)
        return readfile.Parsed(int(res.n_reads), int(res.consumed), (hits[: int(res.n_hits) * 24].clone(), off[: int(res.n_reads) + 1].clone()))

    def _collect(self, final, call):
        """one collect call -> readfile.Parsed: n_reads is 1 when the call consumed something (the carriers' "go on"), else 0"""
        import torch

        from . import _lib, readfile
        res = _lib.SamResult()
        with torch.cuda.device(self.device):
            rc = call(res)
        if rc == _lib.ERR_FORMAT and res.bad:
            raise (_malformed_bam if self.format == "bam" else _malformed_collated)(self.path, self.stats["lines"] + int(res.bad_line) + 1, int(res.bad))
        _lib.check(rc)
        st = self.stats
        st["calls"] += 1; st["ms_copy"] += res.ms_copy; st["ms_kernels"] += res.ms_kernels; st["ms_collect"] += res.ms_kernels
        if not (res.consumed or final):
            return readfile.Parsed(0, 0)                   # no whole line or record yet: the carrier presents more
        for k, v in (("lines", res.n_lines), ("header_lines", res.n_header), ("blocks", 1), ("bytes_parsed", res.consumed)):
            st[k] += int(v)
        return readfile.Parsed(1 if res.consumed else 0, int(res.consumed))

    def _parse_host(self, text, final, _max_reads):
        from . import _lib
        n = int(text.size)
        if self.collated:
            collect = self._L.sfgpu_bam_collect_host if self.format == "bam" else self._L.sfgpu_sam_collect_host
            return self._collect(final, lambda res: collect(self._h, self._c, _lib.ptr(text), n, int(final), C.byref(res), _lib.current_stream_ptr()))
        parse = self._L.sfgpu_bam_parse_host if self.format == "bam" else self._L.sfgpu_sam_parse_host
        return self._call(n, final, lambda hits, ch, off, cr, res: parse(
            self._h, _lib.ptr(text), n, int(final), _lib.ptr(hits), ch, _lib.ptr(off), cr, C.byref(res), _lib.current_stream_ptr()))

    def _parse_device(self, text, lo, hi, final, _max_reads, _records):
        from . import _lib
        n = hi - lo
        if lo % 16:                                        # the parser wants its text at a 16-byte boundary
            text[:n] = text[lo:hi].clone()
            self._carry.lo, self._carry.hi, lo, hi = 0, n, 0, n
        view = text[lo:]
        if self.collated:
            collect = self._L.sfgpu_bam_collect_device if self.format == "bam" else self._L.sfgpu_sam_collect_device
            out = self._collect(final, lambda res: collect(self._h, self._c, _lib.ptr(view), n, view.numel(), int(final), C.byref(res),
                                                           _lib.current_stream_ptr()))
            self._carry.starved = True                     # what is left is a line or record that has not ended: inflate before the next call
            return out
        parse = self._L.sfgpu_bam_parse_device if self.format == "bam" else self._L.sfgpu_sam_parse_device
        out = self._call(n, final, lambda hits, ch, off, cr, res: parse(
            self._h, _lib.ptr(view), n, view.numel(), int(final), _lib.ptr(hits), ch, _lib.ptr(off), cr, C.byref(res), _lib.current_stream_ptr()))
        if out.n_reads and not final:
            self._carry.starved = True                     # what is left is one group that has not ended: inflate before the next call
        return out

    def _iter_collated(self):
        """the whole file through the collect calls, finish, then slices of batch_reads fragments"""
        import torch

        from . import _lib
        while (self._carry.next(1 << 62) if self.inflate == "device" else self._carry.next(self._parse_host, 1 << 62)) is not None:
            pass
        info = _lib.SamcInfo()
        with torch.cuda.device(self.device):
            _lib.check(self._L.sfgpu_samc_finish(self._c, C.byref(info), _lib.current_stream_ptr()))
        st = self.stats
        st.update(fragments=int(info.n_reads), sort_rounds=int(info.sort_rounds), state_bytes=int(info.state_bytes), ms_finish=info.ms_finish)
        total, first, per_read = int(info.n_reads), 0, max(1, -(-int(info.n_hits) // max(1, int(info.n_reads))))
        while first < total:
            n = min(self.batch_reads, total - first)
            cap_hits = n * per_read + 1024                 # a guess: the call says what it needs
            off = torch.empty(n + 1, dtype=torch.int32, device=self.device)
            res = _lib.SamResult()
            with torch.cuda.device(self.device):
                for _ in range(2):
                    hits = torch.empty(cap_hits * 24, dtype=torch.uint8, device=self.device)
                    rc = self._L.sfgpu_samc_emit(self._c, first, n, _lib.ptr(hits), cap_hits, _lib.ptr(off), C.byref(res), _lib.current_stream_ptr())
                    if rc != _lib.ERR_CAPACITY:
                        break
                    cap_hits = int(res.need_hits)
            _lib.check(rc)
            st["reads"] += n; st["hits"] += int(res.n_hits); st["pairs"] += int(res.n_pairs); st["ms_emit"] += res.ms_kernels
            first += n
            yield hits[: int(res.n_hits) * 24], off

    def __iter__(self):
        if self._h is None:
            raise ValueError("the SAM file is closed")
        try:
            if self.collated:
                yield from self._iter_collated()
                return
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
                (self._L.sfgpu_bam_close if self.format == "bam" else self._L.sfgpu_sam_close)(self._h)
                if self._c is not None:
                    self._L.sfgpu_samc_close(self._c)
            self._h = self._c = None
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
