"""eq_classes.txt back in -- the loader the reference left commented out (loadEquivClasses, src/SailfishQuantify.cpp:1444-1494;
--readEqClasses, :1114), for the file writer.write_equiv_counts writes (GZipWriter::writeEquivCounts, src/GZipWriter.cpp:51-92):

    M \\n  C \\n  name_1 \\n ... name_M \\n  then C lines  k \\t id_1 \\t ... \\t id_k \\t count \\n

The header (M, C, the names) is read here on the host.  The class section is handed to the library by address (the file
is mapped, not read into Python) and parsed on the device (sfgpu_eq_add_text_host); its classes are folded into a builder
with upsert semantics, so several files (lanes, runs) fold into one table.  Every error names the file and the 1-based
line of the file, header lines included.

The way out is the mirror: write_file writes the header here and hands the table's device arrays to the library, which formats
the class section on the device (sfgpu_eqvec_write_text) and delivers it in whole-line chunks (write_classes); text_size only
measures it.  format_text is the independent numpy restatement of the same bytes that tools and tests compare against."""
import ctypes as C
import mmap
import os

import numpy as np
import torch

from . import _lib

_NO_LINE = (1 << 64) - 1
_KIND = {1: "a byte that is not a digit, tab or newline (fields are separated by single tabs; CRLF line ends are refused)",
         2: "an empty line or an empty field",
         3: "the label length k is 0, or the line does not hold exactly k ids and a count",
         4: "a transcript id >= M, the number of transcripts in the header",
         5: "a count that does not fit 64 bits",
         6: "a line longer than the chunk size"}


class EqFileHeader:
    """What precedes the class section: n_transcripts (M), n_classes (C), names, the byte offset of the first class line
    and the number of header lines (2 + M)."""

    def __init__(self, path, n_transcripts, n_classes, names, data_offset):
        self.path, self.n_transcripts, self.n_classes = path, n_transcripts, n_classes
        self.names, self.data_offset = names, data_offset
        self.header_lines = 2 + n_transcripts


def _where(path, line):
    return f"{path}, line {line}"


def _header_from(buf, path):
    """Parse the header out of `buf` (bytes or an mmap)."""
    pos = 0

    def next_line(lineno, what):
        nonlocal pos
        end = buf.find(b"\n", pos)
        if end < 0:
            raise ValueError(f"{_where(path, lineno)}: the file ends inside the header (expected {what})")
        s = bytes(buf[pos:end])
        pos = end + 1
        return s

    vals = []
    for lineno, what in ((1, "M, the number of transcripts"), (2, "C, the number of classes")):
        s = next_line(lineno, what)
        if not s or not s.isdigit() or not s.isascii():
            raise ValueError(f"{_where(path, lineno)}: expected {what} as a decimal integer, got {s[:40]!r}")
        vals.append(int(s))
    M, Cn = vals
    names = []
    for i in range(M):
        lineno = 3 + i
        end = buf.find(b"\n", pos)
        if end < 0:
            raise ValueError(f"{_where(path, lineno)}: the file ends after {i} of the M={M} transcript names")
        s = bytes(buf[pos:end])
        if not s or b"\t" in s or b"\r" in s:
            raise ValueError(f"{_where(path, lineno)}: expected transcript name {i + 1} of M={M}, got {s[:40]!r} "
                             "(truncated names, or a header M larger than the names present?)")
        names.append(s.decode("utf-8"))
        pos = end + 1
    return EqFileHeader(path, M, Cn, names, pos)


def read_header(path):
    """The header of one class file (raises ValueError naming the line)."""
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        if size == 0:
            raise ValueError(f"{_where(path, 1)}: empty file")
        with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            return _header_from(mm, path)


def check_names(header, names):
    """The file must list exactly `names` (the index's transcripts, or the first file's), in that order."""
    names = list(names)
    if header.n_transcripts != len(names):
        raise ValueError(f"{_where(header.path, 1)}: the header lists M={header.n_transcripts} transcripts, expected {len(names)}")
    for i, (a, b) in enumerate(zip(header.names, names)):
        if a != b:
            raise ValueError(f"{_where(header.path, 3 + i)}: transcript {i} is named {a!r}, expected {b!r}")


def check_same_names(headers):
    """Several files fold into one table only when they list the same names in the same order; names the first mismatch."""
    for h in headers[1:]:
        if h.n_transcripts != headers[0].n_transcripts:
            raise ValueError(f"{_where(h.path, 1)}: the header lists M={h.n_transcripts} transcripts, "
                             f"{headers[0].path} lists {headers[0].n_transcripts}")
        check_names(h, headers[0].names)


def fold_file(builder, path, names=None, chunk_bytes=0):
    """Fold the classes of one file into `builder` (an EquivalenceClassBuilder after start()).  `names`, when given, must be
    what the header lists.  Returns (header, result dict of sfgpu_eqtext_result)."""
    with open(path, "rb") as f:
        size = os.fstat(f.fileno()).st_size
        if size == 0:
            raise ValueError(f"{_where(path, 1)}: empty file")
        mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    view = None
    try:
        h = _header_from(mm, path)
        if names is not None:
            check_names(h, names)
        view = np.frombuffer(mm, dtype=np.uint8)
        res = _lib.EqTextResult()
        rc = builder._add_text(view.ctypes.data + h.data_offset, size - h.data_offset, h.n_transcripts, chunk_bytes, res)
        if rc != _lib.OK:
            if res.err_line != _NO_LINE:
                raise ValueError(f"{_where(path, h.header_lines + res.err_line + 1)}: {_KIND.get(res.err_kind, 'malformed line')}")
            _lib.check(rc)
        if res.n_lines != h.n_classes:
            line = h.header_lines + min(res.n_lines, h.n_classes) + 1
            raise ValueError(f"{_where(path, line)}: the header announces C={h.n_classes} classes, the file holds {res.n_lines}")
        return h, res.as_dict()
    finally:
        del view
        mm.close()


def fold_files(builder, paths, names=None, chunk_bytes=0):
    """Fold several files (lanes, runs) into one builder: equal labels add their counts.  All headers are read and compared
    first (same names, same order; `names` too when given), so a mismatch folds nothing.  Returns (headers, results)."""
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    headers = [read_header(p) for p in paths]
    if not headers:
        raise ValueError("no class files given")
    if names is not None:
        check_names(headers[0], names)
    check_same_names(headers)
    results = [fold_file(builder, p, chunk_bytes=chunk_bytes)[1] for p in paths]
    return headers, results


def _device_table(vec):
    """(rowptr, ids, counts) device tensors of an EqVec or of such a triple; 32-bit rowptr / ids and 64-bit counts, as exported."""
    rowptr, ids, counts = (vec.rowptr, vec.ids, vec.counts) if hasattr(vec, "rowptr") else vec
    for t, sizes, what in ((rowptr, (4,), "rowptr"), (ids, (4,), "ids"), (counts, (8,), "counts")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and not t.is_floating_point() and t.element_size() in sizes):
            raise TypeError(f"{what}: expected a device tensor of {sizes[0] * 8}-bit integers")
    if rowptr.numel() != counts.numel() + 1:
        raise ValueError(f"rowptr has {rowptr.numel()} entries for {counts.numel()} classes")
    return rowptr.contiguous(), ids.contiguous(), counts.contiguous()


def _write_text(vec, chunk_bytes, sink):
    """sfgpu_eqvec_write_text on the table's device, behind torch's current stream; returns (status, result)."""
    rowptr, ids, counts = _device_table(vec)
    res = _lib.EqTextWriteResult()
    with torch.cuda.device(rowptr.device):
        rc = _lib.lib().sfgpu_eqvec_write_text(_lib.ptr(rowptr), _lib.ptr(ids), _lib.ptr(counts), counts.numel(), int(chunk_bytes),
                                               sink, None, C.byref(res), _lib.current_stream_ptr())
    return rc, res


def text_size(vec):
    """What the class section of `vec` (an EqVec, or (rowptr, ids, counts) device tensors) will measure, without formatting it:
    the sfgpu_eqtext_write_result as a dict (n_bytes, n_lines, n_ids, max_line_bytes)."""
    rc, res = _write_text(vec, 0, _lib.TEXT_SINK(0))
    _lib.check(rc)
    return res.as_dict()


def write_classes(fileobj, vec, chunk_bytes=0):
    """The class section of `vec` (an EqVec, or (rowptr, ids, counts) device tensors), formatted on the device
    (sfgpu_eqvec_write_text), into the binary file object `fileobj`, chunk by chunk.  Returns the sfgpu_eqtext_write_result as
    a dict.  An exception of fileobj.write stops the writer and is raised again here."""
    raised = []

    def sink(addr, n, _user):
        try:                                   # nothing may unwind through the C frame
            fileobj.write(memoryview((C.c_char * n).from_address(addr)))
            return 0
        except BaseException as e:             # noqa: BLE001  (re-raised below)
            raised.append(e)
            return 1

    rc, res = _write_text(vec, chunk_bytes, _lib.TEXT_SINK(sink))
    if raised:
        raise raised[0]
    _lib.check(rc)
    return res.as_dict()


def write_file(path, names, vec, chunk_bytes=0):
    """eq_classes.txt for the table `vec` over the transcripts `names`: the header (M, C, the names) from the host, the class
    section through write_classes.  The bytes are format_text's.  Returns write_classes' result."""
    rowptr, _, counts = _device_table(vec)
    with open(path, "wb") as f:
        f.write(f"{len(names)}\n{counts.numel()}\n".encode() + "".join(n + "\n" for n in names).encode())
        return write_classes(f, vec, chunk_bytes)


def format_text(names, rowptr, ids, counts):
    """The bytes writer.write_equiv_counts writes for this CSR table (in the given class order), built with numpy instead of a
    per-class Python loop: for tables of millions of classes (tools, tests) and for merged tables handed to another machine."""
    rowptr = np.asarray(rowptr, np.int64); ids = np.asarray(ids, np.uint64); counts = np.asarray(counts, np.uint64)
    C = len(counts)
    k = np.diff(rowptr)
    head = f"{len(names)}\n{C}\n".encode() + "".join(n + "\n" for n in names).encode()
    if C == 0:
        return head
    # tokens in file order: k, the ids, the count -- each followed by '\t', the count by '\n'
    n_tok = int(rowptr[-1]) + 2 * C
    first = rowptr[:-1] + 2 * np.arange(C, dtype=np.int64)
    tok = np.empty(n_tok, np.uint64)
    tok[first] = k.astype(np.uint64)
    tok[first + k + 1] = counts
    tok[np.arange(int(rowptr[-1]), dtype=np.int64) + 2 * np.repeat(np.arange(C, dtype=np.int64), k) + 1] = ids
    nd = np.ones(n_tok, np.int64)
    for e in range(1, 20):
        nd += tok >= np.uint64(10 ** e)
    start = np.zeros(n_tok + 1, np.int64)
    np.cumsum(nd + 1, out=start[1:])
    out = np.full(int(start[-1]), ord("\t"), np.uint8)
    out[start[first + k + 2] - 1] = ord("\n")
    rem = tok.copy()
    for d in range(20):                    # digits from the right
        live = nd > d
        if not live.any():
            break
        idx = np.nonzero(live)[0]
        out[start[idx] + nd[idx] - 1 - d] = (rem[idx] % np.uint64(10)).astype(np.uint8) + ord("0")
        rem[idx] //= np.uint64(10)
    return head + out.tobytes()
