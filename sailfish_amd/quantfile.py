"""quant.sf out -- the file GZipWriter::writeAbundances writes (src/GZipWriter.cpp:194-248):

    Name \\t Length \\t EffectiveLength \\t TPM \\t NumReads \\n        then, for every transcript,
    name \\t Length \\t %g(eff) \\t %g(tpm) \\t %g(num_reads) \\n

write_file writes the header line here and hands the columns' device arrays to the library, which formats the rows on the
device (sfgpu_quant_write_text: the exact %g of sailfish_amd/csrc/gfmt.h) and delivers them in whole-row chunks (write_rows);
text_size only measures them.  format_rows is the host restatement of the same bytes, the per-row loop over "%g" that
writer.write_abundances ran before: it is what tools and tests compare against."""
import ctypes as C

import numpy as np
import torch

from . import _lib

HEADER = b"Name\tLength\tEffectiveLength\tTPM\tNumReads\n"


def format_rows(names, length, eff, tpm, num_reads):
    """The rows of quant.sf for these columns (host sequences or numpy arrays; names as str or bytes), one "%g" at a time."""
    length = np.asarray(length).astype(np.int64) & 0xFFFFFFFF
    eff = np.asarray(eff, np.float64); tpm = np.asarray(tpm, np.float64); num_reads = np.asarray(num_reads, np.float64)
    out = []
    for i, name in enumerate(names):
        if isinstance(name, str):
            name = name.encode("utf-8")
        out.append(name + b"\t%d\t%s\t%s\t%s\n" % (int(length[i]), ("%g" % eff[i]).encode(), ("%g" % tpm[i]).encode(),
                                                      ("%g" % num_reads[i]).encode()))
    return b"".join(out)


def names_blob(names):
    """(bytes, offsets): the names (str as UTF-8, or bytes) back to back and the len(names) + 1 byte offsets (uint64)."""
    enc = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
    off = np.zeros(len(enc) + 1, np.uint64)
    if enc:
        off[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
    return b"".join(enc), off


def _device_columns(names, length, eff, tpm, num_reads):
    """(blob, offsets, length, eff, tpm, num_reads) as contiguous device tensors.  `names` is a (uint8 blob, 64-bit offsets)
    pair of device tensors (Transcripts.name_blob()) or a list of names, uploaded to the device of `eff`."""
    for t, what in ((eff, "eff"), (tpm, "tpm"), (num_reads, "num_reads")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 1):
            raise TypeError(f"{what}: expected a 1-D float64 device tensor")
    if not (isinstance(length, torch.Tensor) and length.is_cuda and not length.is_floating_point() and length.element_size() == 4):
        raise TypeError("length: expected a device tensor of 32-bit integers")
    if isinstance(names, tuple) and len(names) == 2 and isinstance(names[0], torch.Tensor):
        blob, off = names
        if not (blob.is_cuda and blob.element_size() == 1 and off.is_cuda and not off.is_floating_point() and off.element_size() == 8):
            raise TypeError("names: expected (uint8 blob, 64-bit offsets) device tensors")
    else:
        b, o = names_blob(names)
        blob = torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(eff.device)
        off = torch.from_numpy(o.view(np.int64).copy()).to(eff.device)
    n = eff.numel()
    if not (off.numel() == n + 1 and length.numel() == n and tpm.numel() == n and num_reads.numel() == n):
        raise ValueError(f"columns of different lengths: {off.numel() - 1} names, {length.numel()} lengths, {n} / {tpm.numel()} / "
                         f"{num_reads.numel()} doubles")
    return blob.contiguous(), off.contiguous(), length.contiguous(), eff.contiguous(), tpm.contiguous(), num_reads.contiguous()


def _write_text(cols, chunk_bytes, sink):
    """sfgpu_quant_write_text on the columns' device, behind torch's current stream; returns (status, result)."""
    blob, off, length, eff, tpm, num_reads = _device_columns(*cols)
    res = _lib.QuantWriteResult()
    with torch.cuda.device(eff.device):
        rc = _lib.lib().sfgpu_quant_write_text(_lib.ptr(blob) if blob.numel() else None, _lib.ptr(off), _lib.ptr(length), _lib.ptr(eff),
                                               _lib.ptr(tpm), _lib.ptr(num_reads), eff.numel(), int(chunk_bytes), sink, None,
                                               C.byref(res), _lib.current_stream_ptr())
    return rc, res


def text_size(names, length, eff, tpm, num_reads):
    """What the rows will measure, without formatting them: the sfgpu_quant_write_result as a dict (n_bytes, n_rows,
    max_row_bytes, n_slow)."""
    rc, res = _write_text((names, length, eff, tpm, num_reads), 0, _lib.TEXT_SINK(0))
    _lib.check(rc)
    return res.as_dict()


def write_rows(fileobj, names, length, eff, tpm, num_reads, chunk_bytes=0):
    """The rows of quant.sf, formatted on the device (sfgpu_quant_write_text), into the binary file object `fileobj`, chunk by
    chunk.  `names`: Transcripts.name_blob() or a list of names; `length`: 32-bit integer device tensor; the other columns:
    float64 device tensors.  Returns the sfgpu_quant_write_result as a dict.  An exception of fileobj.write stops the writer and
    is raised again here."""
    raised = []

    def sink(addr, n, _user):
        try:                                   # nothing may unwind through the C frame
            fileobj.write(memoryview((C.c_char * n).from_address(addr)))
            return 0
        except BaseException as e:             # noqa: BLE001  (re-raised below)
            raised.append(e)
            return 1

    rc, res = _write_text((names, length, eff, tpm, num_reads), chunk_bytes, _lib.TEXT_SINK(sink))
    if raised:
        raise raised[0]
    _lib.check(rc)
    return res.as_dict()


def write_file(path, names, length, eff, tpm, num_reads, chunk_bytes=0):
    """quant.sf at `path`: the header line from the host, the rows through write_rows.  The bytes are HEADER + format_rows'.
    Returns write_rows' result."""
    with open(path, "wb") as f:
        f.write(HEADER)
        return write_rows(f, names, length, eff, tpm, num_reads, chunk_bytes)
