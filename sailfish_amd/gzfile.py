"""gzip files written from device memory -- GZipWriter::writeBootstrap<T> (src/GZipWriter.cpp:249-285) without the host
compressor: the raw bytes of device tensors become one gzip member whose DEFLATE blocks are produced on the device
(sfgpu_gz_open / sfgpu_gz_write_device / sfgpu_gz_close, sailfish_amd/csrc/gzwrite.hip).  Any gzip reader inflates the file to
the bytes written, in order; the compressed bytes are not zlib's.

`BgzfDeviceWriter` is its twin for the blocked form (BGZF: the container of BAM, what samtools and IGV read), whose members carry
real (length, distance) matches (sfgpu_bgzw_*, sailfish_amd/csrc/bgzf_write.hip); `write_bgzf` is the host-side writer of that
form, which `readfile.ReadFile` and `samfile.SamFile` inflate on the device."""
import ctypes as C
import os
import struct
import zlib

import torch

from . import _lib


class GzDeviceWriter:
    """GzDeviceWriter(path or binary file object).  write(tensor) appends the raw bytes of a contiguous device tensor,
    close() finishes the member and returns the sfgpu_gz_result as a dict (also kept as .result); usable as a context manager.
    The stream is opened by the first write, on that tensor's device (by close, on the current device, for an empty file).
    An exception of the file object's write stops the stream and is raised again by the call that met it."""

    def __init__(self, fileobj_or_path, chunk_bytes=0):
        self._own = isinstance(fileobj_or_path, (str, bytes, os.PathLike))
        self._f = open(fileobj_or_path, "wb") if self._own else fileobj_or_path
        self._chunk = int(chunk_bytes)
        self._h = None
        self._closed = False
        self._raised = []
        self.result = None

        def sink(addr, n, _user):
            try:                                   # nothing may unwind through the C frame
                self._f.write(memoryview((C.c_char * n).from_address(addr)))
                return 0
            except BaseException as e:             # noqa: BLE001  (re-raised by _check)
                self._raised.append(e)
                return 1
        self._sink = _lib.TEXT_SINK(sink)          # alive as long as the handle

    def _check(self, rc):
        if self._raised:
            raise self._raised.pop(0)
        _lib.check(rc)

    def _open(self, device):
        if self._h is None:
            h = C.c_void_p()
            with torch.cuda.device(device):
                rc = _lib.lib().sfgpu_gz_open(C.byref(h), self._sink, None, self._chunk)
            self._check(rc)
            self._h, self._device = h, device

    def write(self, tensor):
        if self._closed:
            raise ValueError("write to a closed GzDeviceWriter")
        if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda):
            raise TypeError("GzDeviceWriter.write expects a device tensor")
        if not tensor.is_contiguous():
            raise ValueError("GzDeviceWriter.write expects a contiguous tensor")
        self._open(tensor.device)
        if tensor.device != self._device:
            raise ValueError(f"the stream was opened on {self._device}, the tensor lies on {tensor.device}")
        n = tensor.numel() * tensor.element_size()
        with torch.cuda.device(self._device):
            rc = _lib.lib().sfgpu_gz_write_device(self._h, _lib.ptr(tensor), n, _lib.current_stream_ptr())
        self._check(rc)
        return n

    def close(self):
        if self._closed:
            return self.result
        self._closed = True
        try:
            self._open(torch.device("cuda", torch.cuda.current_device()))
            res = _lib.GzResult()
            h, self._h = self._h, None
            with torch.cuda.device(self._device):
                rc = _lib.lib().sfgpu_gz_close(h, C.byref(res))
            self.result = res.as_dict()
            self._check(rc)
        finally:
            if self._own:
                self._f.close()
        return self.result

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class BgzfDeviceWriter:
    """BgzfDeviceWriter(path or binary file object, chunk_bytes=0): the twin of GzDeviceWriter for a BGZF file (sfgpu_bgzw_open /
    sfgpu_bgzw_write_device / sfgpu_bgzw_close).  write(tensor) appends the raw bytes of a contiguous device tensor as members of
    32 768 payload bytes (the write's last one short), close() writes the EOF member and returns the sfgpu_bgzw_result as a dict
    (also kept as .result and .stats); usable as a context manager.  The stream is opened by the first write, on that tensor's
    device (by close, on the current device, for an empty file).  An exception of the file object's write stops the stream and is
    raised again by the call that met it.  The file is a function of the bytes and of the way they are split into writes."""

    def __init__(self, fileobj_or_path, chunk_bytes=0):
        self._own = isinstance(fileobj_or_path, (str, bytes, os.PathLike))
        self._f = open(fileobj_or_path, "wb") if self._own else fileobj_or_path
        self._chunk = int(chunk_bytes)
        self._h = None
        self._closed = False
        self._raised = []
        self.result = None

        def sink(addr, n, _user):
            try:                                   # nothing may unwind through the C frame
                self._f.write(memoryview((C.c_char * n).from_address(addr)))
                return 0
            except BaseException as e:             # noqa: BLE001  (re-raised by _check)
                self._raised.append(e)
                return 1
        self._sink = _lib.TEXT_SINK(sink)          # alive as long as the handle

    @property
    def stats(self):
        return self.result

    def _check(self, rc):
        if self._raised:
            raise self._raised.pop(0)
        _lib.check(rc)

    def _open(self, device):
        if self._h is None:
            h = C.c_void_p()
            with torch.cuda.device(device):
                rc = _lib.lib().sfgpu_bgzw_open(C.byref(h), self._sink, None, self._chunk)
            self._check(rc)
            self._h, self._device = h, device

    def write(self, tensor):
        if self._closed:
            raise ValueError("write to a closed BgzfDeviceWriter")
        if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda):
            raise TypeError("BgzfDeviceWriter.write expects a device tensor")
        if not tensor.is_contiguous():
            raise ValueError("BgzfDeviceWriter.write expects a contiguous tensor")
        self._open(tensor.device)
        if tensor.device != self._device:
            raise ValueError(f"the stream was opened on {self._device}, the tensor lies on {tensor.device}")
        n = tensor.numel() * tensor.element_size()
        with torch.cuda.device(self._device):
            rc = _lib.lib().sfgpu_bgzw_write_device(self._h, _lib.ptr(tensor), n, _lib.current_stream_ptr())
        self._check(rc)
        return n

    def close(self):
        if self._closed:
            return self.result
        self._closed = True
        try:
            self._open(torch.device("cuda", torch.cuda.current_device()))
            res = _lib.BgzwResult()
            h, self._h = self._h, None
            with torch.cuda.device(self._device):
                rc = _lib.lib().sfgpu_bgzw_close(h, C.byref(res))
            self.result = res.as_dict()
            self._check(rc)
        finally:
            if self._own:
                self._f.close()
        return self.result

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")      # the empty member that ends a BGZF file


def bgzf_member(payload, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    """one BGZF member: gzip header with the 'BC' subfield (BSIZE = member bytes - 1), raw DEFLATE of `payload`, CRC-32, ISIZE"""
    if len(payload) > 65536:
        raise ValueError("a BGZF member holds at most 65536 bytes")
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body = z.compress(payload) + z.flush()
    total = 18 + len(body) + 8
    if total > 65536:
        raise ValueError(f"the member would be {total} bytes: lower member_bytes (65280 always fits)")
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", total - 1) + body
            + struct.pack("<II", zlib.crc32(payload), len(payload)))


def write_bgzf(path_or_file, data, level=6, member_bytes=65280, strategy=zlib.Z_DEFAULT_STRATEGY):
    """`data` (bytes-like) as a BGZF file: members of member_bytes payload bytes each, deflated by zlib on the host, and the
    28-byte EOF member.  Any gzip reader inflates it to `data`.  Returns the number of bytes written."""
    if not 1 <= member_bytes <= 65536:
        raise ValueError("member_bytes must be 1 .. 65536")
    own = isinstance(path_or_file, (str, bytes, os.PathLike))
    f = open(path_or_file, "wb") if own else path_or_file
    try:
        view, n = memoryview(data).cast("B"), 0
        for a in range(0, len(view), member_bytes):
            n += f.write(bgzf_member(bytes(view[a:a + member_bytes]), level, strategy))
        n += f.write(BGZF_EOF)
    finally:
        if own:
            f.close()
    return n
