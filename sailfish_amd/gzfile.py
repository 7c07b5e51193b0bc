"""gzip files written from device memory -- GZipWriter::writeBootstrap<T> (src/GZipWriter.cpp:249-285) without the host
compressor: the raw bytes of device tensors become one gzip member whose DEFLATE blocks are produced on the device
(sfgpu_gz_open / sfgpu_gz_write_device / sfgpu_gz_close, sailfish_amd/csrc/gzwrite.hip).  Any gzip reader inflates the file to
the bytes written, in order; the compressed bytes are not zlib's."""
import ctypes as C
import os

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
