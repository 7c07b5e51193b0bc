"""What the BGZF inflate kernel (sfgpu_bgzf_inflate_host, csrc/bgzf_read.hip) spends per member, by what the members hold: the
same 8 x 65 280 bytes of FASTQ text as stored blocks (level 0), literals only (Z_HUFFMAN_ONLY), level 6 and Z_FIXED, and 65 280
zero bytes (254 matches of length 258 per member) -- once as 8 members and once as 800 in one launch.  ms_kernels is the
library's device-event time of the third call.  A launch of 800 members lasts as long as one of 8: the kernel is bound by the
serial decode of one member, not by the device.

    python tools/bgzf_kinds_probe.py > profiles/bgzf_kinds_probe.txt"""
import ctypes as C
import io
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from sailfish_amd import _lib, gzfile  # noqa: E402
from test_bgzf_cpu import text_3000  # noqa: E402


def run(name, data, reps, dev):
    data = data * reps
    out = torch.empty(65536 * 8 * reps + 64, dtype=torch.uint8, device=dev)
    for _ in range(3):
        res = _lib.BgzfResult()
        _lib.check(_lib.lib().sfgpu_bgzf_inflate_host(data, len(data), 1, _lib.ptr(out), out.numel(), C.byref(res), None))
    print(f"{name:14s} members {res.n_members:4d}  payload {res.n_bytes_out / 1e6:7.3f} MB  ms_kernels {res.ms_kernels:7.3f}  "
          f"ms_copy {res.ms_copy:6.3f}", flush=True)


def main():
    dev = torch.device("cuda:0")
    text = text_3000()[: 65280 * 8]

    def members(**kw):
        f = io.BytesIO()
        gzfile.write_bgzf(f, text, **kw)
        return f.getvalue()[: -len(gzfile.BGZF_EOF)]
    for reps in (1, 100):
        run("level0", members(level=0), reps, dev)
        run("huffman_only", members(strategy=zlib.Z_HUFFMAN_ONLY), reps, dev)
        run("level6", members(level=6), reps, dev)
        run("fixed", members(strategy=zlib.Z_FIXED), reps, dev)
        run("zeros", gzfile.bgzf_member(bytes(65280)) * 8, reps, dev)


if __name__ == "__main__":
    main()
