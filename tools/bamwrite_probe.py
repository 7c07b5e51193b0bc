"""The mapper's alignments written compressed from the device (samfile.SamDeviceWriter(format="sam.gz" / "bam"):
sfgpu_sam_write_bgzf feeding sfgpu_bgzw_*) on the batch of tools/samwrite_probe.py -- 100 000 read pairs of 2 x 100 bases with
0 .. 3 hit records each against 30 000 transcript names -- in one process beside the plain device writer and the host writers
samfile.write_sam(bgzf=True) and samfile.write_bam (a per-record Python loop, then zlib per member).  Every file is inflated and
compared -- the SAM files with the plain text, the device BAM file with the host writer's -- before anything is timed.  File sizes
stand beside zlib level 1 and level 6 at the same member cut (32 768 payload bytes), computed here with zlib.

Clocks: *_write_s are host wall time (time.perf_counter) around the whole writer, open to close, after torch.cuda.synchronize();
ms_format / ms_encode / ms_copy are device events and ms_sink the host clock inside the sink, from the writer's stats.  The first
run of each leg warms code objects, pools and the page cache and is dropped; the other five are all reported, with their median.

--oriented runs a second leg instead of the one above: the same batch with qualities of every base and oriented=True (the lines
with 0x10 carry SEQ reverse-complemented and QUAL reversed), "sam.gz" and "bam" beside the plain oriented text.  The inflated
"sam.gz" is compared with the plain oriented text (which tools/samwrite_probe.py --oriented compares with write_sam), the "bam"
writer with write_bam(quals=, oriented=True) on the first 2 000 reads; then five writes of each after a warm-up, with a plain
pinned copy of as many bytes as the formatter hands to the encoder.  The record goes to profiles/bamqual_probe.json unless --json
says otherwise.

    python tools/bamwrite_probe.py [--out DIR] [--json FILE] [--reads 100000] [--repeats 5] [--write-only] [--oriented]
Prints one JSON line and writes FILE (default profiles/bamwrite_probe.json).  --write-only: three "sam.gz" and three "bam" writes, nothing else
(for rocprofv3 --kernel-trace --stats)."""
import argparse
import gzip
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sailfish_amd import samfile  # noqa: E402
from samwrite_probe import batch  # noqa: E402

MEMBER = 32768


def zlib_file_bytes(data, level):
    n = 28
    for a in range(0, len(data), MEMBER):
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        n += 18 + len(z.compress(data[a:a + MEMBER]) + z.flush()) + 8
    return n


def oriented_leg(a, dev, names, ref_len, hits, off, b1, b2, d_batch, up, rng):
    d_hits, d_off, d_seqs = d_batch
    L = a.read_len
    q1, q2 = (rng.integers(33, 127, a.reads * L).astype(np.uint8) for _ in range(2))
    d_quals = (up(q1), up(q2))
    path = {fmt: os.path.join(a.out, "oriented." + fmt) for fmt in ("sam", "sam.gz", "bam")}

    def device_write(fmt):
        with samfile.SamDeviceWriter(path[fmt], names, ref_len, True, format=fmt, oriented=True) as w:
            w.write(d_hits, d_off, seqs=d_seqs, quals=d_quals)
        return dict(w.stats)

    for fmt in path:
        device_write(fmt)
    text = open(path["sam"], "rb").read()
    assert gzip.decompress(open(path["sam.gz"], "rb").read()) == text, "the compressed oriented file does not inflate to the plain one"
    stream = gzip.decompress(open(path["bam"], "rb").read())
    n = min(2000, a.reads)                                 # the host writer packs base by base in Python: a prefix of the batch
    sub = os.path.join(a.out, "oriented.sub.bam")
    with samfile.SamDeviceWriter(sub, names, ref_len, True, format="bam", oriented=True) as w:
        w.write(d_hits[:24 * int(off[n])], d_off[:n + 1], seqs=tuple((b[:n * L], o[:n + 1]) for b, o in d_seqs), quals=tuple(q[:n * L] for q in d_quals))
    cut = lambda x: [(x[0][i * L:(i + 1) * L].tobytes(), x[1][i * L:(i + 1) * L].tobytes()) for i in range(n)]  # noqa: E731
    samfile.write_bam(sub + ".host", names, ref_len, hits[:int(off[n])], off[:n + 1], seqs=cut((b1, b2)), quals=cut((q1, q2)), oriented=True)
    assert gzip.decompress(open(sub, "rb").read()) == gzip.decompress(open(sub + ".host", "rb").read()), "the oriented device BAM writer and write_bam disagree"
    legs = {}
    for fmt in path:
        runs = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = device_write(fmt)
            runs.append(dict(st, write_s=time.perf_counter() - t0))
        legs[fmt] = runs
    med = statistics.median
    rec = dict(reads=a.reads, hits=int(len(hits)), text_bytes=len(text), bam_stream_bytes=len(stream), device=torch.cuda.get_device_name(0),
               file_bytes={fmt: os.path.getsize(p) for fmt, p in path.items()}, writer=legs)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for fmt, n_in in (("sam", len(text)), ("sam.gz", len(text)), ("bam", len(stream))):
        runs = legs[fmt]
        rec[fmt + "_median"] = dict(write_s=med(r["write_s"] for r in runs), ms_format=med(r["ms_format"] for r in runs),
                                    ms_copy=med(r["ms_copy"] for r in runs), ms_sink=med(r["ms_sink"] for r in runs))
        if fmt != "sam":
            rec[fmt + "_median"]["ms_encode"] = med(r["ms_encode"] for r in runs)
        src = torch.empty(n_in, dtype=torch.uint8, device=dev).random_(0, 255)
        dst = torch.empty(n_in, dtype=torch.uint8).pin_memory()
        copies = []
        for i in range(a.repeats + 1):
            ev[0].record()
            dst.copy_(src, non_blocking=True)
            ev[1].record()
            torch.cuda.synchronize()
            if i:
                copies.append(ev[0].elapsed_time(ev[1]))
        rec[fmt + "_median"]["plain_copy_ms_of_formatted_bytes"] = med(copies)
    print(json.dumps(rec))
    out = a.json if a.json != os.path.join(ROOT, "profiles", "bamwrite_probe.json") else os.path.join(ROOT, "profiles", "bamqual_probe.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bamwrite_probe_out")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "bamwrite_probe.json"))
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--refs", type=int, default=30_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--write-only", action="store_true")
    ap.add_argument("--oriented", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    rng = np.random.default_rng(23)
    names = [f"ENST{i:011d}.{i % 9 + 1}" for i in range(a.refs)]
    ref_len = rng.integers(6200, 20000, a.refs)
    hits, off, b1, b2, boff = batch(a.reads, a.read_len, a.refs, rng)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(dev)  # noqa: E731
    d_hits, d_off = up(hits.view(np.uint8).reshape(-1)), up(off.view(np.int32))
    d_seqs = ((up(b1), up(boff)), (up(b2), up(boff)))
    path = {fmt: os.path.join(a.out, "mappings." + fmt) for fmt in ("sam", "sam.gz", "bam")}

    def device_write(fmt):
        with samfile.SamDeviceWriter(path[fmt], names, ref_len, True, format=fmt) as w:
            w.write(d_hits, d_off, seqs=d_seqs)
        return dict(w.stats)

    if a.oriented:
        oriented_leg(a, dev, names, ref_len, hits, off, b1, b2, (d_hits, d_off, d_seqs), up, rng)
        return
    if a.write_only:
        for fmt in ("sam.gz", "bam"):
            for _ in range(3):
                st = device_write(fmt)
            print(json.dumps(st))
        return
    seqs = [(b1[i * a.read_len:(i + 1) * a.read_len].tobytes(), b2[i * a.read_len:(i + 1) * a.read_len].tobytes()) for i in range(a.reads)]
    host_path = os.path.join(a.out, "host.sam.gz")

    host_bam_path = os.path.join(a.out, "host.bam")

    def host_write():
        samfile.write_sam(host_path, names, ref_len, hits, off, seqs=seqs, bgzf=True)

    def host_write_bam():
        samfile.write_bam(host_bam_path, names, ref_len, hits, off, seqs=seqs)

    for fmt in path:
        device_write(fmt)
    host_write()
    host_write_bam()
    text = open(path["sam"], "rb").read()
    assert gzip.decompress(open(path["sam.gz"], "rb").read()) == text, "the compressed device file does not inflate to the plain one"
    assert gzip.decompress(open(host_path, "rb").read()) == text, "the host writer disagrees"
    stream = gzip.decompress(open(path["bam"], "rb").read())
    assert stream == gzip.decompress(open(host_bam_path, "rb").read()), "the device BAM file does not inflate to write_bam's stream"
    legs = {}
    for fmt in path:
        runs = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = device_write(fmt)
            runs.append(dict(st, write_s=time.perf_counter() - t0))
        legs[fmt] = runs
    host, host_bam = [], []
    for fn, times in ((host_write, host), (host_write_bam, host_bam)):
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t0)
    med = statistics.median
    rec = dict(reads=a.reads, hits=int(len(hits)), text_bytes=len(text), device=torch.cuda.get_device_name(0), member_payload=MEMBER,
               file_bytes={"sam": len(text), "sam.gz": os.path.getsize(path["sam.gz"]), "host write_sam(bgzf=True), level 6, 65280-byte members":
                           os.path.getsize(host_path), "zlib level 1 at the same cut": zlib_file_bytes(text, 1),
                           "zlib level 6 at the same cut": zlib_file_bytes(text, 6), "bam": os.path.getsize(path["bam"]), "bam stream": len(stream),
                           "host write_bam, level 6, 65280-byte members": os.path.getsize(host_bam_path),
                           "bam stream, zlib level 1 at the same cut": zlib_file_bytes(stream, 1),
                           "bam stream, zlib level 6 at the same cut": zlib_file_bytes(stream, 6)},
               writer=legs, host_bgzf_write_s=host, host_bgzf_write_s_median=med(host), host_write_bam_s=host_bam,
               host_write_bam_s_median=med(host_bam))
    for fmt, runs in legs.items():
        rec[fmt + "_median"] = dict(write_s=med(r["write_s"] for r in runs), ms_format=med(r["ms_format"] for r in runs),
                                    ms_copy=med(r["ms_copy"] for r in runs), ms_sink=med(r["ms_sink"] for r in runs))
    for fmt, n_in in (("sam.gz", len(text)), ("bam", len(stream))):
        gz = legs[fmt]
        enc = med(r["ms_encode"] for r in gz)
        rec[fmt + "_median"].update(ms_encode=enc, encode_GBps_of_input=n_in / enc / 1e6, members=gz[0]["members"], matches=gz[0]["matches"],
                                    literals=gz[0]["literals"], stored_members=gz[0]["stored_members"])
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
