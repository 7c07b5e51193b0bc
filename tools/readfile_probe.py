"""Read files at run size through the device parser (sfgpu_reads_parse_host; sailfish_amd/readfile.py) and through the path it
replaces, in one process on the same files:
  device  readfile.ReadFile(path).read(all): blocks of the file -> pinned staging -> kernels -> (bases, offsets) on the device
  host    a Python loop over the lines into a list of bytes, mapper.pack_sequences, and the copy to the device
on a paired FASTQ (--pairs, 2 000 000 pairs of 2 x 100 bases, generated in-process) and a FASTA wrapped at 60 columns
(--transcripts, 100 000 of 200 .. 4000 bases).  The two results are compared (bases and offsets, equal) BEFORE any time is reported.

Clocks: *_s are host wall time (time.perf_counter) after torch.cuda.synchronize(); ms_copy / ms_kernels are the library's device
events summed over the parse calls of a file; file_read_s is a bare readinto loop over the file (page cache warm, like the parse
runs); h2d_pinned_ms is ONE plain copy of the file's bytes from a pinned tensor to the device, device events around it: the
yardstick the parse kernels are held against.  The first run of each leg warms code objects, pools and the page cache and is
dropped; the rest are all reported, with their medians.

    python tools/readfile_probe.py [--out DIR] [--pairs 2000000] [--transcripts 100000] [--repeats 5]
Prints one JSON line and writes DIR/readfile_probe.json."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sailfish_amd import mapper, readfile  # noqa: E402


def write_fastq(path, n, read_len, mate, rng):
    """fixed-width records, built as one byte matrix per slab of reads"""
    with open(path, "wb") as f:
        for a in range(0, n, 250_000):
            m = min(n, a + 250_000) - a
            name = np.char.add(np.char.add("@r", np.char.zfill(np.arange(a, a + m).astype(str), 9)), f"/{mate}\n").astype("S14")
            rec = np.empty((m, 14 + read_len + 1 + 2 + read_len + 1), np.uint8)
            rec[:, :14] = np.frombuffer(name.tobytes(), np.uint8).reshape(m, 14)
            rec[:, 14:14 + read_len] = rng.choice(np.frombuffer(b"ACGT", np.uint8), (m, read_len))
            rec[:, 14 + read_len:17 + read_len] = np.frombuffer(b"\n+\n", np.uint8)
            rec[:, 17 + read_len:-1] = rng.integers(33, 127, (m, read_len), dtype=np.uint8)
            rec[:, -1] = 10
            f.write(rec.tobytes())


def write_fasta(path, n, rng):
    with open(path, "wb") as f:
        for t in range(n):
            s = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(rng.integers(200, 4001))).tobytes()
            f.write(b">ENST%011d gene\n" % t + b"\n".join(s[a:a + 60] for a in range(0, len(s), 60)) + b"\n")


def host_fastq(path):
    seqs = []
    with open(path, "rb") as f:
        for i, line in enumerate(f):
            if i & 3 == 1:
                seqs.append(line.rstrip(b"\r\n"))
    return seqs


def host_fasta(path):
    seqs, cur = [], None
    with open(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if cur is not None:
                    seqs.append(b"".join(cur))
                cur = []
            else:
                cur.append(line.rstrip(b"\r\n"))
    if cur is not None:
        seqs.append(b"".join(cur))
    return seqs


def run_file(path, host_loop, dev, repeats):
    size = os.path.getsize(path)
    device, host, reads, copies = [], [], [], []
    buf = np.empty(32 << 20, np.uint8)
    pinned = torch.empty(size, dtype=torch.uint8).pin_memory()
    with open(path, "rb", buffering=0) as f:
        f.readinto(memoryview(pinned.numpy()))
    d_raw = torch.empty(size, dtype=torch.uint8, device=dev)
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with readfile.ReadFile(path, dev) as rf:
            b, o = rf.read(1 << 62)
            torch.cuda.synchronize()
            device.append(dict(device_s=time.perf_counter() - t0, **rf.stats))
        t0 = time.perf_counter()
        with open(path, "rb", buffering=0) as f:
            while f.readinto(buf):
                pass
        reads.append(time.perf_counter() - t0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); d_raw.copy_(pinned, non_blocking=True); e1.record()
        torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        seqs = host_loop(path)
        t1 = time.perf_counter()
        hb, ho = mapper.pack_sequences(seqs)
        t2 = time.perf_counter()
        hb, ho = hb.to(dev), ho.to(dev)
        torch.cuda.synchronize()
        host.append(dict(host_s=time.perf_counter() - t0, host_loop_s=t1 - t0, host_pack_s=t2 - t1, host_copy_s=time.perf_counter() - t2))
        assert torch.equal(b, hb) and torch.equal(o, ho), f"{path}: the device result differs from the host path's"
        n_records, n_bases = int(o.numel()) - 1, int(o[-1])
        del seqs, hb, ho, b, o
    med = lambda rows, k: statistics.median(r[k] for r in rows[1:])  # noqa: E731
    return dict(file_bytes=size, records=n_records, bases=n_bases, device_runs=device[1:], host_runs=host[1:], file_read_s=reads[1:],
                h2d_pinned_ms=copies[1:], device_s_median=med(device, "device_s"), ms_copy_median=med(device, "ms_copy"),
                ms_kernels_median=med(device, "ms_kernels"), file_read_s_median=statistics.median(reads[1:]),
                h2d_pinned_ms_median=statistics.median(copies[1:]), host_s_median=med(host, "host_s"),
                kernels_below_plain_copy=med(device, "ms_kernels") < statistics.median(copies[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="readfile_probe_out")
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--transcripts", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    rng = np.random.default_rng(31)
    props = torch.cuda.get_device_properties(0)
    rec = dict(pairs=a.pairs, read_len=a.read_len, transcripts=a.transcripts, device=torch.cuda.get_device_name(0),
               gcn_arch=getattr(props, "gcnArchName", None), compute_units=props.multi_processor_count)
    with tempfile.TemporaryDirectory() as tmp:
        for mate in (1, 2):
            p = os.path.join(tmp, f"reads_{mate}.fastq")
            write_fastq(p, a.pairs, a.read_len, mate, rng)
            rec[f"fastq_mate{mate}"] = run_file(p, host_fastq, dev, a.repeats)
            os.remove(p)
        p = os.path.join(tmp, "transcripts.fasta")
        write_fasta(p, a.transcripts, rng)
        rec["fasta"] = run_file(p, host_fasta, dev, a.repeats)
    print(json.dumps(rec))
    with open(os.path.join(a.out, "readfile_probe.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
