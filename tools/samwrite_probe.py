"""The mapper's alignments as SAM (sfgpu_sam_write_text; samfile.SamDeviceWriter) at the size of one mapper batch: 100 000 read
pairs of 2 x 100 bases with 0 .. 3 hit records each (15 % unmapped, most records pairs, some orphans) against 30 000 transcript
names, written with SamDeviceWriter from the device arrays, and with samfile.write_sam -- the per-record Python loop over a host
copy -- in one process from the same records.  The two files are compared before anything is timed.  The yardstick is a plain
pinned device-to-host copy of as many bytes as the file has.

Clocks: device_write_s and host_write_s are host wall time (time.perf_counter) around the whole call, after
torch.cuda.synchronize(); format_ms / d2h_ms are device events and sink_ms the host clock inside the sink, from the writer's stats;
plain_copy_ms is device events around one copy into a pinned buffer.  The first run of each leg warms code objects, pools and the
page cache and is dropped; the other five are all reported, with their median.

--oriented adds a second leg on the same batch: qualities of every base and SamDeviceWriter(oriented=True), so that the lines
with 0x10 (half the records) carry SEQ reverse-complemented and QUAL reversed.  Its file is compared with
write_sam(quals=, oriented=True) once, then written five times after a warm-up; the record gains `oriented` (its runs, medians
and a plain pinned copy of as many bytes as ITS text has).  --skip-host leaves the host loop's timing out (a quick A/B of the
device legs).

    python tools/samwrite_probe.py [--out DIR] [--json FILE] [--reads 100000] [--repeats 5] [--write-only] [--oriented] [--skip-host]
Prints one JSON line and writes FILE (default profiles/samwrite_probe.json).  --write-only: three device writes, nothing else
(for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sailfish_amd import samfile  # noqa: E402
from sailfish_amd.hits import HIT_DTYPE  # noqa: E402


def batch(n_reads, read_len, n_refs, rng):
    """(hits, offsets, bases of mate 1, of mate 2, base offsets): one paired batch as the mapper leaves it, on the host"""
    per_read = rng.choice([0, 1, 2, 3], n_reads, p=[0.15, 0.6, 0.15, 0.1])
    off = np.concatenate([[0], np.cumsum(per_read)]).astype(np.uint32)
    n = int(off[-1])
    hits = np.zeros(n, HIT_DTYPE)
    status = rng.choice([3, 3, 3, 3, 1, 2], n_reads)[np.repeat(np.arange(n_reads), per_read)]     # one kind per read, as the mapper gives
    pair = status == 3
    hits["tid"] = rng.integers(0, n_refs, n)
    hits["pos"] = rng.integers(-20, 6000, n)
    hits["mate_pos"] = np.where(pair, hits["pos"] + rng.integers(-300, 300, n), 0)
    hits["mate_pos"] = np.maximum(hits["mate_pos"], -20)
    hits["frag_len"] = np.where(pair, np.abs(hits["mate_pos"] - hits["pos"]) + read_len, 0)
    hits["read_len"] = read_len
    hits["mate_len"] = np.where(pair, read_len, 0)
    hits["fwd"] = rng.integers(0, 2, n)
    hits["mate_fwd"] = np.where(pair, 1 - hits["fwd"], 0)
    hits["mate_status"] = status
    bases = [np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_reads * read_len)] for _ in range(2)]
    return hits, off, bases[0], bases[1], np.arange(n_reads + 1, dtype=np.int64) * read_len


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="samwrite_probe_out")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "samwrite_probe.json"))
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--refs", type=int, default=30_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--write-only", action="store_true")
    ap.add_argument("--oriented", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
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
    path = os.path.join(a.out, "mappings.sam")

    def device_write():
        with samfile.SamDeviceWriter(path, names, ref_len, True) as w:
            w.write(d_hits, d_off, seqs=d_seqs)
            return dict(w.stats)

    if a.write_only:
        for _ in range(3):
            st = device_write()
        print(json.dumps(st))
        return
    seqs = [(b1[i * a.read_len:(i + 1) * a.read_len].tobytes(), b2[i * a.read_len:(i + 1) * a.read_len].tobytes()) for i in range(a.reads)]
    device_write()
    samfile.write_sam(path + ".host", names, ref_len, hits, off, seqs=seqs)
    text = open(path, "rb").read()
    assert open(path + ".host", "rb").read() == text, "the device writer and write_sam disagree"
    runs, loops, copies = [], [], []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = device_write()
        runs.append(dict(st, device_write_s=time.perf_counter() - t0))
    for _ in range(0 if a.skip_host else a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        samfile.write_sam(path + ".host", names, ref_len, hits, off, seqs=seqs)
        loops.append(time.perf_counter() - t0)
    os.remove(path + ".host")
    n_bytes = runs[0]["bytes"]

    def plain_copies(n):
        src = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 255)
        dst = torch.empty(n, dtype=torch.uint8).pin_memory()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        out = []
        for i in range(a.repeats + 1):
            ev[0].record()
            dst.copy_(src, non_blocking=True)
            ev[1].record()
            torch.cuda.synchronize()
            if i:
                out.append(ev[0].elapsed_time(ev[1]))
        return out

    copies = plain_copies(n_bytes)
    med = statistics.median
    oriented = None
    if a.oriented:
        q1, q2 = (rng.integers(33, 127, a.reads * a.read_len).astype(np.uint8) for _ in range(2))
        d_quals = (up(q1), up(q2))
        qpath = os.path.join(a.out, "mappings.oriented.sam")

        def oriented_write():
            with samfile.SamDeviceWriter(qpath, names, ref_len, True, oriented=True) as w:
                w.write(d_hits, d_off, seqs=d_seqs, quals=d_quals)
                return dict(w.stats)

        oriented_write()
        L = a.read_len
        samfile.write_sam(qpath + ".host", names, ref_len, hits, off, seqs=seqs, oriented=True,
                          quals=[(q1[i * L:(i + 1) * L].tobytes(), q2[i * L:(i + 1) * L].tobytes()) for i in range(a.reads)])
        assert open(qpath + ".host", "rb").read() == open(qpath, "rb").read(), "the oriented device writer and write_sam disagree"
        os.remove(qpath + ".host")
        qruns = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = oriented_write()
            qruns.append(dict(st, device_write_s=time.perf_counter() - t0))
        qcopies = plain_copies(qruns[0]["bytes"])
        with open(qpath, "rb") as f:
            reversed_lines = sum(1 for l in f if not l.startswith(b"@") and int(l.split(b"\t", 2)[1]) & 0x10)
        oriented = dict(text_bytes=qruns[0]["bytes"], reversed_lines=reversed_lines, writer=qruns, plain_copy_ms=qcopies,
                        device_write_s_median=med(r["device_write_s"] for r in qruns), format_ms_median=med(r["ms_format"] for r in qruns),
                        d2h_ms_median=med(r["ms_copy"] for r in qruns), sink_ms_median=med(r["ms_sink"] for r in qruns),
                        plain_copy_ms_median=med(qcopies))
    rec = dict(reads=a.reads, hits=int(len(hits)), lines=runs[0]["lines"], file_bytes=len(text), text_bytes=n_bytes, device=torch.cuda.get_device_name(0),
               writer=runs, host_write_s=loops, plain_copy_ms=copies,
               device_write_s_median=med(r["device_write_s"] for r in runs), format_ms_median=med(r["ms_format"] for r in runs),
               d2h_ms_median=med(r["ms_copy"] for r in runs), sink_ms_median=med(r["ms_sink"] for r in runs),
               host_write_s_median=med(loops) if loops else None, plain_copy_ms_median=med(copies))
    if oriented is not None:
        rec["oriented"] = oriented
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
