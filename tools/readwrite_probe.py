"""Reads written as FASTQ from the device (sfgpu_reads_write_text / _bgzf; readfile.ReadDeviceWriter) at the size of two mapper
batches: 2 000 000 reads of 100 bases with 20-byte names and qualities, written plain and as BGZF, with every read selected and
with 5 % selected (what write_unmapped= selects on a good library).  A slice of the batch is written first and compared with
readfile.reads_text_host, and every leg's first file is read back and compared with the statement's size; then each leg is
written once to warm up and five times for the record.

Clocks: wall_s is host wall time (time.perf_counter) around write() + close(), after torch.cuda.synchronize(); ms_format / ms_copy /
ms_encode are device events and ms_sink the host clock inside the sink, from the writer's stats.  The yardsticks, in the same
process on the same arrays: plain_copy_ms, device events around one copy of as many bytes as the leg's text has into a pinned
buffer; host_loop_s, the per-record Python loop the writer replaces, over host copies of the arrays (the copies are not timed);
and sam_format_ms, the format time of samfile.SamDeviceWriter on a single-end batch of unmapped reads with names, bases and
qualities whose text has about as many bytes (sam_bytes says how many).

    python tools/readwrite_probe.py [--out DIR] [--json FILE] [--reads 2000000] [--repeats 5] [--skip-host]
Prints one JSON line and writes FILE (default profiles/readwrite_probe.json)."""
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
from sailfish_amd import readfile, samfile  # noqa: E402

READ_LEN, NAME_LEN = 100, 20


def batch(n, rng):
    """(bases, offsets, qualities, names, name offsets) on the host: n reads of READ_LEN bases with NAME_LEN-byte names"""
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n * READ_LEN)]
    quals = rng.integers(33, 127, n * READ_LEN).astype(np.uint8)
    names = np.frombuffer(b"".join(b"read.%015d" % i for i in range(n)), np.uint8).copy()
    return bases, np.arange(n + 1, dtype=np.int64) * READ_LEN, quals, names, np.arange(n + 1, dtype=np.int64) * NAME_LEN


def host_loop(path, bases, off, quals, names, name_off, select):
    """what the writer replaces: one write per selected record"""
    b, q, nm = bases.tobytes(), quals.tobytes(), names.tobytes()
    o, no = off.tolist(), name_off.tolist()
    with open(path, "wb") as f:
        for r in np.flatnonzero(select).tolist():
            f.write(b"@" + nm[no[r]:no[r + 1]] + b"\n" + b[o[r]:o[r + 1]] + b"\n+\n" + q[o[r]:o[r + 1]] + b"\n")


def device_write(path, d, select, compress):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w = readfile.ReadDeviceWriter(path, compress=compress)
    w.write((d["bases"], d["off"]), quals=d["quals"], names=(d["names"], d["name_off"]), select=select)
    w.close()
    return dict(wall_s=time.perf_counter() - t0, **w.stats)


def plain_copy_ms(n_bytes, dev):
    src = torch.empty(n_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(n_bytes, dtype=torch.uint8).pin_memory()
    out = []
    for _ in range(4):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); dst.copy_(src, non_blocking=True); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out[1:])


def sam_format(path, d, n, dev):
    """SamDeviceWriter over n unmapped single-end reads with names, bases and qualities -> (format ms, bytes), median of 3 after a warm-up"""
    off = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    hits = torch.zeros(0, dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(4):
        w = samfile.SamDeviceWriter(path, ["t0"], np.array([1000], np.uint32), False)
        w.write(hits, off, read_names=(d["names"][: n * NAME_LEN], d["name_off"][: n + 1]), seqs=(d["bases"][: n * READ_LEN], d["off"][: n + 1]),
                quals=d["quals"][: n * READ_LEN])
        w.close()
        runs.append((w.stats["ms_format"], w.stats["bytes"]))
    return statistics.median(r[0] for r in runs[1:]), runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="readwrite_probe_out")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "readwrite_probe.json"))
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    n = args.reads
    host = dict(zip(("bases", "off", "quals", "names", "name_off"), batch(n, rng)))
    d = {k: torch.from_numpy(v).to(dev) for k, v in host.items()}
    selects = {"all": np.ones(n, np.uint8), "5pct": (rng.random(n) < 0.05).astype(np.uint8)}

    # the writer against the statement on a slice, with a selector and with generated names
    m = min(n, 5000)
    seqs = [host["bases"][r * READ_LEN:(r + 1) * READ_LEN].tobytes() for r in range(m)]
    qs = [host["quals"][r * READ_LEN:(r + 1) * READ_LEN].tobytes() for r in range(m)]
    nms = [host["names"][r * NAME_LEN:(r + 1) * NAME_LEN].tobytes() for r in range(m)]
    p = os.path.join(args.out, "slice.fastq")
    with readfile.ReadDeviceWriter(p, chunk_bytes=1 << 16) as w:
        w.write((d["bases"][: m * READ_LEN], d["off"][: m + 1]), quals=d["quals"][: m * READ_LEN], names=(d["names"][: m * NAME_LEN], d["name_off"][: m + 1]),
                select=torch.from_numpy(selects["5pct"][:m]).to(dev))
        w.write((d["bases"][: m * READ_LEN], d["off"][: m + 1]), quals=d["quals"][: m * READ_LEN])
    want = readfile.reads_text_host(seqs, qs, nms, selects["5pct"][:m].tolist()) + readfile.reads_text_host(seqs, qs, None, None, m)
    assert open(p, "rb").read() == want, "the device writer and reads_text_host disagree"

    record = dict(reads=n, read_len=READ_LEN, name_len=NAME_LEN, repeats=args.repeats, device=torch.cuda.get_device_name(0), legs={})
    for sel_name, sel in selects.items():
        d_sel = torch.from_numpy(sel).to(dev)
        n_sel = int(sel.sum())
        text_bytes = n_sel * (NAME_LEN + 2 * READ_LEN + 6)
        for compress in (False, True):
            leg = f"{'bgzf' if compress else 'plain'}_{sel_name}"
            path = os.path.join(args.out, leg + (".fastq.gz" if compress else ".fastq"))
            runs = [device_write(path, d, d_sel, compress) for _ in range(args.repeats + 1)]
            assert runs[0]["reads_written"] == n_sel and runs[0]["bytes"] == text_bytes and os.path.getsize(path) == runs[0]["bytes_out"]
            if not compress:                               # the head and the tail of the file against the statement
                first = np.flatnonzero(sel)[:3].tolist()
                head = b"".join(readfile.reads_text_host([host["bases"][r * READ_LEN:(r + 1) * READ_LEN].tobytes()],
                                                         [host["quals"][r * READ_LEN:(r + 1) * READ_LEN].tobytes()],
                                                         [host["names"][r * NAME_LEN:(r + 1) * NAME_LEN].tobytes()]) for r in first)
                with open(path, "rb") as f:
                    assert f.read(len(head)) == head
            runs = runs[1:]
            med = lambda k: statistics.median(r[k] for r in runs)
            record["legs"][leg] = dict(selected=n_sel, text_bytes=text_bytes, file_bytes=runs[0]["bytes_out"], chunks=runs[0]["chunks"],
                                       wall_s=med("wall_s"), ms_format=med("ms_format"), ms_copy=med("ms_copy"), ms_encode=med("ms_encode"),
                                       ms_sink=med("ms_sink"), wall_s_runs=[r["wall_s"] for r in runs], ms_format_runs=[r["ms_format"] for r in runs])
        cmp_ = dict(plain_copy_ms=plain_copy_ms(text_bytes, dev))
        n_sam = max(1, min(n, text_bytes // (NAME_LEN + 2 * READ_LEN + 25)))
        cmp_["sam_format_ms"], cmp_["sam_bytes"] = sam_format(os.path.join(args.out, "yardstick.sam"), d, n_sam, dev)
        if not args.skip_host:
            hp = os.path.join(args.out, f"host_{sel_name}.fastq")
            t0 = time.perf_counter()
            host_loop(hp, host["bases"], host["off"], host["quals"], host["names"], host["name_off"], sel)
            cmp_["host_loop_s"] = time.perf_counter() - t0
            assert os.path.getsize(hp) == text_bytes
            with open(hp, "rb") as a, open(os.path.join(args.out, f"plain_{sel_name}.fastq"), "rb") as b:
                assert a.read() == b.read(), "the host loop and the device writer disagree"
        record["legs"][f"yardsticks_{sel_name}"] = cmp_
    line = json.dumps(record)
    print(line)
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
