"""The coordinate-sorted BAM file with its BAI index written from the device (samfile.SamDeviceWriter(format="bam",
sort="coordinate"): csrc/bamsort.hip) on the batch of tools/bamwrite_probe.py -- 100 000 read pairs of 2 x 100 bases with 0 .. 3 hit
records each against 30 000 transcript names -- in one process beside the unsorted device writer and the host statements
samfile.write_bam(sort="coordinate") + samfile.build_bai.  Both device files are inflated and compared with the host statement, and
the device index with build_bai of the device file, before anything is timed.

Clocks: *_write_s are host wall time (time.perf_counter) around the whole writer, open to close, after torch.cuda.synchronize();
ms_format / ms_encode / ms_sort / ms_gather are device events, ms_index and ms_sink host clocks, from the writer's stats.  The first
run of each leg warms code objects, pools and the page cache and is dropped; the other five are all reported, with their median.
Yardsticks, not thresholds: ms_gather stands beside a plain device-to-device copy of the sorted stream's bytes; ms_sort -- device
events around the library's one sort_pairs_u64_u32 call and the index fill in front of it, nothing else -- beside torch.sort(stable)
of as many 64-bit keys (the library's sort is not exported on its own).

--unsorted-only times the unchanged writers ("sam", "sam.gz", "bam", sort=None) alone and prints their median format and encode
kernel times: run in fresh processes with SFGPU_LIB_PATH naming the parent commit's library, then this one's, then the parent's
again, the figures say whether the new median lies within the spread of the parent's runs.  A library older than the binding lacks
the new entries; the probe then binds only what the library exports.

    python tools/bamsort_probe.py [--out DIR] [--json FILE] [--reads 100000] [--repeats 5] [--unsorted-only]
Prints one JSON line and, without --unsorted-only, writes FILE (default profiles/bamsort_probe.json)."""
import argparse
import ctypes
import gzip
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from sailfish_amd import _lib, samfile  # noqa: E402
from samwrite_probe import batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bamsort_probe_out")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "bamsort_probe.json"))
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--refs", type=int, default=30_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--unsorted-only", action="store_true")
    a = ap.parse_args()
    if a.unsorted_only:                                   # an older library: bind what it exports
        have = ctypes.CDLL(_lib.LIB_PATH)
        _lib._SIGS = {k: v for k, v in _lib._SIGS.items() if hasattr(have, k)}
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    rng = np.random.default_rng(23)
    names = [f"ENST{i:011d}.{i % 9 + 1}" for i in range(a.refs)]
    ref_len = rng.integers(6200, 20000, a.refs)
    hits, off, b1, b2, boff = batch(a.reads, a.read_len, a.refs, rng)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(dev)  # noqa: E731
    d_hits, d_off = up(hits.view(np.uint8).reshape(-1)), up(off.view(np.int32))
    d_seqs = ((up(b1), up(boff)), (up(b2), up(boff)))
    med = statistics.median

    def device_write(path, fmt, **kw):
        with samfile.SamDeviceWriter(path, names, ref_len, True, format=fmt, **kw) as w:
            w.write(d_hits, d_off, seqs=d_seqs)
        return dict(w.stats)

    def timed(fn):
        runs = []
        for i in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = fn()
            if i:
                runs.append(dict(st or {}, write_s=time.perf_counter() - t0))
        return runs

    if a.unsorted_only:
        rec = dict(lib=_lib.LIB_PATH, reads=a.reads)
        for fmt in ("sam", "sam.gz", "bam"):
            runs = timed(lambda: device_write(os.path.join(a.out, "plain." + fmt), fmt))
            rec[fmt] = dict(ms_format=med(r["ms_format"] for r in runs), ms_format_runs=[r["ms_format"] for r in runs])
            if fmt != "sam":
                rec[fmt].update(ms_encode=med(r["ms_encode"] for r in runs), ms_encode_runs=[r["ms_encode"] for r in runs])
        print(json.dumps(rec))
        return

    seqs = [(b1[i * a.read_len:(i + 1) * a.read_len].tobytes(), b2[i * a.read_len:(i + 1) * a.read_len].tobytes()) for i in range(a.reads)]
    plain, sorted_, host = (os.path.join(a.out, n) for n in ("unsorted.bam", "sorted.bam", "host.sorted.bam"))

    def host_write():
        samfile.write_bam(host, names, ref_len, hits, off, seqs=seqs, sort="coordinate")
        with open(host + ".bai", "wb") as f:
            f.write(samfile.build_bai(host))

    device_write(plain, "bam")
    device_write(sorted_, "bam", sort="coordinate")
    host_write()
    want = gzip.decompress(open(host, "rb").read())
    stream = gzip.decompress(open(sorted_, "rb").read())
    assert stream == want, "the sorted device file does not inflate to write_bam(sort='coordinate')'s stream"
    assert samfile.sort_bam_stream(gzip.decompress(open(plain, "rb").read())) == want, "the unsorted device file holds other records"
    bai = open(sorted_ + ".bai", "rb").read()
    assert bai == samfile.build_bai(sorted_), "the device index is not build_bai of the device file"

    legs = dict(unsorted=timed(lambda: device_write(plain, "bam")), sorted=timed(lambda: device_write(sorted_, "bam", sort="coordinate")),
                sorted_no_index=timed(lambda: device_write(sorted_ + ".noindex", "bam", sort="coordinate", index=False)), host=timed(host_write))
    n_records, head = legs["sorted"][0]["records"], samfile._bam_header(stream)[2]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def device_ms(fn):
        out = []
        for i in range(a.repeats + 1):
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if i:
                out.append(ev[0].elapsed_time(ev[1]))
        return med(out)

    src = torch.empty(len(stream) - head, dtype=torch.uint8, device=dev).random_(0, 255)
    dst = torch.empty_like(src)
    keys = torch.from_numpy(rng.integers(0, 2 ** 62, n_records)).to(dev)
    rec = dict(reads=a.reads, hits=int(len(hits)), records=n_records, stream_bytes=len(stream), index_bytes=len(bai), device=torch.cuda.get_device_name(0),
               file_bytes={"unsorted": os.path.getsize(plain), "sorted": os.path.getsize(sorted_), "host sorted, level 6, 65280-byte members": os.path.getsize(host)},
               state_bytes=legs["sorted"][0]["state_bytes"], runs=legs,
               plain_device_copy_ms_of_the_stream=device_ms(lambda: dst.copy_(src)),
               torch_stable_sort_ms_of_as_many_keys=device_ms(lambda: torch.sort(keys, stable=True)))
    for leg, keys_ in (("unsorted", ("ms_format", "ms_encode", "ms_copy", "ms_sink")),
                       ("sorted", ("ms_format", "ms_encode", "ms_copy", "ms_sink", "ms_sort", "ms_gather", "ms_index")),
                       ("sorted_no_index", ("ms_format", "ms_encode", "ms_sort", "ms_gather")), ("host", ())):
        rec[leg + "_median"] = dict(write_s=med(r["write_s"] for r in legs[leg]), **{k: med(r[k] for r in legs[leg]) for k in keys_})
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
