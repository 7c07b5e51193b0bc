"""A compressed read file at run size through readfile.ReadFile, in one process on the same text: the mate file of
tools/readfile_probe.py (--reads 2 000 000 reads of 100 bases) written as BGZF level 6 (gzfile.write_bgzf), as ordinary gzip
level 6, and plain.
  bgzf_device   ReadFile(bgzf): the device inflater (sfgpu_bgzf_inflate_host) and the parse of the device text
  bgzf_host     ReadFile(bgzf, inflate="host"): Python's gzip on one host thread, then the plain-text path -- what a .gz file cost
                before the device inflater
  gzip_host     ReadFile(ordinary gzip): the same host path, what inflate="auto" chooses for such a file
  gzip_device   ReadFile(ordinary gzip, inflate="device"): the chunked device inflater (sfgpu_gzrd_*: finder, two decode passes,
                window propagation) and the parse of the device text
  plain         ReadFile(plain text): the floor of every compressed path
and, beside them, bgzf_device_one_block and gzip_device_one_block: the device paths with block_bytes = the file's size, so that all
members (chunks) are in one launch (the inflate kernels are bound by the decode latency of one member or chunk, so their rate
grows with the number in flight).
The results are compared (bases and offsets, equal) BEFORE any time is reported.  *_s are host wall time
(time.perf_counter) around open .. read(all) .. torch.cuda.synchronize(); ms_* are the library's device events summed over the
calls of a file.  The first run of each path warms code objects, pools and the page cache and is dropped; the other --repeats
are all reported, with their medians.

    python tools/readgz_probe.py [--out DIR] [--reads 2000000] [--repeats 5]
Prints one JSON line and writes DIR/readgz_probe.json."""
import argparse
import gzip
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sailfish_amd import gzfile, readfile  # noqa: E402
from tools.readfile_probe import write_fastq  # noqa: E402


def run(path, dev, repeats, **kw):
    rows, result = [], None
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with readfile.ReadFile(path, dev, **kw) as rf:
            b, o = rf.read(1 << 62)
            torch.cuda.synchronize()
            rows.append(dict(wall_s=time.perf_counter() - t0, inflate=rf.inflate, **rf.stats))
        if result is None:
            result = (b, o)
        else:
            assert torch.equal(b, result[0]) and torch.equal(o, result[1]), f"{path}: two runs differ"
        del b, o
        print(f"# {os.path.basename(path)} {kw} {rows[-1]['wall_s']:.3f} s", file=sys.stderr, flush=True)
    runs = rows[1:]
    out = dict(file_bytes=os.path.getsize(path), runs=runs, wall_s_median=statistics.median(r["wall_s"] for r in runs))
    for k in ("ms_inflate", "ms_copy", "ms_kernels", "ms_find", "ms_decode", "ms_propagate", "ms_emit", "chunks", "candidates", "false_starts"):
        out[k + "_median"] = statistics.median(r[k] for r in runs)
    return out, result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="readgz_probe_out")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--read-len", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    props = torch.cuda.get_device_properties(0)
    rec = dict(reads=a.reads, read_len=a.read_len, repeats=a.repeats, device=torch.cuda.get_device_name(0),
               gcn_arch=getattr(props, "gcnArchName", None), compute_units=props.multi_processor_count)
    with tempfile.TemporaryDirectory() as tmp:
        plain, bgzf, gz = (os.path.join(tmp, "reads_1.fastq" + ext) for ext in ("", ".bgz", ".gz"))
        write_fastq(plain, a.reads, a.read_len, 1, np.random.default_rng(31))
        text = open(plain, "rb").read()
        t0 = time.perf_counter()
        gzfile.write_bgzf(bgzf, text, level=6)
        rec["write_bgzf_s"] = time.perf_counter() - t0
        print(f"# bgzf written in {rec['write_bgzf_s']:.1f} s", file=sys.stderr, flush=True)
        with gzip.open(gz, "wb", compresslevel=6) as f:
            f.write(text)
        print("# gzip written", file=sys.stderr, flush=True)
        rec["text_bytes"] = len(text)
        del text
        results = {}
        rec["bgzf_device"], results["bgzf_device"] = run(bgzf, dev, a.repeats)
        rec["bgzf_device_one_block"], results["bgzf_device_one_block"] = run(bgzf, dev, a.repeats, block_bytes=os.path.getsize(bgzf))
        rec["plain"], results["plain"] = run(plain, dev, a.repeats)
        rec["bgzf_host"], results["bgzf_host"] = run(bgzf, dev, a.repeats, inflate="host")
        rec["gzip_host"], results["gzip_host"] = run(gz, dev, a.repeats)
        rec["gzip_device"], results["gzip_device"] = run(gz, dev, a.repeats, inflate="device")
        rec["gzip_device_one_block"], results["gzip_device_one_block"] = run(gz, dev, a.repeats, inflate="device", block_bytes=os.path.getsize(gz))
    assert rec["bgzf_device"]["runs"][0]["inflate"] == "device" and rec["bgzf_host"]["runs"][0]["inflate"] == "host"
    assert rec["gzip_host"]["runs"][0]["inflate"] == "host" and rec["plain"]["runs"][0]["inflate"] is None
    assert rec["gzip_device"]["runs"][0]["inflate"] == "device" and rec["gzip_device"]["runs"][0]["chunks"] > 1
    for k, (b, o) in results.items():               # equal before any figure counts
        assert torch.equal(b, results["plain"][0]) and torch.equal(o, results["plain"][1]), f"{k} differs from the plain file's result"
    rec["records"] = int(results["plain"][1].numel()) - 1
    d, h, p = rec["bgzf_device"], rec["bgzf_host"], rec["plain"]
    rec["device_faster_than_host"] = d["wall_s_median"] < h["wall_s_median"]
    rec["host_over_device"] = h["wall_s_median"] / d["wall_s_median"]
    rec["device_over_plain"] = d["wall_s_median"] / p["wall_s_median"]
    rec["inflate_output_GB_per_s"] = rec["text_bytes"] / (d["ms_inflate_median"] * 1e-3) / 1e9
    rec["inflate_output_GB_per_s_one_block"] = rec["text_bytes"] / (rec["bgzf_device_one_block"]["ms_inflate_median"] * 1e-3) / 1e9
    g, gh = rec["gzip_device"], rec["gzip_host"]
    rec["gzip_device_faster_than_host"] = g["wall_s_median"] < gh["wall_s_median"]
    rec["gzip_host_over_device"] = gh["wall_s_median"] / g["wall_s_median"]
    rec["gzip_host_over_device_one_block"] = gh["wall_s_median"] / rec["gzip_device_one_block"]["wall_s_median"]
    rec["gzip_device_over_bgzf_device"] = g["wall_s_median"] / d["wall_s_median"]
    print(json.dumps(rec))
    with open(os.path.join(a.out, "readgz_probe.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
