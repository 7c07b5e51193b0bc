"""Read names from the FASTQ parser to the SAM writer, on the device against through the host, at run size and in one process:
  list    ReadFile(names=True) -> a Python list of bytes sliced from the name spans -> SamDeviceWriter.write(read_names=list)
          (packed again with quantfile.names_blob and uploaded): the path of the parent commit, which stays in the tree
  device  ReadFile(names="device") -> the (bytes, offsets) pair the parser wrote (sfgpu_reads_parse_*_n) -> write(read_names=pair)
on two mate files of --reads records (2 000 000; 2 x 100 bases, the record shape of tools/readfile_probe.py) whose reads are drawn
from --transcripts random transcripts, so that the mapper finds them.  Every batch is read, mapped (QuasiIndex.map_reads) and
written as SAM text (SamDeviceWriter) into a sink that hashes (the comparison) or counts (the timed runs) the bytes.  The SHA-256 of
the two mappings files are compared BEFORE anything is timed.

Clocks: *_s are host wall time (time.perf_counter) after torch.cuda.synchronize(), per batch of --batch reads: read_s (both mate
files), map_s, write_s and their sum batch_s; one warm-up run, then --repeats runs, medians over all their batches.  The parser's
ms_kernels (the library's device events) is measured apart, in fresh child processes on one text of --parse-mib MiB cut from the
mate 1 file, through both entries (host-staged and device text) with names off, with spans and with the blob; with --parent-lib the
same children run the parent commit's library (names off and spans: the unchanged paths) before and after the new one.

    python tools/readnames_probe.py [--json FILE] [--reads 2000000] [--batch 1000000] [--repeats 5] [--parent-lib libsfgpu_parent.so]
Prints one JSON line and writes FILE (default profiles/readnames_probe.json)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RECORD = 14 + 100 + 3 + 100 + 1                      # bytes of one record of write_reads at read_len 100


def write_reads(paths, n, read_len, frag, tx, tx_off, rng):
    """mate files of fixed-width records (the shape of readfile_probe.write_fastq) whose reads lie on the transcripts: mate 1 the
    first read_len bases of a fragment of `frag` bases, mate 2 the reverse complement of its last read_len"""
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    lens = np.diff(tx_off)
    with open(paths[0], "wb") as f1, open(paths[1], "wb") as f2:
        for a in range(0, n, 250_000):
            m = min(n, a + 250_000) - a
            t = rng.integers(0, len(lens), m)
            pos = tx_off[t] + (rng.random(m) * (lens[t] - frag + 1)).astype(np.int64)
            cols = np.arange(read_len)
            b1 = tx[pos[:, None] + cols]
            b2 = comp[tx[pos[:, None] + (frag - 1) - cols]]
            for mate, f, bases in ((1, f1, b1), (2, f2, b2)):
                name = np.char.add(np.char.add("@r", np.char.zfill(np.arange(a, a + m).astype(str), 9)), f"/{mate}\n").astype("S14")
                rec = np.empty((m, 14 + read_len + 1 + 2 + read_len + 1), np.uint8)
                rec[:, :14] = np.frombuffer(name.tobytes(), np.uint8).reshape(m, 14)
                rec[:, 14:14 + read_len] = bases
                rec[:, 14 + read_len:17 + read_len] = np.frombuffer(b"\n+\n", np.uint8)
                rec[:, 17 + read_len:-1] = rng.integers(33, 127, (m, read_len), dtype=np.uint8)
                rec[:, -1] = 10
                f.write(rec.tobytes())


class Sink:
    """what SamDeviceWriter writes into: counts the bytes, and hashes them when asked to"""

    def __init__(self, hashed):
        self.n, self.h = 0, hashlib.sha256() if hashed else None

    def write(self, b):
        self.n += len(b)
        if self.h is not None:
            self.h.update(b)
        return len(b)

    def flush(self):
        pass


def one_run(paths, idx, tnames, ref_len, mode, batch, dev, hashed=False):
    from sailfish_amd import readfile, samfile
    sink = Sink(hashed)
    w = samfile.SamDeviceWriter(sink, tnames, ref_len, True)
    rows, parse = [], None
    with readfile.ReadFile(paths[0], dev, names=mode) as f1, readfile.ReadFile(paths[1], dev) as f2:
        while True:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r1, r2 = f1.read(batch), f2.read(batch)
            n = int(r1[1].numel()) - 1
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if n == 0:
                break
            h, o = idx.map_reads(r1, r2)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            w.write(h, o, read_names=f1.last_names, seqs=(r1, r2))
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            rows.append(dict(reads=n, read_s=t1 - t0, map_s=t2 - t1, write_s=t3 - t2, batch_s=t3 - t0))
        parse = dict(mate1_ms_kernels=f1.stats["ms_kernels"], mate1_ms_copy=f1.stats["ms_copy"], mate1_calls=f1.stats["calls"],
                     mate2_ms_kernels=f2.stats["ms_kernels"])
    w.close()
    return dict(batches=rows, sam_bytes=sink.n, sha256=sink.h.hexdigest() if hashed else None, **parse)


# ---- the parser alone, by raw ctypes so that a library without the _n entries can be run too ---------------------------------

class Result(C.Structure):             # sfgpu_reads_result
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("consumed", C.c_uint64), ("n_lines", C.c_uint64),
                ("error_record", C.c_uint64), ("error_line", C.c_uint64), ("format", C.c_int32), ("error_kind", C.c_int32),
                ("ms_copy", C.c_double), ("ms_kernels", C.c_double)]


def parse_child(lib_path, text_path, repeats):
    """ms_kernels of one parse call on the text, per entry and per form of names -> JSON on stdout"""
    L = C.CDLL(lib_path)
    dev = torch.device("cuda:0")
    text = np.fromfile(text_path, np.uint8)
    n = int(text.size)
    max_reads = n // RECORD + 1
    P, U = C.c_void_p, C.c_uint64
    has_n = hasattr(L, "sfgpu_reads_parse_host_n")
    bases = torch.empty(n, dtype=torch.uint8, device=dev)
    off = torch.empty(max_reads + 1, dtype=torch.int64, device=dev)
    span = torch.empty(2 * max_reads, dtype=torch.int64, device=dev)
    blob = torch.empty((n + 15) & ~15, dtype=torch.uint8, device=dev)
    blob_off = torch.empty(max_reads + 1, dtype=torch.int64, device=dev)
    d_text = torch.zeros(((n + 16) & ~15) + 16, dtype=torch.uint8, device=dev)
    d_text[:n] = torch.from_numpy(text).to(dev)
    out = dict(library=os.path.basename(lib_path), bytes=n, has_blob_entries=has_n)
    stream = P(torch.cuda.current_stream().cuda_stream)
    for entry in ("host", "device"):
        src = [P(text.ctypes.data), U(n)] if entry == "host" else [P(d_text.data_ptr()), U(n), U(d_text.numel())]
        for form in ("off", "spans") + (("blob",) if has_n else ()):
            fn = getattr(L, f"sfgpu_reads_parse_{entry}_" + ("n" if form == "blob" else "q"))
            fn.restype = C.c_int
            args = src + [C.c_int(1), U(max_reads), P(bases.data_ptr()), P(0), U(n), P(off.data_ptr()), P(span.data_ptr() if form == "spans" else 0)]
            n_name = U(0)
            if form == "blob":
                args += [P(blob.data_ptr()), U(blob.numel()), P(blob_off.data_ptr()), C.byref(n_name)]
            ms, res = [], Result()
            for _ in range(repeats + 1):
                rc = fn(*args, C.byref(res), stream)
                torch.cuda.synchronize()
                assert rc == 0 and res.n_reads == n // RECORD, (rc, res.n_reads)
                ms.append(res.ms_kernels)
            if form == "blob":
                assert n_name.value == 12 * res.n_reads
            out[f"{entry}_{form}"] = dict(ms_kernels=ms[1:], median=statistics.median(ms[1:]))
    print(json.dumps(out))


def children(lib_path, text_path, repeats):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parse-child", lib_path, "--text", text_path, "--repeats", str(repeats)],
                       capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise RuntimeError(f"parse child on {lib_path} failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "readnames_probe.json"))
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--transcripts", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parse-mib", type=int, default=32)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parse-child", default=None)
    ap.add_argument("--text", default=None)
    a = ap.parse_args()
    if a.parse_child:
        return parse_child(a.parse_child, a.text, a.repeats)
    from sailfish_amd import _lib, mapper
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(47)
    props = torch.cuda.get_device_properties(0)
    rec = dict(reads=a.reads, batch=a.batch, read_len=100, transcripts=a.transcripts, repeats=a.repeats, device=torch.cuda.get_device_name(0),
               gcn_arch=getattr(props, "gcnArchName", None), compute_units=props.multi_processor_count)
    lens = rng.integers(500, 2501, a.transcripts)
    tx_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tx = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(tx_off[-1]))]
    tnames = ["ENST%011d" % t for t in range(a.transcripts)]
    idx = mapper.QuasiIndex((torch.from_numpy(tx).to(dev), torch.from_numpy(tx_off).to(dev)), device=dev)
    ref_len = idx.ref_len.cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, f"reads_{m}.fastq") for m in (1, 2)]
        t0 = time.perf_counter()
        write_reads(paths, a.reads, 100, 250, tx, tx_off, rng)
        rec["file_bytes"] = os.path.getsize(paths[0])
        note = lambda what: print(f"[readnames_probe] {what} ({time.perf_counter() - t0:.0f} s)", file=sys.stderr, flush=True)  # noqa: E731
        note("files written")
        rec["generate_s"] = time.perf_counter() - t0
        # the same file from both paths, before anything is timed
        legs = (("list", True), ("device", "device"))         # ReadFile's names=
        first = {mode: one_run(paths, idx, tnames, ref_len, arg, a.batch, dev, hashed=True) for mode, arg in legs}
        assert first["list"]["sha256"] == first["device"]["sha256"] and first["list"]["sam_bytes"] == first["device"]["sam_bytes"], \
            "the mappings written with device names differ from those written with the host list"
        rec["sam_bytes"], rec["sam_sha256"] = first["list"]["sam_bytes"], first["list"]["sha256"]
        note("the two mappings files are equal")
        for mode, arg in legs:
            runs = [one_run(paths, idx, tnames, ref_len, arg, a.batch, dev) for _ in range(a.repeats + 1)][1:]
            note(f"{mode}: timed")
            rows = [b for r in runs for b in r["batches"] if b["reads"] == a.batch] or [b for r in runs for b in r["batches"]]
            rec[mode] = dict(runs=runs, **{k + "_median": statistics.median(b[k] for b in rows) for k in ("read_s", "map_s", "write_s", "batch_s")},
                             mate1_ms_kernels_median=statistics.median(r["mate1_ms_kernels"] for r in runs),
                             mate2_ms_kernels_median=statistics.median(r["mate2_ms_kernels"] for r in runs))
        rec["batch_s_list_over_device"] = rec["list"]["batch_s_median"] / rec["device"]["batch_s_median"]
        # the parser alone
        text_path = os.path.join(tmp, "parse_text.fastq")
        k = min((a.parse_mib << 20) // RECORD, a.reads)
        with open(paths[0], "rb") as f, open(text_path, "wb") as g:
            g.write(f.read(k * RECORD))
        order = [("new", _lib.LIB_PATH)]
        if a.parent_lib:
            order = [("parent_run1", a.parent_lib), ("new", _lib.LIB_PATH), ("parent_run2", a.parent_lib)]
        rec["parse"] = dict(text_bytes=k * RECORD, records=k, **{label: children(os.path.abspath(p), text_path, a.repeats) for label, p in order})
    idx.close()
    print(json.dumps(rec))
    with open(a.json, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
