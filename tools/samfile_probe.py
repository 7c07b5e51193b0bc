"""The SAM reader at run size (sfgpu_sam_*; sailfish_amd/samfile.py SamFile): a synthetic paired-end SAM file of about 2 000 000
fragments (100-base mates with SEQ, 1 .. 4 mappings per fragment, some orphans and unmapped reads; a body of --body fragments
drawn over synth.transcript_lengths, written by samfile.write_sam and repeated) through
  plain        the text file,
  bgzf         the same text as blocked gzip (gzfile.write_bgzf): inflated on the device,
  gzip         ordinary gzip level 6 with inflate="auto": inflated by Python's gzip module on the host,
  gzip_device  the same file with inflate="device" (sfgpu_gzrd_*),
each split into the wall time of iterating the SamFile end to end, its parse kernels (ms_kernels), its staged copies (ms_copy)
and, on the device paths, the inflate (ms_inflate), device events from the library's results;
  copy         a plain pinned host-to-device copy of the same bytes, the yardstick for the parse kernels,
  host         samfile.read_sam_host on a prefix of --prefix fragments, scaled to the file,
in one process.  The device result is compared with read_sam_host's on that prefix (exact records) BEFORE any time is reported.
The first run of each leg warms code objects, pools and the page cache and is dropped; medians of the rest are reported.

    python tools/samfile_probe.py [--out DIR] [--fragments 2000000] [--body 100000] [--prefix 20000] [--repeats 5]
Prints one JSON line and writes DIR/samfile_probe.json."""
import argparse
import gzip
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sailfish_amd import gzfile, samfile, synth  # noqa: E402
from sailfish_amd.hits import HIT_DTYPE  # noqa: E402

READ_LEN = 100


def synth_hits(n_frag, ref_len, seed=11):
    """hit records as a mapper leaves them: per fragment 0 .. 4 records ascending in tid, pairs, or (one fragment in ten) left orphans"""
    rng = np.random.default_rng(seed)
    per = rng.choice([0, 1, 1, 1, 1, 2, 2, 3, 4], n_frag)
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    frag = np.repeat(np.arange(n_frag), per)
    tid = rng.integers(0, len(ref_len), len(frag))
    tid = tid[np.lexsort((tid, frag))]
    h = np.zeros(len(frag), HIT_DTYPE)
    h["tid"] = tid
    h["pos"] = (rng.random(len(frag)) * (ref_len[tid] - 3 * READ_LEN)).astype(np.int32)
    h["read_len"] = READ_LEN
    h["fwd"] = rng.integers(0, 2, len(frag))
    orphan = (frag % 10 == 3)
    h["mate_status"] = np.where(orphan, 1, 3)
    gap = rng.integers(0, 2 * READ_LEN, len(frag))
    h["mate_pos"] = np.where(orphan, 0, h["pos"] + gap)
    h["mate_len"] = np.where(orphan, 0, READ_LEN)
    h["frag_len"] = np.where(orphan, 0, gap + READ_LEN)
    h["mate_fwd"] = np.where(orphan, 0, 1 - h["fwd"])
    return h, off


def make_text(path, n_frag, n_body, names, ref_len):
    """the file: one header, the body of n_body fragments repeated -> (fragments, body text of the first copy)"""
    hits, off = synth_hits(n_body, ref_len)
    rng = np.random.default_rng(5)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n_body, 2, READ_LEN))]
    seqs = [(bytes(m[0]), bytes(m[1])) for m in bases]
    samfile.write_sam(path, names, ref_len, hits, off, read_names=[f"frag{i}/x" for i in range(n_body)], seqs=seqs)
    text = open(path, "rb").read()
    cut = text.index(b"\nfrag0/x\t") + 1
    head, body = text[:cut], text[cut:]
    copies = max(1, round(n_frag / n_body))
    with open(path, "wb") as f:
        f.write(head)
        for _ in range(copies):
            f.write(body)
    return copies * n_body, head, body, hits, off


def read_all(path, dev, **kw):
    f = samfile.SamFile(path, dev, True, **kw)
    parts = [(h, o) for h, o in f]
    torch.cuda.synchronize()
    return parts, f.stats


def med(rows, k):
    return statistics.median(r[k] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="samfile_probe_out")
    ap.add_argument("--fragments", type=int, default=2_000_000)
    ap.add_argument("--body", type=int, default=100_000)
    ap.add_argument("--prefix", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--transcripts", type=int, default=100_000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    ref_len = np.maximum(synth.transcript_lengths(a.transcripts).numpy().astype(np.int64), 4 * READ_LEN)
    names = [f"ENST{t:011d}.{1 + t % 9}" for t in range(a.transcripts)]
    plain = os.path.join(a.out, "probe.sam")
    n_frag, head, body, hits, off = make_text(plain, a.fragments, min(a.body, a.fragments), names, ref_len)
    n_bytes = os.path.getsize(plain)

    # ---- the device reader against the contract, on a prefix
    n_pre = min(a.prefix, len(off) - 1)
    lines_pre = 2 * int(np.where(hits["mate_status"][: off[n_pre]] == 3, 1, 0).sum()) + int((hits["mate_status"][: off[n_pre]] != 3).sum()) + \
        2 * int((np.diff(off[: n_pre + 1].astype(np.int64)) == 0).sum())
    pre_text = head + b"\n".join(body.split(b"\n")[:lines_pre]) + b"\n"
    pre_path = os.path.join(a.out, "prefix.sam")
    with open(pre_path, "wb") as f:
        f.write(pre_text)
    t0 = time.perf_counter()
    want_hits, want_off = samfile.read_sam_host(pre_text, names, True)
    host_s = time.perf_counter() - t0
    assert len(want_off) - 1 == n_pre and np.array_equal(want_off, off[: n_pre + 1]), "the prefix does not hold the fragments it should"
    parts, _ = read_all(pre_path, dev, block_bytes=1 << 20)
    got_hits = np.concatenate([h.cpu().numpy().view(HIT_DTYPE) for h, _ in parts])
    got_off = np.concatenate([[0]] + [o.cpu().numpy().view(np.uint32)[1:].astype(np.int64) + base for (_, o), base in
                                      zip(parts, np.concatenate([[0], np.cumsum([int(o[-1]) for _, o in parts])[:-1]]))])
    assert got_hits.tobytes() == want_hits.tobytes() and np.array_equal(got_off, want_off), "the device records differ from read_sam_host's"
    host = [dict(read_sam_host_prefix_s=host_s)]
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        samfile.read_sam_host(pre_text, names, True)
        host.append(dict(read_sam_host_prefix_s=time.perf_counter() - t0))

    # ---- the carriers
    text = open(plain, "rb").read()
    bgzf, gz = os.path.join(a.out, "probe.sam.bgzf"), os.path.join(a.out, "probe.sam.gz")
    gzfile.write_bgzf(bgzf, text)
    with gzip.open(gz, "wb", compresslevel=6) as f:
        f.write(text)
    legs = {}
    for leg, path, kw in (("plain", plain, {}), ("bgzf", bgzf, {}), ("gzip", gz, {}), ("gzip_device", gz, dict(inflate="device"))):
        rows, first = [], None
        for _ in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parts, st = read_all(path, dev, **kw)
            rows.append(dict(samfile_s=time.perf_counter() - t0, **{k: st[k] for k in ("ms_kernels", "ms_copy", "ms_inflate", "blocks", "calls")}))
            counts = tuple(st[k] for k in ("lines", "header_lines", "reads", "hits", "pairs"))
            first = first or counts
            assert counts == first and st["reads"] == n_frag, (leg, counts, first)
            del parts
        legs[leg] = dict(file_bytes=os.path.getsize(path), runs=rows[1:], samfile_s_median=med(rows[1:], "samfile_s"),
                         ms_kernels_median=med(rows[1:], "ms_kernels"), ms_copy_median=med(rows[1:], "ms_copy"),
                         ms_inflate_median=med(rows[1:], "ms_inflate"), lines=first[0], reads=first[2], hits=first[3], pairs=first[4])
    assert len({(v["lines"], v["reads"], v["hits"], v["pairs"]) for v in legs.values()}) == 1, "the carriers disagree"

    # ---- the yardstick: the same bytes through one pinned buffer
    raw = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).pin_memory()
    dst = torch.empty_like(raw, device=dev)
    copy = []
    for _ in range(a.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(raw, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        copy.append(dict(pinned_copy_ms=e0.elapsed_time(e1)))

    props = torch.cuda.get_device_properties(0)
    scale = n_frag / n_pre
    rec = dict(fragments=n_frag, transcripts=a.transcripts, file_bytes=n_bytes, prefix_fragments=n_pre, device=torch.cuda.get_device_name(0),
               gcn_arch=getattr(props, "gcnArchName", None), compute_units=props.multi_processor_count, legs=legs, host_runs=host[1:],
               copy_runs=copy[1:], read_sam_host_prefix_s_median=med(host[1:], "read_sam_host_prefix_s"),
               read_sam_host_scaled_s=med(host[1:], "read_sam_host_prefix_s") * scale, pinned_copy_ms_median=med(copy[1:], "pinned_copy_ms"))
    rec["parse_kernels_over_copy"] = legs["plain"]["ms_kernels_median"] / rec["pinned_copy_ms_median"]
    for p in (plain, pre_path, bgzf, gz):
        os.remove(p)
    print(json.dumps(rec))
    with open(os.path.join(a.out, "samfile_probe.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
