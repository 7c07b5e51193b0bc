"""The BAM reader at run size (sfgpu_bam_*; sailfish_amd/samfile.py SamFile): about 2 000 000 synthetic paired-end fragments (the
file of tools/samfile_probe.py: 100-base mates with SEQ, 1 .. 4 mappings per fragment, some orphans and unmapped reads; a body of
--body fragments written by samfile.write_sam and repeated) once as
  bam     the BAM stream of those lines (samfile.sam_to_bam of the body, repeated) in BGZF members, and once as
  bgzf    the SAM text of the same records in BGZF members,
both through samfile.SamFile in one process: members inflated on the device, the records parsed where they land.  The two results
are compared first (counts and every batch's records after joining); then each leg is run --repeats + 1 times, the first run is
dropped, and medians are reported: wall time, ms_inflate, ms_kernels (the parse), ms_copy;
  copy    a plain pinned host-to-device copy of the inflated BAM bytes, the yardstick.
The claim to confirm is parse < inflate for the BAM leg (ms_kernels < ms_inflate).  The split of the parse into its stages comes
from a kernel trace of a run of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bamfile_probe.py --parse-only
    python tools/bamfile_probe.py --stats-csv DIR/.../*_kernel_stats.csv        (folds the kernels into tile / link / enumerate /
                                                                                  records / back end / inflate and adds them)

The stage times of the traced run are per read of the file (the trace holds --parse-only's two reads; the sums are halved).
--keep leaves the two probe files in DIR, and a run that finds them there reads them instead of building them.

    python tools/bamfile_probe.py [--out DIR] [--fragments 2000000] [--body 100000] [--repeats 5] [--keep] [--parse-only] [--stats-csv FILE]
Prints one JSON line and writes DIR/bamfile_probe.json."""
import argparse
import csv
import gzip
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sailfish_amd import gzfile, samfile, synth  # noqa: E402
from sailfish_amd.hits import HIT_DTYPE  # noqa: E402
from samfile_probe import READ_LEN, make_text  # noqa: E402

STAGES = (("tile", ("k_bam_tile",)), ("link", ("k_bam_super", "k_bam_walk", "k_bam_entries")), ("enumerate", ("k_bam_enum", "k_bam_compact")),
          ("records", ("k_bam_records", "k_bam_heads", "k_bam_cut", "k_bam_refs")),
          ("back_end", ("k_sam_pairs", "k_sam_survive", "k_sam_keys", "k_sam_write", "radix", "sort", "scan", "Scan", "Sort")),
          ("inflate", ("k_bgzf", "bgzf")))


def fold_stats(path, reads=2):
    """a rocprofv3 kernel stats file of --parse-only (two reads of the file) -> {stage: ms per read} (scans and sorts count as back end)"""
    out = {k: 0.0 for k, _ in STAGES}
    out["other"] = 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name, ns = row.get("Name", ""), float(row.get("TotalDurationNs", 0) or 0)
            stage = next((k for k, keys in STAGES if any(x in name for x in keys)), "other")
            out[stage] += ns / 1e6 / reads
    return out


def read_all(path, dev, **kw):
    f = samfile.SamFile(path, dev, True, **kw)
    parts = [(h, o) for h, o in f]
    torch.cuda.synchronize()
    return parts, f.stats, f.format


def joined(parts):
    hits = np.concatenate([h.cpu().numpy().view(HIT_DTYPE) for h, _ in parts])
    per_read = np.concatenate([np.diff(o.cpu().numpy().view(np.uint32).astype(np.int64)) for _, o in parts])
    return hits, per_read


def med(rows, k):
    return statistics.median(r[k] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="bamfile_probe_out")
    ap.add_argument("--fragments", type=int, default=2_000_000)
    ap.add_argument("--body", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--transcripts", type=int, default=100_000)
    ap.add_argument("--keep", action="store_true", help="leave probe.bam and probe.sam.bgzf in DIR")
    ap.add_argument("--parse-only", action="store_true", help="one warm-up and one read of the BAM file, nothing else (for a kernel trace)")
    ap.add_argument("--stats-csv", help="fold a rocprofv3 kernel stats file into the stages and add them to DIR/bamfile_probe.json")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    out_json = os.path.join(a.out, "bamfile_probe.json")
    if a.stats_csv:
        rec = json.load(open(out_json)) if os.path.exists(out_json) else {}
        rec["stage_ms_of_the_traced_run"] = fold_stats(a.stats_csv)
        print(json.dumps(rec["stage_ms_of_the_traced_run"]))
        with open(out_json, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        return
    dev = torch.device("cuda:0")
    ref_len = np.maximum(synth.transcript_lengths(a.transcripts).numpy().astype(np.int64), 4 * READ_LEN)
    names = [f"ENST{t:011d}.{1 + t % 9}" for t in range(a.transcripts)]
    bam_path, sam_path = os.path.join(a.out, "probe.bam"), os.path.join(a.out, "probe.sam.bgzf")
    n_body = min(a.body, a.fragments)
    n_frag = max(1, round(a.fragments / n_body)) * n_body
    if not (os.path.exists(bam_path) and os.path.exists(sam_path)):
        plain = os.path.join(a.out, "probe.sam")
        n_frag, head, body, _, _ = make_text(plain, n_body, n_body, names, ref_len)      # (one copy on disk; the repeats are made here)
        os.remove(plain)
        copies = max(1, round(a.fragments / n_body))
        n_frag *= copies
        first = samfile.sam_to_bam(head + body)
        header_bytes = samfile._bam_header(first)[2]
        gzfile.write_bgzf(bam_path, first[:header_bytes] + first[header_bytes:] * copies)
        gzfile.write_bgzf(sam_path, head + body * copies)

    def done():
        if not a.keep:
            os.remove(bam_path); os.remove(sam_path)

    if a.parse_only:
        for _ in range(2):
            parts, st, fmt = read_all(bam_path, dev)
        print(json.dumps(dict(format=fmt, reads=st["reads"], ms_kernels=st["ms_kernels"], ms_inflate=st["ms_inflate"])))
        done()
        return

    # ---- the two formats say the same
    (b_parts, b_st, b_fmt), (s_parts, s_st, s_fmt) = read_all(bam_path, dev), read_all(sam_path, dev)
    assert (b_fmt, s_fmt) == ("bam", "sam")
    assert all(b_st[k] == s_st[k] for k in ("reads", "hits", "pairs")) and b_st["reads"] == n_frag, (b_st, s_st)
    assert b_st["lines"] == s_st["lines"] - s_st["header_lines"]
    (bh, br), (sh, sr) = joined(b_parts), joined(s_parts)
    assert bh.tobytes() == sh.tobytes() and np.array_equal(br, sr), "the BAM records differ from the SAM records"
    del b_parts, s_parts, bh, sh

    legs = {}
    for leg, path in (("bam", bam_path), ("bgzf", sam_path)):
        rows = []
        for _ in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parts, st, _ = read_all(path, dev)
            rows.append(dict(samfile_s=time.perf_counter() - t0, **{k: st[k] for k in ("ms_kernels", "ms_copy", "ms_inflate", "blocks", "calls")}))
            del parts
        legs[leg] = dict(file_bytes=os.path.getsize(path), runs=rows[1:], **{k + "_median": med(rows[1:], k) for k in ("samfile_s", "ms_kernels", "ms_copy", "ms_inflate")})

    with gzip.open(bam_path, "rb") as f:
        stream = f.read()
    raw = torch.from_numpy(np.frombuffer(stream, np.uint8).copy()).pin_memory()
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
    rec = dict(fragments=n_frag, transcripts=a.transcripts, bam_stream_bytes=len(stream), records=b_st["lines"], device=torch.cuda.get_device_name(0),
               gcn_arch=getattr(props, "gcnArchName", None), compute_units=props.multi_processor_count, legs=legs, copy_runs=copy[1:],
               pinned_copy_ms_median=med(copy[1:], "pinned_copy_ms"))
    rec["bam_parse_below_inflate"] = legs["bam"]["ms_kernels_median"] < legs["bam"]["ms_inflate_median"]
    done()
    print(json.dumps(rec))
    with open(out_json, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
