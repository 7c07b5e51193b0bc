"""The collated SAM / BAM reader at run size (sfgpu_samc_*, sfgpu_sam_collect_*, sfgpu_bam_collect_*; samfile.SamFile(collate=True)):
one set of records -- about 2 000 000 paired-end fragments as tools/samfile_probe.py builds them, every copy of the body with
read names of its own -- written
  grouped_sam   name-grouped, as the mapper leaves it,
  sorted_sam    its alignment lines in (transcript, POS) order, unmapped lines last, as `samtools sort` leaves them,
  grouped_bam / sorted_bam   the same two as BAM (BGZF),
and read in one process:
  grouped_sam, grouped_bam by the name-grouped reader (the yardstick),
  all four with collate=True,
  copy          a plain pinned host-to-device copy of the SAM bytes.
Results are compared BEFORE any time is reported: the collated reading of a grouped file must equal the name-grouped reader's
records and offsets exactly; the sorted forms must give the same fragments, hits and pairs, the same multiset of records, and SAM
and BAM the same arrays.  The first run of each leg is dropped; medians of the rest: wall time of iterating the SamFile, and for the
collated reads ms_collect / ms_finish / ms_emit, sort_rounds and state_bytes.

    python tools/samcollate_probe.py [--out DIR] [--fragments 2000000] [--body 100000] [--repeats 5] [--no-bam]
Prints one JSON line and writes DIR/samcollate_probe.json."""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import samfile_probe as base  # noqa: E402
from sailfish_amd import gzfile, samfile, synth  # noqa: E402
from sailfish_amd.hits import HIT_DTYPE  # noqa: E402


def tag(c):
    """the four bytes that stand for "frag" in the read names of copy c"""
    return b"%04d" % c


def renamed(chunk, c, count):
    out = chunk.replace(b"frag", tag(c))
    assert out.count(tag(c)) >= count and len(out) == len(chunk)
    return out


def build(out, n_frag, n_body, names, ref_len, bam):
    """-> paths and sizes.  The body is written once by samfile.write_sam; a copy differs from it in the names alone."""
    plain = os.path.join(out, "grouped.sam")
    _, head, body, _, _ = base.make_text(plain, n_body, n_body, names, ref_len)
    copies = max(1, round(n_frag / n_body))
    lines = body.split(b"\n")[:-1]
    tid_of = {n.encode(): i for i, n in enumerate(names)}
    fields = [l.split(b"\t", 4) for l in lines]
    key_t = np.array([tid_of.get(f[2], len(names)) for f in fields], np.int64)
    key_p = np.array([int(f[3]) for f in fields], np.int64)
    # the order of the whole file: stable by (tid, POS) over (copy, line of the body)
    order = np.lexsort((np.tile(key_p, copies), np.tile(key_t, copies)))
    with open(plain, "wb") as f:
        f.write(head)
        for c in range(copies):
            f.write(renamed(body, c, len(lines)))
    sorted_sam = os.path.join(out, "sorted.sam")
    per_copy = [[l + b"\n" for l in renamed(body, c, len(lines)).split(b"\n")[:-1]] for c in range(copies)]
    n = len(lines)
    with open(sorted_sam, "wb") as f:
        f.write(head.replace(b"SO:unsorted\tGO:query", b"SO:coordinate"))
        f.write(b"".join(per_copy[i // n][i % n] for i in order.tolist()))
    del per_copy
    paths = dict(grouped_sam=plain, sorted_sam=sorted_sam)
    if bam:
        stream = samfile.sam_to_bam(head + body)
        h_bytes = samfile._bam_header(stream)[2]
        recs, p = [], h_bytes
        while p < len(stream):
            q = p + 4 + struct.unpack_from("<i", stream, p)[0]
            recs.append(stream[p:q]); p = q
        assert len(recs) == n
        body_bam = stream[h_bytes:]
        g = os.path.join(out, "grouped.bam")
        gzfile.write_bgzf(g, stream[:h_bytes] + b"".join(renamed(body_bam, c, n) for c in range(copies)))
        per_copy = [[r.replace(b"frag", tag(c)) for r in recs] for c in range(copies)]
        s = os.path.join(out, "sorted.bam")
        head_sorted = samfile.sam_to_bam(head.replace(b"SO:unsorted\tGO:query", b"SO:coordinate"))
        gzfile.write_bgzf(s, head_sorted + b"".join(per_copy[i // n][i % n] for i in order.tolist()))
        paths.update(grouped_bam=g, sorted_bam=s)
    return paths, copies * n_body, copies * n


def read_all(path, dev, **kw):
    f = samfile.SamFile(path, dev, True, **kw)
    parts = [(h, o) for h, o in f]
    torch.cuda.synchronize()
    return parts, f.stats


def joined(parts):
    hits = np.concatenate([np.zeros(0, HIT_DTYPE)] + [h.cpu().numpy().view(HIT_DTYPE) for h, _ in parts])
    off, at = [np.zeros(1, np.int64)], 0
    for _, o in parts:
        o = o.cpu().numpy().view(np.uint32).astype(np.int64)
        off.append(o[1:] + at); at += int(o[-1])
    return hits, np.concatenate(off)


def med(rows, k):
    return statistics.median(r[k] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="samcollate_probe_out")
    ap.add_argument("--fragments", type=int, default=2_000_000)
    ap.add_argument("--body", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--transcripts", type=int, default=100_000)
    ap.add_argument("--no-bam", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    ref_len = np.maximum(synth.transcript_lengths(a.transcripts).numpy().astype(np.int64), 4 * base.READ_LEN)
    names = [f"ENST{t:011d}.{1 + t % 9}" for t in range(a.transcripts)]
    t0 = time.perf_counter()
    paths, n_frag, n_lines = build(a.out, a.fragments, min(a.body, a.fragments), names, ref_len, not a.no_bam)
    build_s = time.perf_counter() - t0

    # ---- the results, compared first
    legs = [("grouped_sam", False), ("grouped_sam", True), ("sorted_sam", True)]
    if not a.no_bam:
        legs += [("grouped_bam", False), ("grouped_bam", True), ("sorted_bam", True)]
    want = joined(read_all(paths["grouped_sam"], dev)[0])
    multiset = np.sort(want[0].view(np.dtype((np.void, HIT_DTYPE.itemsize))))
    by_form = {}
    for form, collate in legs:
        hits, off = joined(read_all(paths[form], dev, collate=collate)[0])
        assert len(off) - 1 == n_frag, (form, collate, len(off) - 1, n_frag)
        if form.startswith("grouped"):
            assert hits.tobytes() == want[0].tobytes() and np.array_equal(off, want[1]), f"{form} (collate={collate}) differs from the name-grouped reading"
        else:
            assert np.array_equal(np.sort(hits.view(np.dtype((np.void, HIT_DTYPE.itemsize)))), multiset), f"{form}: other records than the grouped file's"
            by_form[form] = (hits, off)
    if "sorted_bam" in by_form:
        assert by_form["sorted_bam"][0].tobytes() == by_form["sorted_sam"][0].tobytes() and np.array_equal(by_form["sorted_bam"][1], by_form["sorted_sam"][1])
    del by_form, want, multiset

    # ---- the times
    out = {}
    keys = ("ms_kernels", "ms_copy", "ms_inflate", "calls")
    ckeys = ("ms_collect", "ms_finish", "ms_emit", "sort_rounds", "state_bytes", "fragments")
    for form, collate in legs:
        rows = []
        for _ in range(a.repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parts, st = read_all(paths[form], dev, collate=collate)
            rows.append(dict(samfile_s=time.perf_counter() - t0, **{k: st[k] for k in keys + (ckeys if collate else ())}))
            del parts
        rows = rows[1:]
        leg = dict(file_bytes=os.path.getsize(paths[form]), runs=rows, samfile_s_median=med(rows, "samfile_s"), ms_kernels_median=med(rows, "ms_kernels"),
                   ms_copy_median=med(rows, "ms_copy"), ms_inflate_median=med(rows, "ms_inflate"))
        if collate:
            leg.update({k + "_median": med(rows, k) for k in ("ms_collect", "ms_finish", "ms_emit")}, sort_rounds=rows[0]["sort_rounds"],
                       state_bytes=rows[0]["state_bytes"])
        out[form + ("_collated" if collate else "")] = leg

    raw = torch.from_numpy(np.fromfile(paths["grouped_sam"], np.uint8)).pin_memory()
    dst = torch.empty_like(raw, device=dev)
    copy = []
    for _ in range(a.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(raw, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        copy.append(e0.elapsed_time(e1))
    props = torch.cuda.get_device_properties(0)
    rec = dict(fragments=n_frag, alignment_lines=n_lines, transcripts=a.transcripts, build_s=build_s, device=torch.cuda.get_device_name(0),
               gcn_arch=getattr(props, "gcnArchName", None), compute_units=props.multi_processor_count, legs=out,
               pinned_copy_ms_median=statistics.median(copy[1:]))
    for p in paths.values():
        os.remove(p)
    print(json.dumps(rec))
    with open(os.path.join(a.out, "samcollate_probe.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
