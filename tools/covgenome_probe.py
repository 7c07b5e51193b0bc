"""dev probe: what the genome coverage (sfgpu_covg_*) costs -> profiles/covgenome_probe.json

On the coverage probe's batch (tools/coverage_probe.py: 80 000 transcripts, VERIFY_R error-free pairs of 2 x 100 bases, posteriors under
weights 10^U(-3, 3)) with a synthetic annotation generated here from a seed: genes of 4 isoforms that share a gene's exons of 150 to
400 bases from the first on (an isoform's last block is cut to its length), both strands, 24 chromosomes.  The device result on a
slice is first asserted equal to hits.coverage_genome_host.  Then medians of 5 after a warm-up of
 - the projection (sfgpu_covg_project): its wall ms and its stages -- count / scan / emit, the sort, gather / scan, the runs;
 - the genome file, plain and BGZF, into memory;
beside, in the same process, sfgpu_cov_finish on a fresh handle, the transcript file's write, torch.sort of as many 64-bit keys as
there are events, and a plain device copy of the events' bytes (16 a event: key and delta)."""
import argparse
import collections
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sailfish_amd as sf
from sailfish_amd import coverage as cov, genes, hits as H, synth

med = statistics.median
N_CHROM = 24


def annotation(ref_len, seed=39):
    """-> genes.Placement for transcripts of these lengths, and the host seconds it took"""
    t0 = time.perf_counter()
    rng = np.random.default_rng(seed)
    M = len(ref_len)
    chrom, strand, off, starts, lens = np.zeros(M, np.int32), np.zeros(M, np.int8), np.zeros(M + 1, np.int64), [], []
    cursor = [1000] * N_CHROM
    for g0 in range(0, M, 4):
        g = g0 // 4
        c, s = g % N_CHROM, 1 if (g // N_CHROM) % 2 == 0 else -1
        longest = int(ref_len[g0:g0 + 4].max())
        exons, total = [], 0
        while total < longest:
            exons.append(int(rng.integers(150, 401))); total += exons[-1]
        at, lo = [], 0                                     # the exons' offsets along the gene, introns of 200 to 2 000 bases between them
        for n in exons:
            at.append(lo); lo += n + int(rng.integers(200, 2001))
        span = at[-1] + exons[-1] if exons else 0
        for t in range(g0, min(g0 + 4, M)):
            chrom[t], strand[t], left = c, s, int(ref_len[t])
            for a, n in zip(at, exons):
                if left <= 0:
                    break
                n = min(n, left); left -= n
                starts.append(cursor[c] + (a if s > 0 else span - a - n)); lens.append(n)
            off[t + 1] = len(starts)
        cursor[c] += span + 5000
    pl = genes.Placement(np.zeros(M, np.uint8), chrom, strand, off, np.array(starts, np.uint32), np.array(lens, np.uint32), N_CHROM,
                         [b"chr%d" % (i + 1) for i in sorted(range(N_CHROM), key=lambda i: b"chr%d" % (i + 1))])
    return pl, time.perf_counter() - t0


def timed_wall(fn, reps):
    out = []
    for i in range(reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        if i:
            out.append((1e3 * (time.perf_counter() - t0), r))
    return out


def probe(M, R, reps, L=100):
    import verify_probe as VP
    dev, ACGT = VP.dev, VP.ACGT
    g = torch.Generator(device=dev); g.manual_seed(1)
    ref_len = synth.transcript_lengths(M, device=dev).long()
    off = torch.zeros(M + 1, dtype=torch.int64, device=dev); torch.cumsum(ref_len, 0, out=off[1:])
    N = int(off[-1])
    seq = ACGT[torch.randint(0, 4, (N,), generator=g, device=dev)]
    t = torch.randint(0, M, (R,), generator=g, device=dev)
    p0 = (torch.rand(R, generator=g, device=dev, dtype=torch.float64) * (ref_len[t] - 250).clamp_min(0).double()).long()
    comp = torch.zeros(256, dtype=torch.uint8, device=dev); comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    roff = torch.arange(R + 1, device=dev, dtype=torch.int64) * L
    index = sf.mapper.QuasiIndex((seq, off), device=dev)
    m1, m2 = VP.make_mates(seq, N, off[t] + p0, L, comp, g, 0.0)
    w = 10.0 ** (6 * torch.rand(M, generator=g, device=dev, dtype=torch.float64) - 3)
    names = [f"ENST{i:011d}.{i % 9 + 1}" for i in range(M)]
    d_names = cov._device_names(names, dev)
    len32 = ref_len.to(torch.int32)
    len_host = len32.cpu().numpy().view(np.uint32)
    pl, model_s = annotation(len_host)
    d_chrom_names = cov._device_names(pl.chrom_names, dev)
    hits, hoff = index.map_reads((m1.reshape(-1), roff), (m2.reshape(-1), roff))
    n = hits.numel() // 24
    p = H.posteriors(hits, hoff, w)[0]
    # a slice against the statement
    k = min(R, 5000)
    cut = int(hoff[k].item())
    with cov.CoverageDevice(len32, dev) as c:
        c.add(hits[: cut * 24], hoff[: k + 1], posteriors=p[:cut])
        c.finish()
        t_runs = tuple(x.cpu().numpy().view(dt) for x, dt in zip(c.runs(), (np.uint32, np.uint32, np.uint32, np.uint64)))
        with c.project(pl) as gc:
            got = tuple(x.cpu().numpy() for x in gc.runs())
            got_st = dict(gc.result)
    want, want_st = H.coverage_genome_host(t_runs, pl, len_host)
    assert all(np.array_equal(a.view(b.dtype), b) for a, b in zip(got, want)) and all(got_st[key] == want_st[key] for key in want_st), (got_st, want_st)
    # finish on a fresh handle each time; the last one is kept
    f_all, last = [], None
    for i in range(reps + 1):
        c = cov.CoverageDevice(len32, dev)
        c.add(hits, hoff, posteriors=p)
        res = c.finish()
        if i:
            f_all.append(res["finish_ms"])
        if i < reps:
            c.close()
        else:
            last = c
    # the projection
    gc = last.project(pl)
    runs = timed_wall(lambda: dict(gc.project(last)), reps)
    stage = {key: med([r[key] for _, r in runs]) for key in ("project_ms", "emit_ms", "sort_ms", "sum_ms", "runs_ms")}
    result = {key: v for key, v in gc.result.items() if not key.endswith("_ms")}
    # the two files
    legs = collections.OrderedDict()
    for leg, who, nm, kw in (("genome_text", gc, d_chrom_names, {}), ("genome_bgzf", gc, d_chrom_names, dict(compress=True)), ("transcript_text", last, d_names, {}),
                             ("transcript_bgzf", last, d_names, dict(compress=True))):
        sizes = []

        def write():
            f = io.BytesIO()
            r = who.write(f, nm, **kw)
            sizes.append(len(f.getvalue()))
            return r
        ws = timed_wall(write, reps)
        legs[leg] = dict(wall_ms=med([x for x, _ in ws]), format_ms=med([r["format_ms"] for _, r in ws]), d2h_ms=med([r["d2h_ms"] for _, r in ws]),
                         wall_ms_runs=[x for x, _ in ws], file_bytes=sizes[-1], text_bytes=int(ws[-1][1]["n_bytes"]))
    ne = max(int(result["n_events"]), 1)
    keys = torch.randint(0, 1 << 62, (ne,), generator=g, device=dev, dtype=torch.int64)
    sort_all = [x for x, _ in timed_wall(lambda: torch.sort(keys), reps)]
    src = torch.empty(16 * ne, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    copy_all = [x for x, _ in timed_wall(lambda: dst.copy_(src), reps)]
    gc.close(); last.close(); index.close()
    return dict(pairs=R, transcripts=M, bases=N, records=n, transcript_runs=int(last.result["runs"]), blocks=int(pl.exon_off[-1]), chromosomes=N_CHROM,
                annotation_host_s=model_s, result=result, project_wall_ms=med([x for x, _ in runs]), project_wall_ms_runs=[x for x, _ in runs], **stage,
                stage_ms_runs={key: [r[key] for _, r in runs] for key in stage}, sort_share=stage["sort_ms"] / stage["project_ms"] if stage["project_ms"] else None,
                bytes_per_event=result["state_bytes"] / ne, cov_finish_ms=med(f_all), cov_finish_ms_runs=f_all, writer=legs, torch_sort_ms=med(sort_all),
                torch_sort_ms_runs=sort_all, event_copy_ms=med(copy_all), event_copy_ms_runs=copy_all)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?", default=os.path.join(ROOT, "profiles", "covgenome_probe.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    M, R = int(os.environ.get("VERIFY_M", 80000)), int(os.environ.get("VERIFY_R", 10_000_000))
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, row=probe(M, R, a.repeats))
    with open(a.path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["row"]))
    print("wrote", a.path)
