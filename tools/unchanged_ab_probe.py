"""One leg of a parent / new / parent comparison of device paths that a change is meant to leave alone, each leg a fresh process:

 - the device writers (samfile.SamDeviceWriter, formats "sam", "sam.gz", "bam") on the batch of tools/samwrite_probe.py (100 000
   pairs of 2 x 100 bases, 0 .. 3 records each, 30 000 transcript names): host wall time of open + write + close into memory
   (io.BytesIO), after torch.cuda.synchronize(), and the formatter's device time from the writer's stats (`ms_format`);
 - sfgpu_hits_verify_gapped on a batch of tools/verify_probe.py (--pairs, default 2 M; 80 000 transcripts; 2 % substitutions, an
   indel of 1 - 3 bases in 5 % of the mates; max_indel 3, min identity 0.9): host wall time around the call, synchronised;
 - on that same batch, sfgpu_hits_verify (0.9), sfgpu_hits_align_gapped (max_indel 3) on the gapped pass's survivors, and
   sfgpu_hits_md_tags on those survivors with that alignment;
 - mapper.quantify_reads end to end on the first 100 000 pairs of that batch, every mapping option on (sorted oriented BAM with the
   gapped alignments and the tags, validation with max_indel 3, the unmapped reads), writing into a temporary directory: host wall
   time of the whole call.

 - with --coverage-only nothing of the above but, on the verification batch's records, the transcript coverage file
   (coverage.CoverageDevice: uniform weights, add and finish once, then write into memory, plain and BGZF): host wall time of the
   write, synchronised, and the format kernels' device time from its result.

Every figure is the median of --repeats (default 7) runs after one warm-up run; all runs are kept.  --root names the tree whose
`sailfish_amd` is measured (built there beforehand; default: the tree this file is in), so that the same driver measures a checkout
of the parent commit and this one:

    python tools/unchanged_ab_probe.py --label parent1 --root /path/to/parent/checkout --json profiles/NAME.json
    python tools/unchanged_ab_probe.py --label new --json profiles/NAME.json
    python tools/unchanged_ab_probe.py --label parent2 --root /path/to/parent/checkout --json profiles/NAME.json

Each call appends its leg to the `runs` of the JSON file (created if absent) and prints it as one line."""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
WHAT = ("parent / new / parent in fresh processes on one device, one call of tools/unchanged_ab_probe.py a leg: the device writers on the batch of "
        "tools/samwrite_probe.py (100 000 pairs; wall ms of SamDeviceWriter open + write + close into memory, and the formatter's device ms) and "
        "sfgpu_hits_verify_gapped on a batch of tools/verify_probe.py (2 % substitutions, an indel in 5 % of the mates, max_indel 3), with "
        "sfgpu_hits_verify on that batch, sfgpu_hits_align_gapped on the gapped pass's survivors and sfgpu_hits_md_tags on them with that alignment, "
        "and mapper.quantify_reads on the first 100 000 pairs with every mapping option on; medians of `repeats` runs after a warm-up")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--json", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--transcripts", type=int, default=80_000)
    ap.add_argument("--coverage-only", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import numpy as np
    import torch
    import sailfish_amd as sf                      # the measured tree's: imported before the probes below would find their own
    from sailfish_amd import _lib, samfile, synth
    assert os.path.samefile(os.path.dirname(os.path.dirname(sf.__file__)), a.root), sf.__file__
    sys.path.insert(0, HERE)
    import samwrite_probe
    import verify_probe

    dev = torch.device("cuda:0")
    med = statistics.median
    leg = dict(label=a.label, device=torch.cuda.get_device_name(0), repeats=a.repeats)

    # the writers
    if not a.coverage_only:
        writers(a, leg, dev, np, torch, samfile, samwrite_probe, med)
    rest(a, leg, dev, np, torch, sf, _lib, synth, verify_probe, med)


def writers(a, leg, dev, np, torch, samfile, samwrite_probe, med):
    rng = np.random.default_rng(23)
    n_reads, read_len, n_refs = 100_000, 100, 30_000
    names = [f"ENST{i:011d}.{i % 9 + 1}" for i in range(n_refs)]
    ref_len = rng.integers(6200, 20000, n_refs)
    hits, off, b1, b2, boff = samwrite_probe.batch(n_reads, read_len, n_refs, rng)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(dev)  # noqa: E731
    d_hits, d_off = up(hits.view(np.uint8).reshape(-1)), up(off.view(np.int32))
    d_seqs = ((up(b1), up(boff)), (up(b2), up(boff)))
    for fmt in ("sam", "sam.gz", "bam"):
        ms, ms_format, n_bytes = [], [], 0
        for i in range(a.repeats + 1):
            f = io.BytesIO()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with samfile.SamDeviceWriter(f, names, ref_len, True, format=fmt) as w:
                w.write(d_hits, d_off, seqs=d_seqs)
                st = dict(w.stats)
            dt = 1e3 * (time.perf_counter() - t0)
            n_bytes = len(f.getvalue())
            if i:
                ms.append(dt); ms_format.append(st["ms_format"])
        leg[fmt] = dict(ms=med(ms), ms_format=med(ms_format), ms_runs=ms, ms_format_runs=ms_format, bytes=n_bytes)



def coverage_writer(a, leg, dev, torch, sf, tlen, names, h, hoff, med):
    """the transcript coverage file of the records (h, hoff), plain and BGZF, into memory"""
    from sailfish_amd import coverage as cov
    d_names = cov._device_names(names, dev)
    with cov.CoverageDevice(tlen.to(torch.int32), dev) as c:
        c.add(h, hoff)
        res = c.finish()
        out = dict(runs=res["runs"])
        for kind, kw in (("text", {}), ("bgzf", dict(compress=True))):
            ms, fmt, size = [], [], 0
            for i in range(a.repeats + 1):
                f = io.BytesIO()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                w = c.write(f, d_names, **kw)
                torch.cuda.synchronize()
                if i:
                    ms.append(1e3 * (time.perf_counter() - t0)); fmt.append(w["format_ms"])
                size = len(f.getvalue())
            out[kind] = dict(ms=med(ms), ms_format=med(fmt), ms_runs=ms, ms_format_runs=fmt, bytes=size)
    leg["coverage_write"] = out


def rest(a, leg, dev, np, torch, sf, _lib, synth, verify_probe, med):
    # the gapped scoring pass
    M, R, L, K = a.transcripts, a.pairs, 100, 3
    ACGT = verify_probe.ACGT
    g = torch.Generator(device=dev); g.manual_seed(1)
    tlen = synth.transcript_lengths(M, device=dev).long()
    toff = torch.zeros(M + 1, dtype=torch.int64, device=dev); torch.cumsum(tlen, 0, out=toff[1:])
    N = int(toff[-1])
    seq = ACGT[torch.randint(0, 4, (N,), generator=g, device=dev)]
    t = torch.randint(0, M, (R,), generator=g, device=dev)
    p = (torch.rand(R, generator=g, device=dev, dtype=torch.float64) * (tlen[t] - 250).clamp_min(0).double()).long()
    comp = torch.zeros(256, dtype=torch.uint8, device=dev); comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    roff = torch.arange(R + 1, device=dev, dtype=torch.int64) * L
    index = sf.mapper.QuasiIndex((seq, toff), device=dev)
    m1, m2 = verify_probe.make_mates(seq, N, toff[t] + p, L, comp, g, 0.05)
    for m in (m1, m2):
        hit = torch.rand(m.shape, generator=g, device=dev) < 0.02
        m[hit] = ACGT[torch.randint(0, 4, (int(hit.sum()),), generator=g, device=dev)]
    r1, r2 = m1.reshape(-1), m2.reshape(-1)
    h, hoff = index.map_reads((r1, roff), (r2, roff))
    n = h.numel() // 24
    if a.coverage_only:
        coverage_writer(a, leg, dev, torch, sf, tlen, [f"ENST{i:011d}.{i % 9 + 1}" for i in range(M)], h, hoff, med)
        index.close()
        return finish(a, leg)
    out_hits, out_off, scores = torch.empty_like(h), torch.empty_like(hoff), torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=dev)
    go = _lib.VerifyGOpts(900, 0, K); gst = _lib.VerifyGStats(); n_out = C.c_uint64(0)
    Lb = _lib.lib()

    def gapped():
        _lib.check(Lb.sfgpu_hits_verify_gapped(index._h, _lib.ptr(r1), _lib.ptr(roff), _lib.ptr(r2), _lib.ptr(roff), R, _lib.ptr(h), _lib.ptr(hoff), C.byref(go),
                                               _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores), C.byref(n_out), C.byref(gst), None))
    g_ms, g_all = verify_probe.timed(gapped, a.repeats)
    leg["verify_gapped"] = dict(ms=g_ms, ms_runs=g_all, pairs=R, records=n, stats=gst.as_dict())
    s_hits, s_off = out_hits[: n_out.value * 24].clone(), out_off.clone()     # the gapped pass's survivors

    # the ungapped scoring pass on the same batch
    uo = _lib.VerifyOpts(900, 0); ust = _lib.VerifyStats()

    def ungapped():
        _lib.check(Lb.sfgpu_hits_verify(index._h, _lib.ptr(r1), _lib.ptr(roff), _lib.ptr(r2), _lib.ptr(roff), R, _lib.ptr(h), _lib.ptr(hoff), C.byref(uo),
                                        _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores), C.byref(n_out), C.byref(ust), None))
    u_ms, u_all = verify_probe.timed(ungapped, a.repeats)
    leg["verify"] = dict(ms=u_ms, ms_runs=u_all, pairs=R, records=n, stats=ust.as_dict())

    # the alignment of the gapped pass's survivors, with exactly the room it needs
    n_s = s_hits.numel() // 24
    pos, nm = torch.zeros(2 * n_s, dtype=torch.int32, device=dev), torch.zeros(2 * n_s, dtype=torch.int32, device=dev)
    op_off = torch.zeros(2 * n_s + 1, dtype=torch.int64, device=dev)
    ao = _lib.AlignGOpts(K, 0, 0); ast = _lib.AlignGStats(); need = C.c_uint64(0)
    al = (index._h, _lib.ptr(r1), _lib.ptr(roff), _lib.ptr(r2), _lib.ptr(roff), R, _lib.ptr(s_hits), _lib.ptr(s_off), C.byref(ao), _lib.ptr(pos), _lib.ptr(nm),
          _lib.ptr(op_off))
    rc = Lb.sfgpu_hits_align_gapped(*al, None, 0, C.byref(need), C.byref(ast), None)
    assert rc in (_lib.OK, _lib.ERR_RANGE), rc
    ops = torch.empty(max(need.value, 1), dtype=torch.int32, device=dev)

    def align():
        _lib.check(Lb.sfgpu_hits_align_gapped(*al, _lib.ptr(ops), ops.numel(), C.byref(need), C.byref(ast), None))
    a_ms, a_all = verify_probe.timed(align, a.repeats)
    leg["align_gapped"] = dict(ms=a_ms, ms_runs=a_all, records=n_s, stats=ast.as_dict())

    # the tags of those survivors over that alignment, with exactly the room they need
    md_off = torch.zeros(2 * n_s + 1, dtype=torch.int64, device=dev)
    mst = _lib.MdTagStats()
    ml = (index._h, _lib.ptr(r1), _lib.ptr(roff), _lib.ptr(r2), _lib.ptr(roff), R, _lib.ptr(s_hits), _lib.ptr(s_off), _lib.ptr(pos), _lib.ptr(op_off), _lib.ptr(ops),
          _lib.ptr(nm), _lib.ptr(md_off))
    rc = Lb.sfgpu_hits_md_tags(*ml, None, 0, C.byref(need), C.byref(mst), None)
    assert rc in (_lib.OK, _lib.ERR_RANGE), rc
    md = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)

    def tag():
        _lib.check(Lb.sfgpu_hits_md_tags(*ml, _lib.ptr(md), md.numel(), C.byref(need), C.byref(mst), None))
    t_ms, t_all = verify_probe.timed(tag, a.repeats)
    leg["md_tags"] = dict(ms=t_ms, ms_runs=t_all, records=n_s, stats=mst.as_dict())
    index.close()

    # the driver, from the reads to the files
    Q = min(R, 100_000)
    l1, l2 = ([row.tobytes() for row in m[:Q].cpu().numpy()] for m in (m1, m2))
    tnames = [f"t{i}" for i in range(M)]
    q_all, q_stats = [], {}
    for i in range(a.repeats + 1):
        with tempfile.TemporaryDirectory() as tmp:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            qrc, exp = sf.mapper.quantify_reads(tnames, (seq, toff), l1, l2, "IU", os.path.join(tmp, "out"), device=dev, cmd_options={"libType": "IU"},
                                                write_mappings=os.path.join(tmp, "m.bam"), mappings_format="bam", mappings_oriented=True, mappings_sorted=True,
                                                validate_mappings=True, max_indel=K, mappings_gapped=True, mappings_tags=True,
                                                write_unmapped=(os.path.join(tmp, "u1.fa"), os.path.join(tmp, "u2.fa")))
            torch.cuda.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            assert qrc == 0
            q_stats = dict(verify=exp.verify_stats, align=exp.align_stats, tags=exp.tag_stats, unmapped=exp.unmapped_stats, bam_bytes=os.path.getsize(os.path.join(tmp, "m.bam")))
        if i:
            q_all.append(dt)
    leg["quantify_reads"] = dict(ms=med(q_all), ms_runs=q_all, pairs=Q, stats=q_stats)

    finish(a, leg)


def finish(a, leg):
    print(json.dumps(leg), flush=True)
    doc = dict(what=WHAT, runs=[])
    if os.path.exists(a.json):
        with open(a.json) as f:
            doc = json.load(f)
    doc["runs"].append(leg)
    os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
    with open(a.json, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
