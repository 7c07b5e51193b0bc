"""dev probe: what the posterior pass (sfgpu_hits_posteriors) and the ZW tag cost -> profiles/posterior_probe.json

 - the pass on the batch of tools/verify_probe.py (80 000 transcripts, VERIFY_R pairs of 2 x 100 bases from fragments of 250,
   error-free), weights 10^U(-3, 3): its result on a slice is first asserted equal to hits.posteriors_host; then medians of 5 after a
   warm-up of sfgpu_hits_posteriors, of sfgpu_hits_verify on the same records, and of a plain device-to-device copy of the bytes the
   pass moves (24 bytes a record read and 4 written by the tid pass; 4 + 16 bytes a record and 4 a read by the read pass; the weight
   table twice);
 - the writers on the batch of tools/samwrite_probe.py / tools/bamwrite_probe.py (100 000 pairs, 0 .. 3 records each), oriented, with
   the bases: SamDeviceWriter "sam", "sam.gz" and "bam" into memory, untagged (the _a entries), with made-up tags (_t), with tags and
   posteriors and with posteriors alone (_p): the format kernels' ms, the copies' ms and the wall ms of open + write + close;
 - mapper.quantify_files on two mate files of tools/readnames_probe.py (--reads pairs on --transcripts transcripts, plain FASTQ) with
   and without mappings_posteriors=True: wall time of the whole call, the difference being the second pass over the reads."""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sailfish_amd as sf
from sailfish_amd import _lib, hits as H, samfile, synth

med = statistics.median


def pass_cost(M, R, L=100):
    import verify_probe as VP
    dev, ACGT = VP.dev, VP.ACGT
    g = torch.Generator(device=dev); g.manual_seed(1)
    ref_len = synth.transcript_lengths(M, device=dev).long()
    off = torch.zeros(M + 1, dtype=torch.int64, device=dev); torch.cumsum(ref_len, 0, out=off[1:])
    N = int(off[-1])
    seq = ACGT[torch.randint(0, 4, (N,), generator=g, device=dev)]
    t = torch.randint(0, M, (R,), generator=g, device=dev)
    p = (torch.rand(R, generator=g, device=dev, dtype=torch.float64) * (ref_len[t] - 250).clamp_min(0).double()).long()
    comp = torch.zeros(256, dtype=torch.uint8, device=dev); comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    roff = torch.arange(R + 1, device=dev, dtype=torch.int64) * L
    index = sf.mapper.QuasiIndex((seq, off), device=dev)
    m1, m2 = VP.make_mates(seq, N, off[t] + p, L, comp, g, 0.0)
    r1, r2 = (m1.reshape(-1), roff), (m2.reshape(-1), roff)
    hits, hoff = index.map_reads(r1, r2)
    w = 10.0 ** (6 * torch.rand(M, generator=g, device=dev, dtype=torch.float64) - 3)
    # the pass on a slice against the statement
    k = min(R, 5000)
    cut = int(hoff[k].item())
    dp, drec, df32, dst = H.posteriors(hits[: cut * 24], hoff[: k + 1], w)
    wp, wrec, wf32, wst = H.posteriors_host(hits[: cut * 24].cpu().numpy().view(H.HIT_DTYPE), hoff[: k + 1].cpu().numpy().view(np.uint32), w.cpu().numpy())
    assert np.array_equal(dp.cpu().numpy().view(np.uint64), wp.view(np.uint64)) and np.array_equal(drec.cpu().numpy().view(np.uint32), wrec)
    assert np.array_equal(df32.cpu().numpy().view(np.uint32), wf32.view(np.uint32)) and dst == wst, (dst, wst)
    # the whole batch
    n = hits.numel() // 24
    po, rec, f32 = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    st = _lib.PosteriorStats()
    Lb = _lib.lib()

    def post():
        _lib.check(Lb.sfgpu_hits_posteriors(_lib.ptr(hits), _lib.ptr(hoff), R, _lib.ptr(w), M, _lib.ptr(po), _lib.ptr(rec), _lib.ptr(f32), C.byref(st), None))
    out_hits, out_off, scores = torch.empty_like(hits), torch.empty_like(hoff), torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=dev)
    o = _lib.VerifyOpts(900, 0); vst = _lib.VerifyStats(); n_out = C.c_uint64(0)

    def verify():
        _lib.check(Lb.sfgpu_hits_verify(index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(hits), _lib.ptr(hoff), C.byref(o),
                                        _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores), C.byref(n_out), C.byref(vst), None))
    p_ms, p_all = VP.timed(post)
    v_ms, v_all = VP.timed(verify)
    moved = (24 + 4 + 4 + 16) * n + 4 * (R + 1) + 2 * 8 * M
    src = torch.empty(moved, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    c_ms, c_all = VP.timed(lambda: dst.copy_(src))
    row = dict(pairs=R, transcripts=M, records=n, stats=st.as_dict(), posteriors_ms=p_ms, posteriors_ms_runs=p_all, verify_ms=v_ms, verify_ms_runs=v_all,
               bytes_moved=moved, d2d_copy_ms=c_ms, d2d_copy_ms_runs=c_all, posteriors_over_verify=p_ms / v_ms, posteriors_over_copy=p_ms / c_ms,
               posteriors_ms_per_10M_pairs=p_ms * 1e7 / R)
    index.close()
    print(json.dumps(row), flush=True)
    return row


def writer_cost(repeats, n_reads=100_000, read_len=100, n_refs=30_000):
    import samwrite_probe
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(23)
    names = [f"ENST{i:011d}.{i % 9 + 1}" for i in range(n_refs)]
    ref_len = rng.integers(6200, 20000, n_refs)
    hits, off, b1, b2, boff = samwrite_probe.batch(n_reads, read_len, n_refs, rng)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).to(dev)  # noqa: E731
    d_hits, d_off = up(hits.view(np.uint8).reshape(-1)), up(off.view(np.int32))
    d_seqs = ((up(b1), up(boff)), (up(b2), up(boff)))
    n = len(hits)
    md = np.frombuffer(b"100" * (2 * n), np.uint8)                       # made-up tags: nm 0 and MD "100" on every slot
    tags = (torch.zeros(2 * n, dtype=torch.int32, device=dev), up(3 * np.arange(2 * n + 1, dtype=np.int64)), up(md))
    w = torch.from_numpy(10.0 ** rng.uniform(-3, 3, n_refs)).to(dev)
    post = H.posteriors(d_hits, d_off, w)[:3]
    out = {}
    for fmt in ("sam", "sam.gz", "bam"):
        for leg, kw in (("untagged", {}), ("tags", dict(tags=tags)), ("tags_posteriors", dict(tags=tags, posteriors=post)), ("posteriors", dict(posteriors=post))):
            ms, fmt_ms, copy_ms, n_bytes = [], [], [], 0
            for i in range(repeats + 1):
                f = io.BytesIO()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with samfile.SamDeviceWriter(f, names, ref_len, True, format=fmt, oriented=True) as wr:
                    wr.write(d_hits, d_off, seqs=d_seqs, **kw)
                    st = dict(wr.stats)
                dt = 1e3 * (time.perf_counter() - t0)
                n_bytes = len(f.getvalue())
                if i:
                    ms.append(dt); fmt_ms.append(st["ms_format"]); copy_ms.append(st["ms_copy"])
            out[f"{fmt}:{leg}"] = dict(ms=med(ms), ms_format=med(fmt_ms), ms_copy=med(copy_ms), ms_runs=ms, ms_format_runs=fmt_ms, bytes=n_bytes)
            print(json.dumps({f"{fmt}:{leg}": out[f"{fmt}:{leg}"]}), flush=True)
    return dict(pairs=n_reads, records=n, legs=out)


def driver_cost(repeats, reads, transcripts, batch):
    import readnames_probe
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(47)
    lens = rng.integers(500, 2501, transcripts)
    tx_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tx = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(tx_off[-1]))]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        paths = [os.path.join(tmp, f"reads_{m}.fastq") for m in (1, 2)]
        readnames_probe.write_reads(paths, reads, 100, 250, tx, tx_off, rng)
        fa = os.path.join(tmp, "tx.fa")
        with open(fa, "wb") as f:
            for t in range(transcripts):
                f.write(b">ENST%011d\n" % t + tx[tx_off[t]:tx_off[t + 1]].tobytes() + b"\n")
        stats = None
        for leg, kw in (("without", {}), ("with", dict(mappings_posteriors=True))):
            ms = []
            for i in range(repeats + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc, exp = sf.mapper.quantify_files(fa, paths[0], paths[1], "IU", os.path.join(tmp, "out_" + leg), sf.SailfishOpts(), device=dev, batch_reads=batch,
                                                   cmd_options={"libType": "IU"}, write_mappings=os.path.join(tmp, leg + ".sam"), **kw)
                torch.cuda.synchronize()
                assert rc == 0
                if i:
                    ms.append(1e3 * (time.perf_counter() - t0))
                stats = exp.posterior_stats or stats
            out[leg] = dict(ms=med(ms), ms_runs=ms, sam_bytes=os.path.getsize(os.path.join(tmp, leg + ".sam")))
            print(json.dumps({leg: out[leg]}), flush=True)
        assert open(os.path.join(tmp, "out_with", "quant.sf"), "rb").read() == open(os.path.join(tmp, "out_without", "quant.sf"), "rb").read()
    return dict(pairs=reads, transcripts=transcripts, batch_reads=batch, legs=out, posterior_stats=stats, second_pass_ms=out["with"]["ms"] - out["without"]["ms"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?", default=os.path.join(ROOT, "profiles", "posterior_probe.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--batch", type=int, default=1_000_000)
    ap.add_argument("--transcripts", type=int, default=20_000)
    a = ap.parse_args()
    M, R = int(os.environ.get("VERIFY_M", 80000)), int(os.environ.get("VERIFY_R", 10_000_000))
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats)
    doc["pass"] = pass_cost(M, R)
    doc["writers"] = writer_cost(a.repeats)
    doc["driver"] = driver_cost(a.repeats, a.reads, a.transcripts, a.batch)
    with open(a.path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.path)
