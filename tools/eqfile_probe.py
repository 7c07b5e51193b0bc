"""Class-file reader and writer at cfg3 size (sfgpu_eq_add_text_host, sfgpu_eqvec_write_text; sailfish_amd/eqfile.py): writes an
eq_classes.txt of the 400 M-read / 200 k-transcript synthetic experiment with the device writer and times the file read, the H2D
copy, the parse kernels, the fold + finish, requantify end to end, and the host baseline (a per-line Python parse feeding
insertGroups).  The write leg times eqfile.write_file (format kernels, D2H copies, the sink), the per-class Python loop the writer
used before, the numpy format_text, and a plain pinned D2H copy of the same bytes.

The table is the one the class build would make from cfg3's reads: pool labels (synth.label_pool, P = 4 M) drawn as
synth.reads_from_pool draws them (min of two uniform picks) -- each label's count is a binomial of R reads instead of 400 M reads
generated one by one -- folded through insertGroups and exported.  The file is written with eqfile.write_file and compared once
with eqfile.format_text; a small case checks first that format_text's bytes are writer.write_equiv_counts'.

    python tools/eqfile_probe.py [--out DIR] [--reads 400000000] [--parse-only] [--write] [--write-only] [--no-host]
Prints one JSON line.  --write: the write leg alone, with its baselines.  --parse-only: write the file and fold it once;
--write-only: write the file three times (both for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sailfish_amd as sf  # noqa: E402
from sailfish_amd import eqfile, synth  # noqa: E402


def check_writer_bytes(dev, tmp):
    M = 500
    ref_len, ids, off = synth.workload(M, 2000, 20_000, device="cpu")
    names = [f"t{i}" for i in range(M)]
    sopt = sf.SailfishOpts()
    exp = sf.ReadExperiment(sf.Transcripts(names, ref_len.numpy().view(np.uint32), device=dev), sopt)
    eq = exp.equivalenceClassBuilder(); eq.start(); eq.add_batch(ids.to(dev), off.to(dev)); eq.finish()
    sf.writer.write_equiv_counts(tmp, exp, sopt)
    rp, ii, cc, _ = eq.eqVec().to_numpy()
    assert eqfile.format_text(names, rp, ii, cc) == open(os.path.join(tmp, "aux", "eq_classes.txt"), "rb").read()


def cfg3_table(dev, M=200_000, P=4_000_000, R=400_000_000):
    poff, pids = synth.label_pool(M, P, device="cpu")
    p = np.arange(P, dtype=np.float64)
    prob = (2.0 * (P - p) - 1.0) / (float(P) * P)            # P(min(a, b) = p) for a, b uniform on [0, P)
    rng = np.random.default_rng(7)
    cnt = rng.binomial(R, prob).astype(np.uint64)
    hit = np.nonzero(cnt)[0]
    poff, pids = poff.numpy(), pids.numpy()
    k = poff[hit + 1] - poff[hit]
    rp = np.zeros(len(hit) + 1, np.int64); np.cumsum(k, out=rp[1:])
    idx = np.repeat(poff[hit], k) + (np.arange(int(rp[-1])) - np.repeat(rp[:-1], k))
    eq = sf.EquivalenceClassBuilder(device=dev); eq.start()
    eq.insertGroups(torch.from_numpy(pids[idx].astype(np.int32)).to(dev), torch.from_numpy(rp.astype(np.int32)).to(dev),
                    torch.from_numpy(cnt[hit].view(np.int64)).to(dev))
    eq.finish()
    rowptr, ids, counts, _ = eq.eqVec().to_numpy()
    ref_len = synth.transcript_lengths(M).numpy().view(np.uint32)
    return [f"ENST{i:011d}" for i in range(M)], ref_len, (rowptr, ids, counts), eq.eqVec()


def loop_write(path, names, rowptr, ids, counts):
    """writer.write_equiv_counts as it was before the device writer: one Python iteration per class over a host copy"""
    with open(path, "w") as f:
        f.write(f"{len(names)}\n{len(counts)}\n")
        for name in names:
            f.write(name + "\n")
        for c in range(len(counts)):
            lab = ids[rowptr[c]:rowptr[c + 1]]
            f.write(f"{len(lab)}\t" + "".join(f"{t}\t" for t in lab) + f"{counts[c]}\n")


def write_leg(a, dev, path, names, vec, text, rec):
    """eqfile.write_file against the loop, format_text (timed by the caller) and a plain pinned D2H copy of the class section"""
    runs = []
    for _ in range(4):                                       # the first run warms code objects, pools and the page cache
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = eqfile.write_file(path, names, vec)
        runs.append(dict(res, write_file_s=time.perf_counter() - t))
    assert open(path, "rb").read() == text
    rec["writer"] = runs[1:]
    rec["text_size"] = eqfile.text_size(vec)
    n = runs[-1]["n_bytes"]
    d = torch.zeros(n, dtype=torch.uint8, device=dev)
    h = torch.empty(n, dtype=torch.uint8).pin_memory()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ds = []
    for _ in range(4):
        e0.record(); h.copy_(d, non_blocking=True); e1.record(); e1.synchronize()
        ds.append(e0.elapsed_time(e1))
    rec["pinned_d2h_ms"] = ds[1:]
    t = time.perf_counter()
    with open(path + ".copy", "wb") as f:
        f.write(memoryview(h.numpy()))
    rec["plain_file_write_s"] = time.perf_counter() - t
    os.remove(path + ".copy")
    del d, h
    if not a.no_host:
        rowptr, ids, counts, _ = vec.to_numpy()
        t = time.perf_counter()
        loop_write(path + ".loop", names, rowptr, ids, counts)
        rec["python_loop_write_s"] = time.perf_counter() - t
        assert open(path + ".loop", "rb").read() == text
        os.remove(path + ".loop")


def host_parse(text, header):
    """the obvious host reader: one Python iteration per class line, then insertGroups"""
    ids, lens, counts = [], [], []
    for line in text[header.data_offset:].split(b"\n"):
        if not line:
            continue
        tok = line.split(b"\t")
        k = int(tok[0])
        ids.extend(map(int, tok[1:1 + k])); lens.append(k); counts.append(int(tok[-1]))
    off = np.zeros(len(lens) + 1, np.int64); np.cumsum(lens, out=off[1:])
    return np.asarray(ids, np.uint32), off, np.asarray(counts, np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="eqfile_probe_out")
    ap.add_argument("--reads", type=int, default=400_000_000)
    ap.add_argument("--parse-only", action="store_true")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--write-only", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    rec = {}
    check_writer_bytes(dev, os.path.join(a.out, "small"))
    names, ref_len, (rowptr, ids, counts), vec = cfg3_table(dev, R=a.reads)
    path = os.path.join(a.out, "eq_classes.txt")
    if a.write_only:
        for _ in range(3):
            res = eqfile.write_file(path, names, vec)
        print(json.dumps(dict(classes=len(counts), ids=len(ids), **res)))
        return
    t = time.perf_counter()
    text = eqfile.format_text(names, rowptr, ids, counts)
    rec["format_text_s"] = time.perf_counter() - t
    write_leg(a, dev, path, names, vec, text, rec)
    header = eqfile.read_header(path)
    rec.update(classes=len(counts), ids=len(ids), file_bytes=len(text), class_section_bytes=len(text) - header.data_offset)
    if a.write:
        print(json.dumps(rec))
        with open(os.path.join(a.out, "eqfile_probe_write.json"), "w") as f:
            json.dump(rec, f, indent=1)
        return

    def fold(chunk=0):
        eq = sf.EquivalenceClassBuilder(device=dev); eq.start()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eq.add_eq_file(path, names=names, chunk_bytes=chunk)
        t1 = time.perf_counter()
        eq.finish()
        t2 = time.perf_counter()
        return eq, res, t1 - t0, t2 - t1

    eq, res, _, _ = fold()                                    # warm-up (code objects, pools, page cache)
    if a.parse_only:
        print(json.dumps(dict(rec, parse_ms=res["parse_ms"], h2d_ms=res["h2d_ms"])))
        return
    want = eq.eqVec().to_numpy()
    runs = []
    for _ in range(3):
        eq, res, t_add, t_fin = fold()
        got = eq.eqVec().to_numpy()
        assert all(np.array_equal(x, y) for x, y in zip(got, want))
        runs.append(dict(res, add_eq_file_s=t_add, finish_s=t_fin))
    rec["reader"] = runs
    # the file read (page cache) and a plain pinned H2D of the same bytes
    t = time.perf_counter()
    with open(path, "rb") as f:
        blob = f.read()
    rec["file_read_s"] = time.perf_counter() - t
    h = torch.frombuffer(bytearray(blob), dtype=torch.uint8).pin_memory()
    d = torch.empty_like(h, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    hs = []
    for _ in range(3):
        e0.record(); d.copy_(h, non_blocking=True); e1.record(); e1.synchronize()
        hs.append(e0.elapsed_time(e1))
    rec["pinned_h2d_ms"] = hs
    del d, h
    # requantify end to end: a finished run's directory around the file
    prev, out2 = os.path.join(a.out, "run1"), os.path.join(a.out, "run2")
    sopt = sf.SailfishOpts(useVBOpt=True)
    rc, _ = sf.quant.quantify_eq_classes(names, ref_len, [path], prev, sopt, device=dev)
    assert rc == 0
    os.makedirs(os.path.join(prev, "aux"), exist_ok=True)
    os.replace(path, os.path.join(prev, "aux", "eq_classes.txt"))
    path = os.path.join(prev, "aux", "eq_classes.txt")
    rq = []
    for _ in range(2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        rc, exp = sf.quant.requantify(prev, out2, sf.SailfishOpts(useVBOpt=True), device=dev)
        assert rc == 0
        rq.append(dict(total_s=time.perf_counter() - t, **exp.timings, iters=exp.last_optimizer_stats["iters"],
                       reader=exp.eqfile_results[0]))
    rec["requantify"] = rq
    if not a.no_host:
        t = time.perf_counter()
        hid, hoff, hcnt = host_parse(blob, header)
        t_parse = time.perf_counter() - t
        heq = sf.EquivalenceClassBuilder(device=dev); heq.start()
        torch.cuda.synchronize()
        t = time.perf_counter()
        heq.insertGroups(torch.from_numpy(hid.view(np.int32)).to(dev), torch.from_numpy(hoff.astype(np.int32)).to(dev),
                         torch.from_numpy(hcnt.view(np.int64)).to(dev))
        heq.finish()
        t_fold = time.perf_counter() - t
        assert all(np.array_equal(x, y) for x, y in zip(heq.eqVec().to_numpy(), want))
        rec["host_baseline"] = dict(python_parse_s=t_parse, insert_groups_finish_s=t_fold)
    print(json.dumps(rec))
    with open(os.path.join(a.out, "eqfile_probe.json"), "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
