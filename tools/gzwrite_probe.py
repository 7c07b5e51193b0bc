"""bootstraps.gz at cfg5's size, both ways: the host path (writer.BootstrapWriter.__call__ as the samplers' per-sample
callback: zlib level 6 on one CPU thread) and the device path (BootstrapWriter.write_device over the samplers' matrix,
sfgpu_gz_*; sailfish_amd/csrc/gzwrite.hip), on the same samples, alternating.

The experiment is cfg3 / cfg5's table (tools/eqfile_probe.cfg3_table: 200 k transcripts, the classes of 400 M reads); the EM runs
once, then for Gibbs draws (--gibbs, default 1000) and bootstrap replicates (--boot, default 100) the sample-writing phase is timed
as quant._quantify_tail runs it (timings["samples_s"]: sampler + writer), plus the sampler alone, the encoder's own counters
(encode_ms / d2h_ms / sink_ms from device events), a plain pinned device-to-host copy of the same bytes, and the sizes against
zlib level 6 on a slice.  The host path is timed on --host-gibbs / --host-boot samples (default 50 / 10) and scaled by the count:
it is one sample at a time, so its time is linear in the number of samples.

    python tools/gzwrite_probe.py [--out DIR] [--gibbs N] [--boot N] [--reads R] [--encode-only]
Prints one JSON line.  --encode-only: three device writes of the Gibbs matrix and nothing else (for rocprofv3 --kernel-trace --stats,
and for an A/B of two builds: the line holds every write's result)."""
import argparse
import gzip
import json
import os
import sys
import time
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sailfish_amd as sf  # noqa: E402
from eqfile_probe import cfg3_table  # noqa: E402


def level6(raw):
    o = zlib.compressobj(6, zlib.DEFLATED, 31)
    return len(o.compress(raw) + o.flush())


def write_both(out, sopt, mat, n_host, rec, key):
    """the device writer over the whole matrix (3 runs after a warm-up), the host writer over the first n_host rows"""
    runs = []
    for i in range(4):
        w = sf.writer.BootstrapWriter(os.path.join(out, f"{key}_dev"), sopt)
        torch.cuda.synchronize()
        t = time.perf_counter()
        w.write_device(mat)
        w.close()
        runs.append(dict(w.last_result, wall_s=time.perf_counter() - t))
    rec[key + "_device_writer"] = runs[1:]
    nbytes = mat.numel() * mat.element_size()
    rec[key + "_bytes"] = nbytes
    rec[key + "_encode_GBps_in"] = [nbytes / r["encode_ms"] / 1e6 for r in runs[1:]]
    host = mat[:n_host].cpu().numpy()
    w = sf.writer.BootstrapWriter(os.path.join(out, f"{key}_host"), sopt)
    t = time.perf_counter()
    for row in host:
        w(row)
    w.close()
    dt = time.perf_counter() - t
    rec[key + "_host_writer"] = dict(samples=n_host, wall_s=dt, MBps=host.nbytes / dt / 1e6, scaled_to_all_s=dt * mat.shape[0] / n_host)
    # same payload, and the sizes on the rows both wrote
    dev_payload = gzip.open(os.path.join(out, f"{key}_dev", "aux", "bootstrap", "bootstraps.gz")).read(host.nbytes)
    assert dev_payload == host.tobytes()
    one = sf.writer.BootstrapWriter(os.path.join(out, f"{key}_dev_part"), sopt)
    one.write_device(mat[:n_host]); one.close()
    rec[key + "_size_vs_level6"] = one.last_result["n_bytes_out"] / level6(host.tobytes())
    rec[key + "_ratio"] = host.nbytes / one.last_result["n_bytes_out"]
    rec[key + "_distinct_values_row0"] = int(len(np.unique(host[0])))
    d = torch.empty(runs[-1]["n_bytes_out"], dtype=torch.uint8, device=mat.device)
    h = torch.empty(runs[-1]["n_bytes_out"], dtype=torch.uint8).pin_memory()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ds = []
    for _ in range(4):
        e0.record(); h.copy_(d, non_blocking=True); e1.record(); e1.synchronize()
        ds.append(e0.elapsed_time(e1))
    rec[key + "_pinned_d2h_of_output_ms"] = ds[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="gzwrite_probe_out")
    ap.add_argument("--gibbs", type=int, default=1000)
    ap.add_argument("--boot", type=int, default=100)
    ap.add_argument("--host-gibbs", type=int, default=50)
    ap.add_argument("--host-boot", type=int, default=10)
    ap.add_argument("--reads", type=int, default=400_000_000)
    ap.add_argument("--encode-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    names, ref_len, _, vec = cfg3_table(dev, R=a.reads)
    sopt = sf.SailfishOpts()
    exp = sf.ReadExperiment(sf.Transcripts(names, ref_len, device=dev), sopt)
    eq = exp.equivalenceClassBuilder(); eq.start()
    eq.insertGroups(vec.ids, vec.rowptr, vec.counts); eq.finish()
    exp.setNumMappedFragments(eq.total_reads)
    sf.efflen.set_effective_lengths(exp, sopt)
    opt = sf.CollapsedEMOptimizer()
    assert opt.optimize(exp, sopt, 0.01, 10000)
    rec = dict(transcripts=len(names), classes=eq.n_classes, gibbs=a.gibbs, boot=a.boot)

    def sample(kind, n, writer):
        torch.cuda.synchronize()
        t = time.perf_counter()
        if kind == "gibbs":
            g = sf.CollapsedGibbsSampler()
            assert g.sample(exp, sopt, writer, n, seed=3)
            mat = g.last_samples
        else:
            so = sf.SailfishOpts(numBootstraps=n)
            assert opt.gatherBootstraps(exp, so, writer, 0.01, 10000, seed=3)
            mat = opt.last_bootstraps
        torch.cuda.synchronize()
        return mat, time.perf_counter() - t

    if a.encode_only:
        mat, _ = sample("gibbs", a.gibbs, None)
        writes = []
        for _ in range(3):
            w = sf.writer.BootstrapWriter(os.path.join(a.out, "enc"), sopt); w.write_device(mat); w.close()
            writes.append(w.last_result)
        print(json.dumps(dict(bytes=mat.numel() * mat.element_size(), writes=writes)))
        return
    for kind, n, n_host in (("gibbs", a.gibbs, a.host_gibbs), ("boot", a.boot, a.host_boot)):
        sample(kind, min(n, 8), None)                                   # warm-up
        mat, t_draw = sample(kind, n, None)
        rec[kind + "_draw_s"] = t_draw
        write_both(a.out, sopt, mat, min(n_host, n), rec, kind)
        # the sample-writing phase as _quantify_tail times it: sampler + writer, new path
        t = time.perf_counter()
        mat2, _ = sample(kind, n, None)
        w = sf.writer.BootstrapWriter(os.path.join(a.out, f"{kind}_tail"), sopt); w.write_device(mat2); w.close()
        rec[kind + "_samples_s_device_path"] = time.perf_counter() - t
        # old path: the writer as the per-sample callback, on n_host samples
        w = sf.writer.BootstrapWriter(os.path.join(a.out, f"{kind}_tail_host"), sopt)
        _, t_old = sample(kind, min(n_host, n), w)
        w.close()
        rec[kind + "_samples_s_host_path"] = dict(samples=min(n_host, n), wall_s=t_old)
        del mat, mat2
    print(json.dumps(rec))
    with open(os.path.join(a.out, "gzwrite_probe.json"), "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
