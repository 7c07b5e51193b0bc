"""Gene-level estimates at cfg3 size (sfgpu_genes_aggregate / sfgpu_genes_write_text; sailfish_amd/genes.py): 200 000 rows with
cfg3-like columns in about 24 000 genes (1 .. 16 transcripts each, transcripts of a gene scattered over the file), through
  host    quantfile.write_file, then genes.aggregate_estimates_to_gene_level on the file just written (the per-row loop that
          `quantify(..., gene_map=...)` ran before: re-open, split, float(), bisect, dict, "%g"), and
  device  genes.aggregate_columns on the same device arrays (vectorised name lookup on the host, fold and rows on the device),
in one process.  The two quant.genes.sf files are compared byte for byte BEFORE any time is reported.  A last leg folds ONE gene
that holds every row (--one-gene-rows, 1 000 000): the serial worst case of the one-lane-per-gene fold, sfgpu_genes_aggregate alone.

Clocks: host_s / host_write_s / host_aggregate_s and device_s are host wall time (time.perf_counter) around the calls, after
torch.cuda.synchronize(); aggregate_ms / format_ms / d2h_ms are device events and sink_ms the host clock inside the sink, from
the library's results.  The first run of each leg warms code objects, pools and the page cache and is dropped; the rest are all
reported, with their median.

    python tools/genes_probe.py [--out DIR] [--rows 200000] [--genes 24000] [--repeats 5] [--one-gene-rows 1000000]
Prints one JSON line and writes DIR/genes_probe.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sailfish_amd import genes, quantfile, synth  # noqa: E402


def cfg3_columns(M, n_genes, dev):
    rng = np.random.default_rng(11)
    ref = synth.transcript_lengths(M).numpy().view(np.uint32)
    eff = np.maximum(ref.astype(np.float64) - rng.random(M) * 180.0, 1.0)
    cnt = np.where(rng.random(M) < 0.3, 0.0, 10.0 ** rng.uniform(-6, 5, M))
    rate = cnt / eff
    tpm = rate / rate.sum() * 1e6
    names = [f"ENST{i:011d}" for i in range(M)]
    gene = rng.integers(0, n_genes, M)
    tgm = genes.TranscriptGeneMap([(n, f"ENSG{g:011d}") for n, g in zip(names, gene)])
    up = lambda a: torch.from_numpy(a.copy()).to(dev)  # noqa: E731
    return tgm, names, up(ref.view(np.int32)), up(eff), up(tpm), up(cnt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="genes_probe_out")
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--genes", type=int, default=24_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--one-gene-rows", type=int, default=1_000_000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    tgm, names, d_ref, d_eff, d_tpm, d_cnt = cfg3_columns(a.rows, a.genes, dev)
    quant = os.path.join(a.out, "quant.sf")
    dev_path = os.path.join(a.out, "device.genes.sf")
    host, device = [], []
    for _ in range(a.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        quantfile.write_file(quant, names, d_ref, d_eff, d_tpm, d_cnt)
        t1 = time.perf_counter()
        host_path = genes.aggregate_estimates_to_gene_level(tgm, quant)
        t2 = time.perf_counter()
        host.append(dict(host_s=t2 - t0, host_write_s=t1 - t0, host_aggregate_s=t2 - t1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = genes.aggregate_columns(tgm, names, d_ref, d_eff, d_tpm, d_cnt, dev_path)
        device.append(dict(device_s=time.perf_counter() - t0, **res["aggregate"], **{k: res["write"][k] for k in
                                                                                   ("n_bytes", "n_chunks", "format_ms", "d2h_ms", "sink_ms")}))
    text = open(dev_path, "rb").read()
    assert text == open(host_path, "rb").read(), "the device file differs from the host function's"
    # one gene holding every row: one lane folds the whole chain
    one = []
    if a.one_gene_rows > 0:
        rng = np.random.default_rng(12)
        n1 = a.one_gene_rows
        up = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
        ids1 = torch.zeros(n1, dtype=torch.int32, device=dev)
        cols1 = (up(rng.integers(200, 100_000, n1).astype(np.int32)), up(rng.random(n1) * 1e4 + 1.0), up(rng.random(n1) * 5.0),
                 up(rng.random(n1) * 100.0))
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            *_, r1 = genes.aggregate_device(ids1, 1, *cols1)
            one.append(dict(r1, wall_s=time.perf_counter() - t0))
        assert one[-1]["n_genes"] == 1 and one[-1]["max_rows_per_gene"] == n1
    props = torch.cuda.get_device_properties(0)
    rec = dict(rows=a.rows, genes=device[-1]["n_genes"], file_bytes=len(text), device=torch.cuda.get_device_name(0),
               gcn_arch=getattr(props, "gcnArchName", None), compute_units=props.multi_processor_count, host=host[1:],
               one_gene=one[1:], one_gene_aggregate_ms_median=statistics.median(r["aggregate_ms"] for r in one[1:]) if one else None,
               device_runs=device[1:], host_s_median=statistics.median(r["host_s"] for r in host[1:]),
               host_aggregate_s_median=statistics.median(r["host_aggregate_s"] for r in host[1:]),
               device_s_median=statistics.median(r["device_s"] for r in device[1:]),
               aggregate_ms_median=statistics.median(r["aggregate_ms"] for r in device[1:]),
               format_ms_median=statistics.median(r["format_ms"] for r in device[1:]))
    print(json.dumps(rec))
    with open(os.path.join(a.out, "genes_probe.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
