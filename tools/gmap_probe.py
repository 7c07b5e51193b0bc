"""The --geneMap reader at annotation size (sfgpu_gmap_*; sailfish_amd/genes.py DeviceGeneMap): a GENCODE-shaped synthetic GTF --
gene / transcript / exon / CDS lines with ten attributes, about 420 000 lines, 29 965 transcripts in 6 000 genes -- through
  host      genes.TranscriptGeneMap.from_gtf (the per-line Python loop),
  device    genes.DeviceGeneMap.from_path, split into reading the file (read_s, host clock inside readinto), the staged copies
            (ms_copy), the parse kernels (ms_kernels) and the sort / dedupe / numbering of finish (ms_finish), device events from
            the library's results,
  lookup    TranscriptGeneMap.gene_ids_of (numpy searchsorted over unicode arrays) against sfgpu_gmap_lookup for 200 000 names,
  copy      a plain pinned host-to-device copy of the same bytes, the yardstick for the parse kernels,
in one process.  The device map is compared with from_gtf's (exact lists) BEFORE any time is reported.  The first run of each leg
warms code objects, pools and the page cache and is dropped; medians of the rest are reported.

    python tools/gmap_probe.py [--out DIR] [--genes 6000] [--repeats 5] [--names 200000]
Prints one JSON line and writes DIR/gmap_probe.json."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sailfish_amd import genes, quantfile  # noqa: E402


def write_gtf(path, n_genes, seed=7):
    """-> (lines, transcripts)"""
    rng = np.random.default_rng(seed)
    n_lines = n_tx = 0
    with open(path, "w") as f:
        f.write("##description: synthetic annotation in the shape of a GENCODE release\n##provider: gmap_probe\n")
        n_lines += 2
        for g in range(n_genes):
            chrom, strand = f"chr{1 + g % 22}", "+-"[g % 2]
            gid, gname = f"ENSG{g:011d}.{1 + g % 17}", f"GENE{g}"
            gtype = ("protein_coding", "lncRNA", "processed_pseudogene")[g % 3]
            start = 10_000 + 37 * g
            gattr = f'gene_id "{gid}"; gene_type "{gtype}"; gene_name "{gname}"; level 2; hgnc_id "HGNC:{g}"; havana_gene "OTTHUMG{g:011d}.2";'
            f.write(f"{chrom}\tHAVANA\tgene\t{start}\t{start + 90_000}\t.\t{strand}\t.\t{gattr}\n")
            n_lines += 1
            n_t = 4 if g >= n_genes - 35 else 5                           # 29 965 transcripts at 6 000 genes
            for t in range(n_t):
                tid = f"ENST{n_tx:011d}.{1 + n_tx % 9}"
                n_tx += 1
                tattr = (f'gene_id "{gid}"; transcript_id "{tid}"; gene_type "{gtype}"; gene_name "{gname}"; transcript_type "{gtype}"; '
                         f'transcript_name "{gname}-2{t:02d}"; level 2; transcript_support_level "{1 + t % 5}"; tag "basic"; '
                         f'havana_transcript "OTTHUMT{n_tx:011d}.1";')
                f.write(f"{chrom}\tHAVANA\ttranscript\t{start}\t{start + 80_000}\t.\t{strand}\t.\t{tattr}\n")
                n_lines += 1
                for e in range(int(rng.integers(3, 11))):
                    eattr = (f'gene_id "{gid}"; transcript_id "{tid}"; gene_type "{gtype}"; gene_name "{gname}"; transcript_type "{gtype}"; '
                             f'transcript_name "{gname}-2{t:02d}"; exon_number {e + 1}; exon_id "ENSE{n_lines:011d}.1"; level 2; tag "basic";')
                    for feature in ("exon", "CDS"):
                        f.write(f"{chrom}\tHAVANA\t{feature}\t{start + 900 * e}\t{start + 900 * e + 300}\t.\t{strand}\t{'.' if feature == 'exon' else e % 3}\t{eattr}\n")
                        n_lines += 1
    return n_lines, n_tx


def med(rows, k):
    return statistics.median(r[k] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="gmap_probe_out")
    ap.add_argument("--genes", type=int, default=6000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--names", type=int, default=200_000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, "probe.gtf")
    n_lines, n_tx = write_gtf(path, a.genes)
    n_bytes = os.path.getsize(path)

    host_map = genes.TranscriptGeneMap.from_gtf(path)
    with genes.DeviceGeneMap.from_path(path, device=dev) as d:
        got = d.to_host()
        assert d.stats["reader"] == "device", d.stats
    assert got.transcript_names == host_map.transcript_names and got.t2g == host_map.t2g and got.gene_names == host_map.gene_names, \
        "the device map differs from from_gtf's"

    host, device = [], []
    for _ in range(a.repeats + 1):
        t0 = time.perf_counter()
        genes.TranscriptGeneMap.from_gtf(path)
        host.append(dict(from_gtf_s=time.perf_counter() - t0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d = genes.DeviceGeneMap.from_path(path, device=dev)
        torch.cuda.synchronize()
        device.append(dict(from_path_s=time.perf_counter() - t0, **{k: d.stats[k] for k in
                                                                   ("read_s", "ms_copy", "ms_kernels", "ms_finish", "calls", "n_lines", "n_records", "sort_rounds")}))
        d.close()

    # the name join: 200 000 names drawn from the map's (with strangers that land between two names)
    rng = np.random.default_rng(3)
    pick = rng.integers(0, len(host_map.transcript_names) - 1, a.names)
    names = [host_map.transcript_names[i] if k else host_map.transcript_names[i][:-1] for i, k in zip(pick.tolist(), (rng.random(a.names) < 0.9).tolist())]
    b, o = quantfile.names_blob(names)
    pair = (torch.from_numpy(np.frombuffer(b, np.uint8).copy()).to(dev), torch.from_numpy(o.view(np.int64).copy()).to(dev))
    lookup = []
    with genes.DeviceGeneMap.from_path(path, device=dev) as d:
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter()
            want, _ = host_map.gene_ids_of(names)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ids, n_past = d.lookup(pair)
            torch.cuda.synchronize()
            lookup.append(dict(gene_ids_of_s=t1 - t0, gmap_lookup_s=time.perf_counter() - t2))
        assert n_past == 0 and np.array_equal(ids.cpu().numpy().view(np.uint32), want)

    # the yardstick: the same bytes through one pinned buffer
    raw = torch.from_numpy(np.fromfile(path, np.uint8)).pin_memory()
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
    rec = dict(lines=n_lines, transcripts=n_tx, genes=len(host_map.gene_names), file_bytes=n_bytes, names=a.names,
               device=torch.cuda.get_device_name(0), gcn_arch=getattr(props, "gcnArchName", None), compute_units=props.multi_processor_count,
               host_runs=host[1:], device_runs=device[1:], lookup_runs=lookup[1:], copy_runs=copy[1:],
               from_gtf_s_median=med(host[1:], "from_gtf_s"), from_path_s_median=med(device[1:], "from_path_s"),
               read_s_median=med(device[1:], "read_s"), ms_copy_median=med(device[1:], "ms_copy"),
               ms_kernels_median=med(device[1:], "ms_kernels"), ms_finish_median=med(device[1:], "ms_finish"),
               gene_ids_of_s_median=med(lookup[1:], "gene_ids_of_s"), gmap_lookup_s_median=med(lookup[1:], "gmap_lookup_s"),
               pinned_copy_ms_median=med(copy[1:], "pinned_copy_ms"))
    rec["parse_kernels_over_copy"] = rec["ms_kernels_median"] / rec["pinned_copy_ms_median"]
    os.remove(path)
    print(json.dumps(rec))
    with open(os.path.join(a.out, "gmap_probe.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
