"""quant.sf writer at cfg3 size (sfgpu_quant_write_text; sailfish_amd/quantfile.py): 200 000 rows with cfg3-like columns (30 % of
the counts exactly zero, the rest over eleven decades; TPM from them) written with quantfile.write_file, and with the per-row
Python loop writer.write_abundances ran before (four D2H column copies, then one "%g" triple per row), in one process on the same
device arrays.  Both write into the same directory (page cache); the files are compared.

Clocks: write_file_s and loop_s are host wall time (time.perf_counter) around the whole call, after torch.cuda.synchronize();
format_ms / d2h_ms are device events and sink_ms the host clock inside the sink, from the library's result.  The first run of each
leg warms code objects, pools and the page cache and is dropped; the rest are all reported, with their median.

    python tools/quantfile_probe.py [--out DIR] [--rows 200000] [--repeats 7] [--write-only]
Prints one JSON line and writes DIR/quantwrite_probe.json.  --write-only: three device writes, nothing else (for rocprofv3
--kernel-trace --stats)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sailfish_amd import quantfile, synth  # noqa: E402
from sailfish_amd.writer import fmt_g  # noqa: E402


def cfg3_columns(M, dev):
    rng = np.random.default_rng(11)
    ref = synth.transcript_lengths(M).numpy().view(np.uint32)
    eff = np.maximum(ref.astype(np.float64) - rng.random(M) * 180.0, 1.0)
    cnt = np.where(rng.random(M) < 0.3, 0.0, 10.0 ** rng.uniform(-6, 5, M))
    rate = cnt / eff
    tpm = rate / rate.sum() * 1e6
    names = [f"ENST{i:011d}" for i in range(M)]
    up = lambda a: torch.from_numpy(a.copy()).to(dev)  # noqa: E731
    return names, up(ref.view(np.int32)), up(eff), up(tpm), up(cnt)


def loop_write(path, names, d_ref, d_eff, d_tpm, d_cnt):
    """writer.write_abundances as it was before the device writer"""
    t = d_tpm.cpu().numpy(); length = d_eff.cpu().numpy()
    cnt = d_cnt.cpu().numpy()
    ref = d_ref.cpu().numpy().view(np.uint32)
    with open(path, "w") as f:
        f.write("Name\tLength\tEffectiveLength\tTPM\tNumReads\n")
        for i, name in enumerate(names):
            f.write(f"{name}\t{int(ref[i])}\t{fmt_g(length[i])}\t{fmt_g(t[i])}\t{fmt_g(cnt[i])}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="quantfile_probe_out")
    ap.add_argument("--rows", type=int, default=200_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--write-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    names, d_ref, d_eff, d_tpm, d_cnt = cfg3_columns(a.rows, dev)
    blob, off = quantfile.names_blob(names)
    d_names = (torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev))
    path = os.path.join(a.out, "quant.sf")
    if a.write_only:
        for _ in range(3):
            res = quantfile.write_file(path, d_names, d_ref, d_eff, d_tpm, d_cnt)
        print(json.dumps(res))
        return
    runs = []
    for _ in range(a.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = quantfile.write_file(path, d_names, d_ref, d_eff, d_tpm, d_cnt)
        runs.append(dict(res, write_file_s=time.perf_counter() - t0))
    text = open(path, "rb").read()
    loops = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop_write(path + ".loop", names, d_ref, d_eff, d_tpm, d_cnt)
        loops.append(time.perf_counter() - t0)
    assert open(path + ".loop", "rb").read() == text
    os.remove(path + ".loop")
    rec = dict(rows=a.rows, file_bytes=len(text), device=torch.cuda.get_device_name(0), writer=runs[1:], loop_s=loops[1:],
               write_file_s_median=statistics.median(r["write_file_s"] for r in runs[1:]),
               format_ms_median=statistics.median(r["format_ms"] for r in runs[1:]),
               d2h_ms_median=statistics.median(r["d2h_ms"] for r in runs[1:]),
               sink_ms_median=statistics.median(r["sink_ms"] for r in runs[1:]),
               loop_s_median=statistics.median(loops[1:]),
               text_size=quantfile.text_size(d_names, d_ref, d_eff, d_tpm, d_cnt))
    print(json.dumps(rec))
    with open(os.path.join(a.out, "quantwrite_probe.json"), "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
