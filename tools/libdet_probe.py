"""dev probe: what the library-format tally (sfgpu_hits_library_kinds) costs -> profiles/libdet_probe.json

On the batch of tools/verify_probe.py (80 000 transcripts, VERIFY_R pairs of 2 x 100 bases from fragments of 250, error-free, mapped
by the device mapper): the pass's result on a slice is first asserted equal to hits.library_kinds_host; then medians of 5 after a
warm-up of
 - the pass with votes on (a budget of 50 000, quant.quantify's default: the vote bytes, the scan and the second kernel run) and with
   votes off (a budget of 0: what every batch costs once the format is decided), both with an expected format;
 - sfgpu_filter_hits on the same records (IU, allow_orphans, no fragment-length sample): it stages the same records the same way and
   does strictly more -- it parks the kept ids, scans and compacts -- so it is the yardstick;
 - a plain device-to-device copy of the bytes the pass reads (24 a record, 4 a read)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sailfish_amd as sf
from sailfish_amd import _lib, hits as H, synth


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
    hits, hoff = index.map_reads((m1.reshape(-1), roff), (m2.reshape(-1), roff))
    index.close()
    del seq, m1, m2
    # the pass on a slice against the statement
    k = min(R, 5000)
    cut = int(hoff[k].item())
    kw = dict(paired_library=True, max_read_occs=200, remaining_votes=1000, expected="IU")
    got = H.library_kinds(hits[: cut * 24], hoff[: k + 1], **kw)
    want = H.library_kinds_host(hits[: cut * 24].cpu().numpy().view(H.HIT_DTYPE), hoff[: k + 1].cpu().numpy().view(np.uint32), **kw)
    assert got == want, (got, want)
    # the whole batch
    n = hits.numel() // 24
    Lb = _lib.lib()
    fmt = _lib.LibFmt(*H.LIBRARY_FORMATS["IU"], 0)
    o = _lib.LibdetOpts(200, 1, 0, 1, fmt)
    st = _lib.LibdetStats()

    def tally(budget):
        rem = C.c_int64(budget)
        _lib.check(Lb.sfgpu_hits_library_kinds(_lib.ptr(hits), _lib.ptr(hoff), R, C.byref(o), C.byref(rem), C.byref(st), None))
    ids, out_off = torch.empty(max(n, 1), dtype=torch.int32, device=dev), torch.empty(R + 1, dtype=torch.int32, device=dev)
    fo = _lib.FilterOpts(200, 1000, 1, 0, 0, 0, 0, fmt)
    fst, frem = _lib.FilterStats(), C.c_int64(0)

    def filt():
        _lib.check(Lb.sfgpu_filter_hits(_lib.ptr(hits), _lib.ptr(hoff), R, C.byref(fo), _lib.ptr(ids), _lib.ptr(out_off), None, C.byref(frem), C.byref(fst), None))
    on_ms, on_all = VP.timed(lambda: tally(50_000))
    off_ms, off_all = VP.timed(lambda: tally(0))
    f_ms, f_all = VP.timed(filt)
    on2_ms, on2_all = VP.timed(lambda: tally(50_000))               # once more behind the others: the spread between two takes
    read = 24 * n + 4 * (R + 1)
    src = torch.empty(read, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    c_ms, c_all = VP.timed(lambda: dst.copy_(src))
    one = _lib.LibdetStats()
    rem = C.c_int64(50_000)
    _lib.check(Lb.sfgpu_hits_library_kinds(_lib.ptr(hits), _lib.ptr(hoff), R, C.byref(o), C.byref(rem), C.byref(one), None))
    row = dict(pairs=R, transcripts=M, records=n, stats=one.as_dict(), decided=H.decide_library_format(one.as_dict(), True)[0],
               votes_on_ms=on_ms, votes_on_ms_runs=on_all, votes_on_again_ms=on2_ms, votes_on_again_ms_runs=on2_all, votes_off_ms=off_ms, votes_off_ms_runs=off_all,
               filter_ms=f_ms, filter_ms_runs=f_all, bytes_read=read, d2d_copy_ms=c_ms, d2d_copy_ms_runs=c_all,
               votes_off_over_filter=off_ms / f_ms, votes_on_over_filter=on_ms / f_ms, votes_off_over_copy=off_ms / c_ms,
               votes_off_ms_per_10M_pairs=off_ms * 1e7 / R)
    print(json.dumps(row), flush=True)
    return row


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?", default=os.path.join(ROOT, "profiles", "libdet_probe.json"))
    a = ap.parse_args()
    M, R = int(os.environ.get("VERIFY_M", 80000)), int(os.environ.get("VERIFY_R", 10_000_000))
    doc = dict(device=torch.cuda.get_device_name(0), repeats=5)
    doc["pass"] = pass_cost(M, R)
    with open(a.path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.path)
