"""dev probe: what mate rescue (sfgpu_hits_rescue_mates) costs and what it finds -> profiles/rescue_probe.json

On the index of tools/verify_probe.py (80 000 transcripts; RESCUE_M) and RESCUE_R pairs (10 M) of 2 x 50 bases from fragments of 250,
with 2 % and with 4 % substitutions: the device's result is first asserted equal to hits.rescue_mates_host on a slice; then medians of 5
after a warm-up of the pass (min_identity 0.9, window 1000), of sfgpu_map_reads and sfgpu_hits_verify on the same batch, and of a plain
device-to-device copy of the bytes the pass has to touch (24 bytes a record in and out, the offsets, and per job the mate and the
transcript bases under its window).  The pass is timed once more with window = 1, where no job has a candidate: what remains is the
compaction and the output, and the difference to the full pass is the search."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sailfish_amd as sf
from sailfish_amd import _lib, hits as H, synth

dev = torch.device("cuda:0")
ACGT = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()                                     # warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(); out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out), out


class Transcripts:
    """the transcripts as rescue_mates_host wants them (bytes by index), cut from the host copy on demand"""
    def __init__(self, seq, off):
        self.seq, self.off = seq.cpu().numpy(), off.cpu().numpy()

    def __len__(self):
        return len(self.off) - 1

    def __getitem__(self, t):
        return self.seq[self.off[t]:self.off[t + 1]].tobytes()


def cost(M, R, L=50, window=1000):
    g = torch.Generator(device=dev); g.manual_seed(1)
    ref_len = synth.transcript_lengths(M, device=dev).long()
    off = torch.zeros(M + 1, dtype=torch.int64, device=dev); torch.cumsum(ref_len, 0, out=off[1:])
    N = int(off[-1])
    seq = ACGT[torch.randint(0, 4, (N,), generator=g, device=dev)]
    t = torch.randint(0, M, (R,), generator=g, device=dev)
    p = (torch.rand(R, generator=g, device=dev, dtype=torch.float64) * (ref_len[t] - 250).clamp_min(0).double()).long()
    start = off[t] + p
    comp = torch.zeros(256, dtype=torch.uint8, device=dev); comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    c1 = torch.empty((R, L), dtype=torch.uint8, device=dev); c2 = torch.empty((R, L), dtype=torch.uint8, device=dev)
    idxs = torch.arange(L, device=dev)
    for a in range(0, R, 1 << 20):                                     # (in pieces: the gather indices are 8 bytes a base)
        s = start[a:a + (1 << 20), None]
        c1[a:a + (1 << 20)] = seq[(s + idxs[None, :]).clamp_max(N - 1)]
        c2[a:a + (1 << 20)] = comp[seq[(s + 249 - idxs[None, :]).clamp_max(N - 1)].long()]
    roff = torch.arange(R + 1, device=dev, dtype=torch.int64) * L
    index = sf.mapper.QuasiIndex((seq, off), device=dev)
    Lb = _lib.lib()
    tx = Transcripts(seq, off)
    rows = []
    for rate in (0.02, 0.04):
        m1, m2 = c1.clone(), c2.clone()
        for m in (m1, m2):
            hit = torch.rand(m.shape, generator=g, device=dev) < rate
            m[hit] = ACGT[torch.randint(0, 4, (int(hit.sum()),), generator=g, device=dev)]
        r1, r2 = (m1.reshape(-1), roff), (m2.reshape(-1), roff)
        hits, hoff = index.map_reads(r1, r2)
        n = hits.numel() // 24
        # the device against the statement on a slice
        k = min(R, 20000)
        cut = int(hoff[k].item())
        sl1, sl2 = ([bytes(x) for x in m[:k].cpu().numpy()] for m in (m1, m2))
        dh, do, dm, dst = H.rescue_mates(index, hits[: cut * 24], hoff[: k + 1], sl1, sl2, min_identity=0.9, window=window)
        wh, wo, wm, wst = H.rescue_mates_host(tx, hits[: cut * 24].cpu().numpy().view(H.HIT_DTYPE), hoff[: k + 1].cpu().numpy(), sl1, sl2, 900, window)
        assert np.array_equal(dh.cpu().numpy().view(H.HIT_DTYPE), wh) and np.array_equal(do.cpu().numpy().view(np.uint32), wo)
        assert np.array_equal(dm.cpu().numpy().view(np.uint16), wm) and dst == wst, (dst, wst)
        out_hits, out_off, mism = torch.empty_like(hits), torch.empty_like(hoff), torch.empty(max(n, 1) * 2, dtype=torch.uint8, device=dev)
        scores, scratch = torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=dev), torch.empty_like(hits)
        o = _lib.RescueOpts(900, window); st = _lib.RescueStats(); vo = _lib.VerifyOpts(900, 0); vst = _lib.VerifyStats(); n_out = C.c_uint64(0); nh = C.c_uint64(0)
        args = (index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(hits), _lib.ptr(hoff))

        def rescue():
            _lib.check(Lb.sfgpu_hits_rescue_mates(*args, C.byref(o), _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(mism), C.byref(n_out), C.byref(st), None))

        def verify():
            _lib.check(Lb.sfgpu_hits_verify(*args, C.byref(vo), _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores), C.byref(n_out), C.byref(vst), None))

        def remap():
            _lib.check(Lb.sfgpu_map_reads(index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(scratch), n, _lib.ptr(out_off),
                                          C.byref(nh), None))
        r_ms, r_all = timed(rescue)
        stats, records_out = st.as_dict(), n_out.value
        o.window = 1                                                   # no job has a candidate: compaction and output alone
        e_ms, e_all = timed(rescue)
        o.window = window
        v_ms, v_all = timed(verify)
        m_ms, m_all = timed(remap)
        moved = 24 * n + 24 * records_out + 8 * (R + 1) + stats["records_orphan"] * L + stats["candidates"] + stats["jobs_with_candidates"] * L
        src = torch.empty(moved, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        c_ms, c_all = timed(lambda: dst.copy_(src))
        jobs = max(stats["records_orphan"], 1)
        rows.append(dict(substitution_rate=rate, pairs=R, read_len=L, window=window, records=n, stats=stats, eligible_read_share=stats["reads_eligible"] / R,
                         candidates_per_job=stats["candidates"] / jobs, rescued_read_share_of_eligible=stats["reads_rescued"] / max(stats["reads_eligible"], 1),
                         rescue_ms=r_ms, rescue_ms_runs=r_all, compaction_and_output_ms=e_ms, compaction_and_output_ms_runs=e_all, search_ms=r_ms - e_ms,
                         search_share=(r_ms - e_ms) / r_ms, base_comparisons_per_ns=stats["candidates"] * L / max(r_ms - e_ms, 1e-9) / 1e6,
                         map_reads_ms=m_ms, map_reads_ms_runs=m_all, verify_ms=v_ms, verify_ms_runs=v_all, bytes_touched=moved, d2d_copy_ms=c_ms,
                         d2d_copy_ms_runs=c_all, rescue_over_map=r_ms / m_ms, rescue_over_verify=r_ms / v_ms, rescue_over_copy=r_ms / c_ms))
        print(json.dumps(rows[-1]), flush=True)
        del src, dst, m1, m2, out_hits, scores, scratch
    index.close()
    return rows


if __name__ == "__main__":
    M, R = int(os.environ.get("RESCUE_M", 80000)), int(os.environ.get("RESCUE_R", 10_000_000))
    out = dict(device=torch.cuda.get_device_name(0), transcripts=M, cost=cost(M, R))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rescue_probe.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)
