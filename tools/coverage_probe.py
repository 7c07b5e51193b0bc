"""dev probe: what the coverage pass (sfgpu_cov_*) costs -> profiles/coverage_probe.json

On the batch of tools/verify_probe.py (80 000 transcripts, VERIFY_R pairs of 2 x 100 bases from fragments of 250), error-free and with
2 % substitutions, posteriors under weights 10^U(-3, 3).  The device result on a slice is first asserted equal to hits.coverage_host.
Then medians of 5 after a warm-up of
 - the add pass (sfgpu_cov_add, posterior weights; and uniform) beside sfgpu_hits_posteriors and sfgpu_hits_verify on the same records
   and beside a plain device-to-device copy of the bytes it reads (24 bytes a record and its 8-byte posterior);
 - finish (scan, runs, summary), each time on a fresh handle that holds the batch once, beside a plain device-to-device copy of the
   slot array;
 - the writer, plain and BGZF, into memory: the format kernels' ms, the staged copies' ms and the wall ms, beside a plain pinned
   device-to-host copy of as many bytes;
and the runs and the file's size."""
import argparse
import ctypes as C
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
from sailfish_amd import _lib, coverage as cov, hits as H, synth

med = statistics.median


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
    Lb = _lib.lib()
    rows = []
    for rate in (0.0, 0.02):
        if rate:
            for m in (m1, m2):
                hit = torch.rand(m.shape, generator=g, device=dev) < rate
                m[hit] = ACGT[torch.randint(0, 4, (int(hit.sum()),), generator=g, device=dev)]
        r1, r2 = (m1.reshape(-1), roff), (m2.reshape(-1), roff)
        hits, hoff = index.map_reads(r1, r2)
        n = hits.numel() // 24
        p = H.posteriors(hits, hoff, w)[0]
        # a slice against the statement
        k = min(R, 5000)
        cut = int(hoff[k].item())
        with cov.CoverageDevice(len32, dev) as c:
            c.add(hits[: cut * 24], hoff[: k + 1], posteriors=p[:cut])
            res = c.finish()
            got = [x.cpu().numpy() for x in c.runs()] + [x.cpu().numpy() for x in c.summary()]
            stats = dict(c.stats)
        wr, ws, wst = H.coverage_host(len32.cpu().numpy().view(np.uint32), [(hits[: cut * 24].cpu().numpy().view(H.HIT_DTYPE), hoff[: k + 1].cpu().numpy().view(np.uint32),
                                                                            p[:cut].cpu().numpy(), None)])
        assert all(np.array_equal(a.view(b.dtype), b) for a, b in zip(got[:4], wr)) and all(np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(got[4:], ws))
        assert stats == {key: wst[key] for key in stats} and res["residue"] == 0 and res["runs"] == wst["runs"]
        # the add pass
        c = cov.CoverageDevice(len32, dev)
        st = _lib.CovStats()

        def add(pp):
            _lib.check(Lb.sfgpu_cov_add(c._h, _lib.ptr(hits), _lib.ptr(hoff), R, _lib.ptr(pp) if pp is not None else None, None, None, None, C.byref(st), None))
        a_ms, a_all = VP.timed(lambda: add(p), reps)
        u_ms, u_all = VP.timed(lambda: add(None), reps)
        c.close()
        po, rec, f32 = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        pst = _lib.PosteriorStats()
        p_ms, p_all = VP.timed(lambda: _lib.check(Lb.sfgpu_hits_posteriors(_lib.ptr(hits), _lib.ptr(hoff), R, _lib.ptr(w), M, _lib.ptr(po), _lib.ptr(rec), _lib.ptr(f32),
                                                                          C.byref(pst), None)), reps)
        out_hits, out_off, scores = torch.empty_like(hits), torch.empty_like(hoff), torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=dev)
        o = _lib.VerifyOpts(900, 0); vst = _lib.VerifyStats(); n_out = C.c_uint64(0)
        v_ms, v_all = VP.timed(lambda: _lib.check(Lb.sfgpu_hits_verify(index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(hits),
                                                                      _lib.ptr(hoff), C.byref(o), _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores), C.byref(n_out),
                                                                      C.byref(vst), None)), reps)
        del out_hits, scores, po, rec, f32
        src = torch.empty(32 * n, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        rc_ms, rc_all = VP.timed(lambda: dst.copy_(src), reps)
        del src, dst
        # finish, on a fresh handle each time
        f_all, last = [], None
        for i in range(reps + 1):
            c = cov.CoverageDevice(len32, dev)
            c.add(hits, hoff, posteriors=p)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            res = c.finish()
            torch.cuda.synchronize()
            if i:
                f_all.append(1e3 * (time.perf_counter() - t0))
            if i < reps:
                c.close()
            else:
                last = c
        slots = N + M
        src = torch.empty(slots, dtype=torch.int64, device=dev); dst = torch.empty_like(src)
        sc_ms, sc_all = VP.timed(lambda: dst.copy_(src), reps)
        del src, dst
        # the writer
        legs = {}
        for leg, kw in (("text", {}), ("bgzf", dict(compress=True))):
            wall, fmt, d2h, size, n_bytes = [], [], [], 0, 0
            for i in range(reps + 1):
                f = io.BytesIO()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                wres = last.write(f, d_names, **kw)
                torch.cuda.synchronize()
                if i:
                    wall.append(1e3 * (time.perf_counter() - t0)); fmt.append(wres["format_ms"]); d2h.append(wres["d2h_ms"])
                size, n_bytes = len(f.getvalue()), int(wres["n_bytes"])
            legs[leg] = dict(wall_ms=med(wall), format_ms=med(fmt), d2h_ms=med(d2h), wall_ms_runs=wall, format_ms_runs=fmt, file_bytes=size, text_bytes=n_bytes)
        src = torch.empty(legs["text"]["text_bytes"], dtype=torch.uint8, device=dev); pin = torch.empty(src.numel(), dtype=torch.uint8, pin_memory=True)
        h_ms, h_all = VP.timed(lambda: pin.copy_(src), reps)
        del src, pin
        last.close()
        rows.append(dict(substitution_rate=rate, pairs=R, transcripts=M, records=n, slots=slots, lines=int(st.lines) // (2 * (reps + 1)), result=res,
                         add_ms=a_ms, add_ms_runs=a_all, add_uniform_ms=u_ms, add_uniform_ms_runs=u_all, posteriors_ms=p_ms, posteriors_ms_runs=p_all,
                         verify_ms=v_ms, verify_ms_runs=v_all, bytes_read=32 * n, d2d_copy_ms=rc_ms, d2d_copy_ms_runs=rc_all, add_over_verify=a_ms / v_ms,
                         add_over_copy=a_ms / rc_ms, finish_ms=med(f_all), finish_ms_runs=f_all, slot_copy_ms=sc_ms, slot_copy_ms_runs=sc_all,
                         finish_over_slot_copy=med(f_all) / sc_ms, writer=legs, pinned_d2h_ms=h_ms, pinned_d2h_ms_runs=h_all))
        print(json.dumps(rows[-1]), flush=True)
    index.close()
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?", default=os.path.join(ROOT, "profiles", "coverage_probe.json"))
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    M, R = int(os.environ.get("VERIFY_M", 80000)), int(os.environ.get("VERIFY_R", 10_000_000))
    doc = dict(device=torch.cuda.get_device_name(0), repeats=a.repeats, rows=probe(M, R, a.repeats))
    with open(a.path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.path)
