"""dev probe: what hit verification (sfgpu_hits_verify) costs and what it drops -> profiles/verify_probe.json

1. cost, on the batch of tools/mapper_probe.py (80 000 transcripts, VERIFY_R pairs of 2 x 100 bases from fragments of 250), error-free
   and with 2 % substitutions: the device's result is first asserted equal to hits.verify_hits_host on a slice; then medians of 5 after
   a warm-up of sfgpu_hits_verify, of sfgpu_map_reads on the same batch, and of a plain device-to-device copy of the bytes the pass has
   to move (each job's mate bases, 24 + 24 bytes a surviving record, 8 bytes of score).
2. effect, on a spliced synthetic transcriptome (60 random exons of 40 - 220 bases, ten genes of four isoforms, 600 single-end reads of
   100 bases from either strand) at 0 / 1 / 2 / 4 % substitutions and min_identity 0.85 / 0.9 / 0.95: records dropped, TRUE records
   (source transcript, strand and position) dropped, reads left without a record.

--max-indel [K] (default 3) runs the gapped legs instead (sfgpu_hits_verify_gapped) -> profiles/verifyg_probe.json
3. cost, on the same batch, error-free, with 2 % substitutions, and with 2 % substitutions plus one insertion or deletion of 1 - 3 bases
   in 5 % of the mates: the gapped entry's result is first asserted equal to hits.verify_hits_gapped_host on a slice; then medians of 5
   after a warm-up of sfgpu_hits_verify_gapped, sfgpu_hits_verify, sfgpu_map_reads and the plain copy, all in this one process; and the
   share of jobs that ran the recurrence (ungapped count > 0, and not behind a failed first job) and that stopped on a band minimum
   above the edits that can still pass, both counted on the device from the entries' own scores at permille 0.
4. effect, on the spliced transcriptome, of reads with one indel of 1 - 3 bases (and 1 % substitutions) at min_identity 0.9: true
   records lost at max_indel 0 and K, and the false records K lets in.

--max-indel [K] --align runs the alignment leg instead (sfgpu_hits_align_gapped) -> profiles/aligng_probe.json
5. cost, on the same batch, error-free and with 2 % substitutions plus one indel of 1 - 3 bases in 5 % of the mates: the batch's
   records are reduced to the survivors of sfgpu_hits_verify_gapped at 0.9; the alignment of a slice is first asserted equal to
   hits.align_hits_host; then medians of 5 after a warm-up of sfgpu_hits_align_gapped on the survivors (with exactly the room it
   needs), of sfgpu_hits_verify_gapped on the batch they came from, and of a plain device-to-device copy of the bytes the pass moves
   (each job's mate bases, 24 bytes a record, 16 bytes a slot, the operations, and the scratch written and read once); the share of
   jobs traced, the slices' scratch peak and the whole batch's."""
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
    """the transcripts as verify_hits_host wants them (bytes by index), cut from the host copy on demand"""
    def __init__(self, seq, off):
        self.seq, self.off = seq.cpu().numpy(), off.cpu().numpy()

    def __len__(self):
        return len(self.off) - 1

    def __getitem__(self, t):
        return self.seq[self.off[t]:self.off[t + 1]].tobytes()


def cost(M, R, L=100):
    g = torch.Generator(device=dev); g.manual_seed(1)
    ref_len = synth.transcript_lengths(M, device=dev).long()
    off = torch.zeros(M + 1, dtype=torch.int64, device=dev); torch.cumsum(ref_len, 0, out=off[1:])
    N = int(off[-1])
    seq = ACGT[torch.randint(0, 4, (N,), generator=g, device=dev)]
    t = torch.randint(0, M, (R,), generator=g, device=dev)
    p = (torch.rand(R, generator=g, device=dev, dtype=torch.float64) * (ref_len[t] - 250).clamp_min(0).double()).long()
    start = off[t] + p
    comp = torch.zeros(256, dtype=torch.uint8, device=dev); comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    m1 = torch.empty((R, L), dtype=torch.uint8, device=dev); m2 = torch.empty((R, L), dtype=torch.uint8, device=dev)
    idxs = torch.arange(L, device=dev)
    for a in range(0, R, 1 << 20):                                     # (in pieces: the gather indices are 8 bytes a base)
        s = start[a:a + (1 << 20), None]
        m1[a:a + (1 << 20)] = seq[(s + idxs[None, :]).clamp_max(N - 1)]
        m2[a:a + (1 << 20)] = comp[seq[(s + 249 - idxs[None, :]).clamp_max(N - 1)].long()]
    roff = torch.arange(R + 1, device=dev, dtype=torch.int64) * L
    index = sf.mapper.QuasiIndex((seq, off), device=dev)
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
        # the device against the statement on a slice
        k = min(R, 1500)
        cut = int(hoff[k].item())
        sl1, sl2 = ([bytes(x) for x in m[:k].cpu().numpy()] for m in (m1, m2))
        tx = Transcripts(seq, off)
        for kb in (False, True):
            dh, do, ds, dst = H.verify_hits(index, hits[: cut * 24], hoff[: k + 1], sl1, sl2, min_identity=0.9, keep_best=kb)
            wh, wo, ws, wst = H.verify_hits_host(tx, hits[: cut * 24].cpu().numpy().view(H.HIT_DTYPE), hoff[: k + 1].cpu().numpy(), sl1, sl2, 900, kb)
            assert np.array_equal(dh.cpu().numpy().view(H.HIT_DTYPE), wh) and np.array_equal(do.cpu().numpy().view(np.uint32), wo)
            assert np.array_equal(ds.cpu().numpy().view(H.SCORE_DTYPE), ws) and dst == wst, (dst, wst)
        out_hits, out_off, scores = torch.empty_like(hits), torch.empty_like(hoff), torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=dev)
        o = _lib.VerifyOpts(900, 0); st = _lib.VerifyStats(); n_out = C.c_uint64(0); nh = C.c_uint64(0)
        scratch = torch.empty_like(hits)

        def verify():
            _lib.check(Lb.sfgpu_hits_verify(index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(hits), _lib.ptr(hoff),
                                            C.byref(o), _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores), C.byref(n_out), C.byref(st), None))

        def remap():
            _lib.check(Lb.sfgpu_map_reads(index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(scratch), n, _lib.ptr(out_off),
                                          C.byref(nh), None))
        v_ms, v_all = timed(verify)
        m_ms, m_all = timed(remap)
        status = hits.view(-1, 24)[:, 22]
        jobs = int(n + (status == 3).sum().item())
        moved = jobs * L + 56 * n_out.value
        src = torch.empty(moved, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        c_ms, c_all = timed(lambda: dst.copy_(src))
        rows.append(dict(substitution_rate=rate, pairs=R, records=n, jobs=jobs, stats=st.as_dict(), verify_ms=v_ms, verify_ms_runs=v_all, map_reads_ms=m_ms,
                         map_reads_ms_runs=m_all, bytes_moved=moved, d2d_copy_ms=c_ms, d2d_copy_ms_runs=c_all, verify_over_map=v_ms / m_ms,
                         verify_over_copy=v_ms / c_ms, verify_ms_per_10M_pairs=v_ms * 1e7 / R, map_reads_ms_per_10M_pairs=m_ms * 1e7 / R))
        print(json.dumps(rows[-1]), flush=True)
        del src, dst
    index.close()
    return rows


def make_mates(seq, N, start, L, comp, g, indel_rate):
    """mates of L bases from fragments of 250 at `start`; a share indel_rate of the mates carries one indel of 1 - 3 bases at a uniform
    position: a deletion skips transcript bases, an insertion puts random bases in"""
    R = start.numel()
    m1 = torch.empty((R, L), dtype=torch.uint8, device=dev); m2 = torch.empty((R, L), dtype=torch.uint8, device=dev)
    idxs = torch.arange(L, device=dev)
    for a in range(0, R, 1 << 20):                                     # (in pieces: the gather indices are 8 bytes a base)
        s = start[a:a + (1 << 20), None]
        n = s.shape[0]
        for m, sign, base in ((m1, 1, 0), (m2, -1, 249)):
            j = idxs[None, :].expand(n, L)
            if indel_rate:
                has = torch.rand((n, 1), generator=g, device=dev) < indel_rate
                size = torch.randint(1, 4, (n, 1), generator=g, device=dev)
                at = torch.randint(1, L - 4, (n, 1), generator=g, device=dev)
                dele = torch.rand((n, 1), generator=g, device=dev) < 0.5
                shift = torch.where(dele, size * (j >= at), -size * (j >= at + size))        # transcript bases skipped / read bases that take none
                j = torch.where(has, j + shift, j)
            v = seq[(s + base + sign * j).clamp(0, N - 1)]
            if sign < 0:
                v = comp[v.long()]
            if indel_rate:
                put = has & ~dele & (idxs[None, :] >= at) & (idxs[None, :] < at + size)
                v = torch.where(put, ACGT[torch.randint(0, 4, (n, L), generator=g, device=dev)], v)
            m[a:a + n] = v
    return m1, m2


def cost_gapped(M, R, K, L=100):
    g = torch.Generator(device=dev); g.manual_seed(1)
    ref_len = synth.transcript_lengths(M, device=dev).long()
    off = torch.zeros(M + 1, dtype=torch.int64, device=dev); torch.cumsum(ref_len, 0, out=off[1:])
    N = int(off[-1])
    seq = ACGT[torch.randint(0, 4, (N,), generator=g, device=dev)]
    t = torch.randint(0, M, (R,), generator=g, device=dev)
    p = (torch.rand(R, generator=g, device=dev, dtype=torch.float64) * (ref_len[t] - 250).clamp_min(0).double()).long()
    start = off[t] + p
    comp = torch.zeros(256, dtype=torch.uint8, device=dev); comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    roff = torch.arange(R + 1, device=dev, dtype=torch.int64) * L
    index = sf.mapper.QuasiIndex((seq, off), device=dev)
    Lb = _lib.lib()
    rows = []
    for rate, indel_rate in ((0.0, 0.0), (0.02, 0.0), (0.02, 0.05)):
        m1, m2 = make_mates(seq, N, start, L, comp, g, indel_rate)
        if rate:
            for m in (m1, m2):
                hit = torch.rand(m.shape, generator=g, device=dev) < rate
                m[hit] = ACGT[torch.randint(0, 4, (int(hit.sum()),), generator=g, device=dev)]
        r1, r2 = (m1.reshape(-1), roff), (m2.reshape(-1), roff)
        hits, hoff = index.map_reads(r1, r2)
        n = hits.numel() // 24
        # the gapped entry against the statement on a slice
        k = min(R, 1500)
        cut = int(hoff[k].item())
        sl1, sl2 = ([bytes(x) for x in m[:k].cpu().numpy()] for m in (m1, m2))
        tx = Transcripts(seq, off)
        sh, so = hits[: cut * 24].cpu().numpy().view(H.HIT_DTYPE), hoff[: k + 1].cpu().numpy()
        edits = H.gapped_edits_host(tx, sh, so, sl1, sl2, K)
        for kb in (False, True):
            dh, do, ds, dst = H.verify_hits(index, hits[: cut * 24], hoff[: k + 1], sl1, sl2, min_identity=0.9, keep_best=kb, max_indel=K)
            wh, wo, ws, wst = H.verify_hits_gapped_host(tx, sh, so, sl1, sl2, 900, kb, K, edits=edits)
            assert np.array_equal(dh.cpu().numpy().view(H.HIT_DTYPE), wh) and np.array_equal(do.cpu().numpy().view(np.uint32), wo)
            assert np.array_equal(ds.cpu().numpy().view(H.GSCORE_DTYPE), ws) and dst == wst, (dst, wst)
        out_hits, out_off, scores = torch.empty_like(hits), torch.empty_like(hoff), torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=dev)
        scratch = torch.empty_like(hits)
        go = _lib.VerifyGOpts(900, 0, K); gst = _lib.VerifyGStats(); o = _lib.VerifyOpts(900, 0); st = _lib.VerifyStats(); n_out = C.c_uint64(0); nh = C.c_uint64(0)
        args = (index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(hits), _lib.ptr(hoff))
        outs = (_lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores), C.byref(n_out))

        def gapped():
            _lib.check(Lb.sfgpu_hits_verify_gapped(*args, C.byref(go), *outs, C.byref(gst), None))

        def ungapped():
            _lib.check(Lb.sfgpu_hits_verify(*args, C.byref(o), *outs, C.byref(st), None))

        def remap():
            _lib.check(Lb.sfgpu_map_reads(index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(scratch), n, _lib.ptr(out_off),
                                          C.byref(nh), None))
        # which jobs run the recurrence, and which stop on a failing band minimum: from the scores of every record (permille 0)
        go.min_identity_permille = 0
        gapped()
        sc = scores.view(torch.int16).view(-1, 4)[:n].to(torch.int32) & 0xFFFF          # edits, ungapped, mate_edits, mate_ungapped
        two = hits.view(-1, 24)[:, 22] == 3
        max_edits = (1000 - 900) * L // 1000
        fail0 = sc[:, 0] > max_edits
        dp0, dp1 = sc[:, 1] > 0, two & ~fail0 & (sc[:, 3] > 0)
        jobs = int(n + two.sum().item())
        dp_jobs = int(dp0.sum().item() + dp1.sum().item())
        stopped = int(fail0.sum().item() + (dp1 & (sc[:, 2] > max_edits)).sum().item())
        skipped = int((two & fail0).sum().item())
        go.min_identity_permille = 900
        g_ms, g_all = timed(gapped)
        gstats = gst.as_dict()
        v_ms, v_all = timed(ungapped)
        m_ms, m_all = timed(remap)
        moved = jobs * L + 56 * n_out.value
        src = torch.empty(moved, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        c_ms, c_all = timed(lambda: dst.copy_(src))
        rows.append(dict(substitution_rate=rate, indel_mate_rate=indel_rate, max_indel=K, pairs=R, records=n, jobs=jobs, gapped_stats=gstats, ungapped_stats=st.as_dict(),
                         gapped_ms=g_ms, gapped_ms_runs=g_all, verify_ms=v_ms, verify_ms_runs=v_all, map_reads_ms=m_ms, map_reads_ms_runs=m_all, d2d_copy_ms=c_ms,
                         d2d_copy_ms_runs=c_all, gapped_over_ungapped=g_ms / v_ms, gapped_over_map=g_ms / m_ms, gapped_over_copy=g_ms / c_ms,
                         dp_jobs=dp_jobs, dp_job_share=dp_jobs / jobs, stopped_jobs=stopped, stopped_job_share=stopped / jobs, jobs_skipped_behind_a_failed_mate=skipped))
        print(json.dumps(rows[-1]), flush=True)
        del src, dst, m1, m2, scratch, out_hits, scores
    index.close()
    return rows


def cost_align(M, R, K, L=100):
    g = torch.Generator(device=dev); g.manual_seed(1)
    ref_len = synth.transcript_lengths(M, device=dev).long()
    off = torch.zeros(M + 1, dtype=torch.int64, device=dev); torch.cumsum(ref_len, 0, out=off[1:])
    N = int(off[-1])
    seq = ACGT[torch.randint(0, 4, (N,), generator=g, device=dev)]
    t = torch.randint(0, M, (R,), generator=g, device=dev)
    p = (torch.rand(R, generator=g, device=dev, dtype=torch.float64) * (ref_len[t] - 250).clamp_min(0).double()).long()
    start = off[t] + p
    comp = torch.zeros(256, dtype=torch.uint8, device=dev); comp[list(b"ACGT")] = torch.tensor(list(b"TGCA"), dtype=torch.uint8, device=dev)
    roff = torch.arange(R + 1, device=dev, dtype=torch.int64) * L
    index = sf.mapper.QuasiIndex((seq, off), device=dev)
    Lb = _lib.lib()
    W = 16 if K <= 7 else 32
    rows = []
    for rate, indel_rate in ((0.0, 0.0), (0.02, 0.05)):
        m1, m2 = make_mates(seq, N, start, L, comp, g, indel_rate)
        if rate:
            for m in (m1, m2):
                hit = torch.rand(m.shape, generator=g, device=dev) < rate
                m[hit] = ACGT[torch.randint(0, 4, (int(hit.sum()),), generator=g, device=dev)]
        r1, r2 = (m1.reshape(-1), roff), (m2.reshape(-1), roff)
        hits, hoff = index.map_reads(r1, r2)
        n_in = hits.numel() // 24
        # the alignment of a slice's survivors against the statement
        k = min(R, 600)
        cut = int(hoff[k].item())
        sl1, sl2 = ([bytes(x) for x in m[:k].cpu().numpy()] for m in (m1, m2))
        tx = Transcripts(seq, off)
        sh, so, _, _ = H.verify_hits(index, hits[: cut * 24], hoff[: k + 1], sl1, sl2, min_identity=0.9, max_indel=K)
        dp, dn, do, dops, dst = H.align_hits(index, sh, so, sl1, sl2, max_indel=K)
        wp, wn, wo, wops, wst, _ = H.align_hits_host(tx, sh.cpu().numpy().view(H.HIT_DTYPE), so.cpu().numpy().view(np.uint32), sl1, sl2, K)
        assert np.array_equal(dp.cpu().numpy(), wp) and np.array_equal(dn.cpu().numpy().view(np.uint32), wn) and np.array_equal(do.cpu().numpy().view(np.uint64), wo)
        assert np.array_equal(dops.cpu().numpy().view(np.uint32), wops) and dst == wst, (dst, wst)
        # the whole batch: its survivors, then the pass on them
        s_hits, s_off, _, gstats = H.verify_hits(index, hits, hoff, r1, r2, min_identity=0.9, max_indel=K)
        s_hits, s_off = s_hits.clone(), s_off.clone()
        n = s_hits.numel() // 24
        pos = torch.empty(2 * n, dtype=torch.int32, device=dev); nm = torch.empty_like(pos); op_off = torch.empty(2 * n + 1, dtype=torch.int64, device=dev)
        ao = _lib.AlignGOpts(K, 0, 0); ast = _lib.AlignGStats(); need = C.c_uint64(0)
        args = (index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R)
        rc = Lb.sfgpu_hits_align_gapped(*args, _lib.ptr(s_hits), _lib.ptr(s_off), C.byref(ao), _lib.ptr(pos), _lib.ptr(nm), _lib.ptr(op_off), None, 0, C.byref(need),
                                        C.byref(ast), None)
        assert rc in (_lib.OK, _lib.ERR_RANGE), rc
        ops = torch.empty(max(need.value, 1), dtype=torch.int32, device=dev)

        def align():
            _lib.check(Lb.sfgpu_hits_align_gapped(*args, _lib.ptr(s_hits), _lib.ptr(s_off), C.byref(ao), _lib.ptr(pos), _lib.ptr(nm), _lib.ptr(op_off), _lib.ptr(ops),
                                                  ops.numel(), C.byref(need), C.byref(ast), None))
        out_hits, out_off, scores = torch.empty_like(hits), torch.empty_like(hoff), torch.empty(max(n_in, 1) * 8, dtype=torch.uint8, device=dev)
        go = _lib.VerifyGOpts(900, 0, K); gst = _lib.VerifyGStats(); n_out = C.c_uint64(0)

        def gapped():
            _lib.check(Lb.sfgpu_hits_verify_gapped(*args, _lib.ptr(hits), _lib.ptr(hoff), C.byref(go), _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores),
                                                   C.byref(n_out), C.byref(gst), None))
        a_ms, a_all = timed(align)
        stats = ast.as_dict()
        g_ms, g_all = timed(gapped)
        whole_scratch = stats["jobs_traced"] * 8 * W * ((L + 15) // 16)
        moved = stats["jobs"] * L + 24 * n + 16 * 2 * n + 4 * stats["words"] + 2 * whole_scratch
        src = torch.empty(moved, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        c_ms, c_all = timed(lambda: dst.copy_(src))
        rows.append(dict(substitution_rate=rate, indel_mate_rate=indel_rate, max_indel=K, pairs=R, records_mapped=n_in, records_aligned=n, align_stats=stats,
                         rescued=gstats["rescued"], align_ms=a_ms, align_ms_runs=a_all, gapped_ms=g_ms, gapped_ms_runs=g_all, bytes_moved=moved, d2d_copy_ms=c_ms,
                         d2d_copy_ms_runs=c_all, align_over_gapped=a_ms / g_ms, align_over_copy=a_ms / c_ms, traced_job_share=stats["jobs_traced"] / max(stats["jobs"], 1),
                         scratch_peak_bytes=stats["scratch_bytes"], scratch_whole_batch_bytes=whole_scratch, words_per_job=stats["words"] / max(stats["jobs"], 1)))
        print(json.dumps(rows[-1]), flush=True)
        del src, dst, m1, m2, out_hits, scores, ops, pos, nm, op_off, s_hits
    index.close()
    return rows


def effect_gapped(K):
    rng = np.random.default_rng(7)
    bases = np.frombuffer(b"ACGT", np.uint8)
    exons = [bytes(rng.choice(bases, rng.integers(40, 221))) for _ in range(60)]
    seqs = []
    for gene in range(10):
        own = exons[6 * gene:6 * gene + 6]
        for iso in range(4):
            keep = [e for i, e in enumerate(own) if i in (0, 5) or rng.random() < 0.6]
            seqs.append(b"".join(keep))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    sub = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}
    truth, reads = [], []
    while len(reads) < 600:
        t = int(rng.integers(0, len(seqs)))
        if len(seqs[t]) < 104:
            continue
        p = int(rng.integers(0, len(seqs[t]) - 103)); fwd = int(rng.random() < 0.5)
        n, at = int(rng.integers(1, 4)), int(rng.integers(1, 96))
        r = seqs[t][p:p + 104]
        r = (r[:at] + r[at + n:] if rng.random() < 0.5 else r[:at] + bytes(rng.choice(bases, n)) + r[at:])[:100]
        b = bytearray(r)
        for i in np.nonzero(rng.random(100) < 0.01)[0]:
            b[i] = sub[b[i]][int(rng.integers(0, 3))]
        r = bytes(b)
        reads.append(r if fwd else r.translate(comp)[::-1]); truth.append((t, fwd, p))
    index = sf.mapper.QuasiIndex(seqs, device=dev)
    hits, off = index.map_reads(reads)
    h, o = sf.mapper.hits_to_numpy(hits, off)

    def is_true(h, o):
        """per record: the read's source transcript and strand, within 4 bases of where the read was cut (either side of the indel)"""
        out = np.zeros(len(h), bool)
        for r, (t, f, p) in enumerate(truth):
            sl = slice(o[r], o[r + 1])
            out[sl] = (h["tid"][sl] == t) & (h["fwd"][sl] == f) & (np.abs(h["pos"][sl].astype(np.int64) - p) <= 4)
        return out
    rows = []
    kept = {}
    for k in (0, K):
        vh, vo, _, st = H.verify_hits(index, hits, off, reads, min_identity=0.9, max_indel=k)
        kh, ko = sf.mapper.hits_to_numpy(vh, vo)
        kept[k] = set(zip(np.repeat(np.arange(len(reads)), np.diff(ko)).tolist(), map(bytes, kh)))
        tr = is_true(kh, ko)
        rows.append(dict(max_indel=k, min_identity=0.9, reads=len(reads), records=len(h), true_records=int(is_true(h, o).sum()), records_kept=len(kh),
                         true_records_lost=int(is_true(h, o).sum() - tr.sum()), false_records_kept=int((~tr).sum()), reads_mapped=st["reads_in"],
                         reads_left_without_records=st["reads_in"] - st["reads_out"]))
        print(json.dumps(rows[-1]), flush=True)
    rows[-1]["false_records_gained_over_max_indel_0"] = rows[-1]["false_records_kept"] - rows[0]["false_records_kept"]
    assert kept[0] <= kept[K]
    index.close()
    return rows


def effect():
    rng = np.random.default_rng(7)
    bases = np.frombuffer(b"ACGT", np.uint8)
    exons = [bytes(rng.choice(bases, rng.integers(40, 221))) for _ in range(60)]
    seqs = []
    for gene in range(10):
        own = exons[6 * gene:6 * gene + 6]
        for iso in range(4):
            keep = [e for i, e in enumerate(own) if i in (0, 5) or rng.random() < 0.6]
            seqs.append(b"".join(keep))
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    truth, clean = [], []
    while len(clean) < 600:
        t = int(rng.integers(0, len(seqs)))
        if len(seqs[t]) < 100:
            continue
        p = int(rng.integers(0, len(seqs[t]) - 99)); fwd = int(rng.random() < 0.5)
        r = seqs[t][p:p + 100]
        clean.append(r if fwd else r.translate(comp)[::-1]); truth.append((t, fwd, p))
    index = sf.mapper.QuasiIndex(seqs, device=dev)
    sub = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}
    rows = []
    for rate in (0.0, 0.01, 0.02, 0.04):
        reads = []
        for r in clean:
            b = bytearray(r)
            for i in np.nonzero(rng.random(100) < rate)[0]:
                b[i] = sub[b[i]][int(rng.integers(0, 3))]
            reads.append(bytes(b))
        hits, off = index.map_reads(reads)
        h, o = sf.mapper.hits_to_numpy(hits, off)

        def true_records(h, o):
            return sum(int(((h["tid"][o[r]:o[r + 1]] == t) & (h["fwd"][o[r]:o[r + 1]] == f) & (h["pos"][o[r]:o[r + 1]] == p)).any()) for r, (t, f, p) in enumerate(truth))
        for mi in (0.85, 0.9, 0.95):
            vh, vo, _, st = H.verify_hits(index, hits, off, reads, min_identity=mi)
            kh, ko = sf.mapper.hits_to_numpy(vh, vo)
            rows.append(dict(substitution_rate=rate, min_identity=mi, records=len(h), records_dropped=len(h) - len(kh), true_records=true_records(h, o),
                             true_records_dropped=true_records(h, o) - true_records(kh, ko), reads_mapped=st["reads_in"],
                             reads_left_without_records=st["reads_in"] - st["reads_out"]))
            print(json.dumps(rows[-1]), flush=True)
    index.close()
    return rows


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?", default=None, help="where the JSON goes (default: profiles/verify_probe.json, or verifyg_probe.json with --max-indel)")
    ap.add_argument("--max-indel", type=int, nargs="?", const=3, default=None, metavar="K", help="run the gapped legs (sfgpu_hits_verify_gapped) with band K, default 3")
    ap.add_argument("--align", action="store_true", help="with --max-indel: run the alignment leg (sfgpu_hits_align_gapped) -> profiles/aligng_probe.json")
    a = ap.parse_args()
    if a.align and a.max_indel is None:
        ap.error("--align needs --max-indel")
    M, R = int(os.environ.get("VERIFY_M", 80000)), int(os.environ.get("VERIFY_R", 10_000_000))
    if a.align:
        out = dict(device=torch.cuda.get_device_name(0), transcripts=M, max_indel=a.max_indel, cost=cost_align(M, R, a.max_indel))
    elif a.max_indel is None:
        out = dict(device=torch.cuda.get_device_name(0), transcripts=M, effect=effect(), cost=cost(M, R))
    else:
        out = dict(device=torch.cuda.get_device_name(0), transcripts=M, max_indel=a.max_indel, effect=effect_gapped(a.max_indel), cost=cost_gapped(M, R, a.max_indel))
    path = a.path or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                  "aligng_probe.json" if a.align else "verifyg_probe.json" if a.max_indel is not None else "verify_probe.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)
