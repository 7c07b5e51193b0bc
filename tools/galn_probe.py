"""dev probe: what the projection of a batch onto the genome (sfgpu_galn_project) costs -> profiles/galn_probe.json

On the verification probe's batch (tools/verify_probe.py: 80 000 transcripts, VERIFY_R pairs of 2 x 100 bases) under the covgenome probe's
synthetic annotation (tools/covgenome_probe.py: genes of 4 isoforms over exons of 150 to 400 bases, both strands, 24 chromosomes), two
legs: the error-free mates with no alignment given (the writer's <len>M) and no tags; and 2 % substitutions plus one indel of 1 - 3
bases in 5 % of the mates, with the alignments of sfgpu_hits_align_gapped (max_indel 3) on the survivors of sfgpu_hits_verify_gapped at
0.9 and the tags of sfgpu_hits_md_tags.  On a slice the device result is first asserted equal to hits.project_alignments_host.  Then
medians of 5 after a warm-up of sfgpu_galn_project into preallocated room (wall ms, the call's own device-event ms and its stages:
the size pass, the scans, the emit pass with the counts' way to the host before it), beside
sfgpu_hits_md_tags on the same records and a plain device copy of the bytes the pass reads and writes: the records in and out, 12
bytes a slot of position, nm and offset on either side, the words in and out, the MD bytes in and out, and what the size pass leaves
for the emit pass (32 bytes a slot plus 8 a record, written once and read once)."""
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
import covgenome_probe as CP
import verify_probe as VP

dev, ACGT = VP.dev, VP.ACGT


def _same(got, want):
    h, off, aln, tags, src, st = got
    n = lambda t, dt: t.cpu().numpy().view(dt).reshape(-1)      # noqa: E731
    assert n(h, H.HIT_DTYPE).tobytes() == want[0].tobytes() and np.array_equal(n(off, np.uint32), want[1]) and np.array_equal(n(src, np.uint32), want[4])
    for g, w, dt in zip(aln, want[2], (np.int32, np.uint32, np.uint64, np.uint32)):
        assert np.array_equal(n(g, dt), w)
    for g, w, dt in zip(tags or (), want[3] or (), (np.uint32, np.uint64, np.uint8)):
        assert np.array_equal(n(g, dt), w)
    assert {k: st[k] for k in want[5]} == want[5], (st, want[5])


def probe(M, R, K=3, L=100):
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
    pl, model_s = CP.annotation(ref_len.to(torch.int32).cpu().numpy().view(np.uint32))
    Lb = _lib.lib()
    rows = []
    with H.GenomeAlignments(pl, dev) as model:
        for rate, indel_rate, aligned in ((0.0, 0.0, False), (0.02, 0.05, True)):
            m1, m2 = VP.make_mates(seq, N, start, L, comp, g, indel_rate)
            if rate:
                for m in (m1, m2):
                    hit = torch.rand(m.shape, generator=g, device=dev) < rate
                    m[hit] = ACGT[torch.randint(0, 4, (int(hit.sum()),), generator=g, device=dev)]
            r1, r2 = (m1.reshape(-1), roff), (m2.reshape(-1), roff)
            hits, hoff = index.map_reads(r1, r2)
            aln = tags = None
            if aligned:
                hits, hoff, _, _ = H.verify_hits(index, hits, hoff, r1, r2, min_identity=0.9, max_indel=K)
                hits, hoff = hits.clone(), hoff.clone()
                aln = H.align_hits(index, hits, hoff, r1, r2, max_indel=K)[:4]
                tags = H.md_tags(index, hits, hoff, r1, r2, aln)[:3]
            n = hits.numel() // 24
            # a slice against the statement
            k = min(R, 2000)
            cut = int(hoff[k].item())
            s_aln = s_tags = None
            if aligned:
                w_end, m_end = int(aln[2][2 * cut].item()), int(tags[1][2 * cut].item())
                s_aln = (aln[0][:2 * cut], aln[1][:2 * cut], aln[2][:2 * cut + 1], aln[3][:w_end])
                s_tags = (tags[0][:2 * cut], tags[1][:2 * cut + 1], tags[2][:m_end])
            host = lambda x, dt: x.cpu().numpy().view(dt)      # noqa: E731
            want = H.project_alignments_host(host(hits[:24 * cut], H.HIT_DTYPE), host(hoff[:k + 1], np.uint32), pl,
                                             None if s_aln is None else tuple(host(x, dt) for x, dt in zip(s_aln, (np.int32, np.uint32, np.uint64, np.uint32))),
                                             None if s_tags is None else tuple(host(x, dt) for x, dt in zip(s_tags, (np.uint32, np.uint64, np.uint8))))
            _same(H.project_alignments(hits[:24 * cut].contiguous(), hoff[:k + 1].contiguous(), model,
                                       None if s_aln is None else tuple(x.contiguous() for x in s_aln), None if s_tags is None else tuple(x.contiguous() for x in s_tags)), want)
            # the whole batch, into room that is there
            *_, st0 = H.project_alignments(hits, hoff, model, aln, tags)
            words_in, md_in = (int(aln[3].numel()), int(tags[2].numel())) if aligned else (0, 0)
            o_hits = torch.empty(24 * n, dtype=torch.uint8, device=dev); o_off = torch.empty(R + 1, dtype=torch.int32, device=dev)
            o_pos, o_nm, o_tnm = (torch.empty(2 * n, dtype=torch.int32, device=dev) for _ in range(3))
            o_aoff, o_moff = (torch.empty(2 * n + 1, dtype=torch.int64, device=dev) for _ in range(2))
            src = torch.empty(n, dtype=torch.int32, device=dev)
            ops = torch.empty(max(st0["words_out"], 1), dtype=torch.int32, device=dev); md = torch.empty(max(md_in, 1), dtype=torch.uint8, device=dev)
            b = _lib.GalnBatch(_lib.ptr(hits), _lib.ptr(hoff), R, 0)
            if aligned:
                b.aln_pos, b.aln_op_off, b.aln_ops, b.aln_nm = _lib.ptr(aln[0]), _lib.ptr(aln[2]), _lib.ptr(aln[3]), _lib.ptr(aln[1])
                b.tag_nm, b.tag_md_off, b.tag_md = _lib.ptr(tags[0]), _lib.ptr(tags[1]), _lib.ptr(tags[2])
            o = _lib.GalnOut(_lib.ptr(o_hits), _lib.ptr(o_off), _lib.ptr(o_pos), _lib.ptr(o_nm), _lib.ptr(o_aoff), _lib.ptr(ops), ops.numel(), _lib.ptr(o_tnm),
                             _lib.ptr(o_moff), _lib.ptr(md), md_in, _lib.ptr(src))
            st, need_ops, need_md, own = _lib.GalnStats(), C.c_uint64(0), C.c_uint64(0), []

            def project():
                _lib.check(Lb.sfgpu_galn_project(model._h, C.byref(b), C.byref(o), C.byref(need_ops), C.byref(need_md), C.byref(st), None))
                own.append((st.project_ms, st.size_ms, st.scan_ms, st.emit_ms))
            p_ms, p_all = VP.timed(project)
            stats = {key: int(getattr(st, key)) for key in H.GENOME_ALN_STATS}
            assert stats == {key: st0[key] for key in stats}
            t_nm = torch.empty(2 * n, dtype=torch.int32, device=dev); t_off = torch.empty(2 * n + 1, dtype=torch.int64, device=dev)
            tst = _lib.MdTagStats(); need = C.c_uint64(0)
            a_ptrs = (_lib.ptr(aln[0]), _lib.ptr(aln[2]), _lib.ptr(aln[3])) if aligned else (None, None, None)
            args = (index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(hits), _lib.ptr(hoff), *a_ptrs, _lib.ptr(t_nm), _lib.ptr(t_off))
            rc = Lb.sfgpu_hits_md_tags(*args, None, 0, C.byref(need), C.byref(tst), None)
            assert rc in (_lib.OK, _lib.ERR_RANGE), rc
            t_md = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
            t_ms, t_all = VP.timed(lambda: _lib.check(Lb.sfgpu_hits_md_tags(*args, _lib.ptr(t_md), t_md.numel(), C.byref(need), C.byref(tst), None)))
            m_out = stats["records_out"]
            slot_in, slot_out = (28, 28) if aligned else (0, 16)     # position 4, nm 4, offset 8; with tags nm 4 and offset 8 more
            scratch = 2 * (8 * n + 32 * 2 * n)                         # written by one pass, read by the next: 8 a record, 32 a slot
            moved = 24 * (n + m_out) + 8 * (R + 1) + 2 * n * slot_in + 2 * m_out * slot_out + 4 * (words_in + stats["words_out"]) + md_in + int(need_md.value) + scratch
            cs = torch.empty(moved // 2, dtype=torch.uint8, device=dev); cd = torch.empty_like(cs)
            c_ms, c_all = VP.timed(lambda: cd.copy_(cs))
            rows.append(dict(substitution_rate=rate, indel_mate_rate=indel_rate, aligned=aligned, tagged=aligned, pairs=R, records=n, stats=stats,
                             project_ms=p_ms, project_ms_runs=p_all, **{key: sorted(x[i] for x in own[1:])[len(own[1:]) // 2] for i, key in enumerate(("project_device_ms", "size_ms", "scan_ms", "emit_ms"))},
                             device_ms_runs=[list(x) for x in own[1:]],
                             md_tags_ms=t_ms, md_tags_ms_runs=t_all, bytes_moved=moved, d2d_copy_ms=c_ms, d2d_copy_ms_runs=c_all, project_over_md_tags=p_ms / t_ms,
                             project_over_copy=p_ms / c_ms, project_ms_per_10M_pairs=p_ms * 1e7 / R))
            print(json.dumps(rows[-1]), flush=True)
            del m1, m2, o_hits, ops, md, cs, cd, t_md
    index.close()
    return dict(transcripts=M, blocks=int(pl.exon_off[-1]), chromosomes=CP.N_CHROM, annotation_host_s=model_s, rows=rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?", default=os.path.join(ROOT, "profiles", "galn_probe.json"))
    a = ap.parse_args()
    M, R = int(os.environ.get("VERIFY_M", 80000)), int(os.environ.get("VERIFY_R", 10_000_000))
    doc = dict(device=torch.cuda.get_device_name(0), **probe(M, R))
    with open(a.path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.path)
