"""dev probe: what the NM / MD tag pass (sfgpu_hits_md_tags) costs -> profiles/mdtag_probe.json

On the batch of tools/verify_probe.py (80 000 transcripts, VERIFY_R pairs of 2 x 100 bases from fragments of 250), error-free without
alignments, and with 2 % substitutions plus one indel of 1 - 3 bases in 5 % of the mates with the alignments of sfgpu_hits_align_gapped
(max_indel 3) on the survivors of sfgpu_hits_verify_gapped at 0.9: the pass's result on a slice is first asserted equal to
hits.md_tags_host; then medians of 5 after a warm-up of sfgpu_hits_md_tags (with exactly the room it needs), of sfgpu_hits_verify on the
same records (it reads the same bases), and of a plain device-to-device copy of the bytes the pass moves (each line's mate bases and
as many transcript bases, 24 bytes a record, 4 + 8 bytes a slot, the operations, the MD bytes); and the share of plain slots."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sailfish_amd as sf
from sailfish_amd import _lib, hits as H, synth
import verify_probe as VP

dev = VP.dev
ACGT = VP.ACGT


def cost(M, R, K=3, L=100):
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
    for rate, indel_rate, aligned in ((0.0, 0.0, False), (0.02, 0.05, True)):
        m1, m2 = VP.make_mates(seq, N, start, L, comp, g, indel_rate)
        if rate:
            for m in (m1, m2):
                hit = torch.rand(m.shape, generator=g, device=dev) < rate
                m[hit] = ACGT[torch.randint(0, 4, (int(hit.sum()),), generator=g, device=dev)]
        r1, r2 = (m1.reshape(-1), roff), (m2.reshape(-1), roff)
        hits, hoff = index.map_reads(r1, r2)
        # the pass on a slice against the statement
        k = min(R, 600)
        cut = int(hoff[k].item())
        sl1, sl2 = ([bytes(x) for x in m[:k].cpu().numpy()] for m in (m1, m2))
        tx = VP.Transcripts(seq, off)
        sh, so = hits[: cut * 24], hoff[: k + 1]
        d_aln = w_aln = None
        if aligned:
            sh, so, _, _ = H.verify_hits(index, sh, so, sl1, sl2, min_identity=0.9, max_indel=K)
            d_aln = H.align_hits(index, sh, so, sl1, sl2, max_indel=K)
            w_aln = tuple(a.cpu().numpy() for a in d_aln[:4])
        dn, do, dm, dst = H.md_tags(index, sh, so, sl1, sl2, d_aln)
        wn, wo, wm, wst = H.md_tags_host(tx, sh.cpu().numpy().view(H.HIT_DTYPE), so.cpu().numpy().view(np.uint32), sl1, sl2, w_aln)
        assert np.array_equal(dn.cpu().numpy().view(np.uint32), wn) and np.array_equal(do.cpu().numpy().view(np.uint64), wo)
        assert dm.cpu().numpy().tobytes() == wm.tobytes() and dst == wst, (dst, wst)
        # the whole batch
        if aligned:
            s_hits, s_off, _, _ = H.verify_hits(index, hits, hoff, r1, r2, min_identity=0.9, max_indel=K)
            s_hits, s_off = s_hits.clone(), s_off.clone()
            aln = H.align_hits(index, s_hits, s_off, r1, r2, max_indel=K)
            a_ptrs, words = (_lib.ptr(aln[0]), _lib.ptr(aln[2]), _lib.ptr(aln[3])), int(aln[3].numel())
        else:
            s_hits, s_off, a_ptrs, words = hits, hoff, (None, None, None), 0
        n = s_hits.numel() // 24
        nm = torch.empty(2 * n, dtype=torch.int32, device=dev); md_off = torch.empty(2 * n + 1, dtype=torch.int64, device=dev)
        st = _lib.MdTagStats(); need = C.c_uint64(0)
        args = (index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(s_hits), _lib.ptr(s_off), *a_ptrs, _lib.ptr(nm), _lib.ptr(md_off))
        rc = Lb.sfgpu_hits_md_tags(*args, None, 0, C.byref(need), C.byref(st), None)
        assert rc in (_lib.OK, _lib.ERR_RANGE), rc
        md = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)

        def tags():
            _lib.check(Lb.sfgpu_hits_md_tags(*args, _lib.ptr(md), md.numel(), C.byref(need), C.byref(st), None))
        out_hits, out_off, scores = torch.empty_like(s_hits), torch.empty_like(s_off), torch.empty(max(n, 1) * 8, dtype=torch.uint8, device=dev)
        o = _lib.VerifyOpts(900, 0); vst = _lib.VerifyStats(); n_out = C.c_uint64(0)

        def verify():
            _lib.check(Lb.sfgpu_hits_verify(index._h, _lib.ptr(r1[0]), _lib.ptr(roff), _lib.ptr(r2[0]), _lib.ptr(roff), R, _lib.ptr(s_hits), _lib.ptr(s_off), C.byref(o),
                                            _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores), C.byref(n_out), C.byref(vst), None))
        t_ms, t_all = VP.timed(tags)
        stats = st.as_dict()
        v_ms, v_all = VP.timed(verify)
        moved = 2 * stats["slots"] * L + 24 * n + 12 * 2 * n + 4 * words + stats["md_bytes"]
        src = torch.empty(moved, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
        c_ms, c_all = VP.timed(lambda: dst.copy_(src))
        rows.append(dict(substitution_rate=rate, indel_mate_rate=indel_rate, aligned=aligned, max_indel=K if aligned else 0, pairs=R, records=n, tag_stats=stats,
                         md_tags_ms=t_ms, md_tags_ms_runs=t_all, verify_ms=v_ms, verify_ms_runs=v_all, bytes_moved=moved, d2d_copy_ms=c_ms, d2d_copy_ms_runs=c_all,
                         md_tags_over_verify=t_ms / v_ms, md_tags_over_copy=t_ms / c_ms, plain_slot_share=stats["slots_plain"] / max(stats["slots"], 1),
                         md_tags_ms_per_10M_pairs=t_ms * 1e7 / R))
        print(json.dumps(rows[-1]), flush=True)
        del src, dst, m1, m2, out_hits, scores, md, nm, md_off
    index.close()
    return rows


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("path", nargs="?", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mdtag_probe.json"))
    a = ap.parse_args()
    M, R = int(os.environ.get("VERIFY_M", 80000)), int(os.environ.get("VERIFY_R", 10_000_000))
    out = dict(device=torch.cuda.get_device_name(0), transcripts=M, cost=cost(M, R))
    with open(a.path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.path)
