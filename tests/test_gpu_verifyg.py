"""Gapped hit verification on the device (csrc/verify.hip: sfgpu_hits_verify_gapped; hits.verify_hits(max_indel=);
QuasiIndex.map_reads(validate=); validate_mappings= / max_indel= of mapper.quantify_reads) against the Python statement
hits.verify_hits_gapped_host: record for record, offsets, scores and stats over the shared corpus (tests/verifyg_corpus.py) for both
group widths, the contract's errors and shapes, max_indel = 0 unchanged, and end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import verify_corpus as old_corpus
import verifyg_corpus as corpus
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _index(case, gpu):
    import sailfish_amd as sf
    return sf.mapper.QuasiIndex(case["seqs"], device=gpu)


def _device(case, gpu):
    import torch
    hits = torch.from_numpy(case["hits"].view(np.uint8).reshape(-1).copy()).to(gpu)
    off = torch.from_numpy(case["off"].view(np.int32).copy()).to(gpu)
    return hits, off


def _numpy(h, o, s, dtype=None):
    from sailfish_amd import hits as H
    return h.cpu().numpy().view(O.HIT_DTYPE), o.cpu().numpy().view(np.uint32), s.cpu().numpy().view(dtype or H.GSCORE_DTYPE)


def _same(got, want, what):
    h, o, s, st = got
    wh, wo, ws, wst = want
    assert np.array_equal(o, wo), what
    assert np.array_equal(h, wh), what
    assert np.array_equal(s, ws), what
    assert st == wst, (what, st, wst)


def test_deletion_in_the_middle_is_rescued(gpu):
    """the first thing to look at: 2 transcript bases missing in the middle of a mate -- dropped at max_indel = 0, kept with edits == 2 at 3"""
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    t = corpus.cases()["indels_se"]["seqs"][0]
    read = t[100:150] + t[152:202]
    idx = sf.mapper.QuasiIndex([t], device=gpu)
    rec = np.array([(0, 100, 0, 0, 100, 0, 1, 0, 0, 0)], dtype=H.HIT_DTYPE)
    h, o, s, st = H.verify_hits(idx, rec, np.array([0, 1], np.uint32), [read], max_indel=0)
    assert h.numel() == 0 and st["failed_identity"] == 1 and "rescued" not in st
    h, o, s, st = H.verify_hits(idx, rec, np.array([0, 1], np.uint32), [read], max_indel=3)
    h, o, s = _numpy(h, o, s)
    assert np.array_equal(h, rec) and o.tolist() == [0, 1] and int(s["edits"][0]) == 2 and int(s["ungapped"][0]) > 25 and s["mate_edits"][0] == s["mate_ungapped"][0] == 0
    assert st == dict(records_in=1, records_out=1, reads_in=1, reads_out=1, failed_identity=0, dropped_not_best=0, sum_edits=2, rescued=1)
    assert H.verify_hits(idx, rec, np.array([0, 1], np.uint32), [read], max_indel=1)[0].numel() == 0
    idx.close()


@pytest.mark.parametrize("name", ["pe_indel", "se_indel", "edges_pe", "edges_se", "indels_pe", "indels_se", "long"])
def test_device_equals_the_statement(gpu, name):
    """every case of the corpus, max_indel 1 2 3 7 (groups of 16 lanes) 8 15 (of 32), permille 0 / 900 / 1000, keep_best on and off"""
    from sailfish_amd import hits as H
    case = corpus.cases()[name]
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    import sailfish_amd as sf
    r1 = tuple(t.to(gpu) for t in sf.mapper.pack_sequences(case["r1"]))
    r2 = None if case["r2"] is None else tuple(t.to(gpu) for t in sf.mapper.pack_sequences(case["r2"]))
    for k in corpus.KS:
        for permille, kb in corpus.OPTIONS:
            h, o, s, st = H.verify_hits(idx, d_hits, d_off, r1, r2, min_identity=permille / 1000, keep_best=kb, max_indel=k)
            _same((*_numpy(h, o, s), st), corpus.expected(name, k, permille, kb), (name, k, permille, kb))
    idx.close()


def _raw(idx, s1, o1, s2, o2, n_reads, d_hits, d_off, permille, kb, k, out_hits, out_off, scores, n_out=True, stats=True, opts=True, index=True):
    """sfgpu_hits_verify_gapped itself -> (rc, n_out, stats)"""
    import torch
    from sailfish_amd import _lib
    o = _lib.VerifyGOpts(permille, int(kb), k)
    st = _lib.VerifyGStats()
    n = C.c_uint64(12345)
    with torch.cuda.device(idx.device):
        torch.cuda.synchronize()
        rc = _lib.lib().sfgpu_hits_verify_gapped(idx._h if index else None, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), n_reads, _lib.ptr(d_hits),
                                                 _lib.ptr(d_off), C.byref(o) if opts else None, _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(scores),
                                                 C.byref(n) if n_out else None, C.byref(st) if stats else None, _lib.current_stream_ptr())
        torch.cuda.synchronize()
    return rc, n.value, st.as_dict()


def test_shapes_of_the_contract(gpu):
    """reads that begin at offsets that are no multiples of 16 (and a packed buffer that does not begin at 0); d_scores_out == NULL; a
    batch with no records; a batch where nothing survives; n_reads == 0"""
    import torch
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    name = "pe_indel"
    case = corpus.cases()[name]
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    zero = dict.fromkeys(H.VERIFYG_STATS, 0)
    for k in (3, 8):
        want = corpus.expected(name, k, 900, True)
        packs = []
        for reads, lead in ((case["r1"], b"xyz"), (case["r2"], b"NNNNNNN")):
            b, o = sf.mapper.pack_sequences([lead] + list(reads))
            assert any(int(x) % 16 for x in o)
            packs.append((b.to(gpu), o[1:].contiguous().to(gpu)))
        h, o, s, st = H.verify_hits(idx, d_hits, d_off, packs[0], packs[1], min_identity=0.9, keep_best=True, max_indel=k)
        _same((*_numpy(h, o, s), st), want, "offset reads")
        # no scores wanted
        R, n = len(case["r1"]), len(case["hits"])
        out_hits, out_off = torch.zeros(n * 24, dtype=torch.uint8, device=gpu), torch.zeros(R + 1, dtype=torch.int32, device=gpu)
        rc, n_out, st = _raw(idx, *packs[0], *packs[1], R, d_hits, d_off, 900, True, k, out_hits, out_off, None)
        assert rc == 0 and n_out == len(want[0]) and st == want[3]
        assert np.array_equal(out_hits[: n_out * 24].cpu().numpy().view(O.HIT_DTYPE), want[0]) and np.array_equal(out_off.cpu().numpy().view(np.uint32), want[1])
        # no records at all
        none_h, none_o = torch.zeros(0, dtype=torch.uint8, device=gpu), torch.zeros(R + 1, dtype=torch.int32, device=gpu)
        h, o, s, st = H.verify_hits(idx, none_h, none_o, case["r1"], case["r2"], max_indel=k)
        assert h.numel() == 0 and s.numel() == 0 and not o.any().item() and o.numel() == R + 1 and st == zero
        rc, n_out, st = _raw(idx, *packs[0], *packs[1], R, None, none_o, 900, False, k, None, out_off, None)
        assert rc == 0 and n_out == 0 and not out_off.any().item()
        # n_reads == 0
        one = torch.full((1,), 7, dtype=torch.int32, device=gpu)
        rc, n_out, st = _raw(idx, None, None, None, None, 0, None, None, 900, False, k, None, one, None)
        assert rc == 0 and n_out == 0 and one.item() == 0 and st == zero
        h, o, s, st = H.verify_hits(idx, none_h, none_o[:1], [], [], max_indel=k)
        assert h.numel() == 0 and o.tolist() == [0] and st["records_in"] == 0
    idx.close()
    # nothing survives: reads that share one seed with a transcript
    rng = np.random.default_rng(32)
    seqs = old_corpus.clean_transcripts(rng)
    reads = old_corpus.planted_reads(rng, seqs, 120)
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    mh, mo = idx.map_reads(reads)
    assert mh.numel() // 24 >= len(reads)
    for k in (3, 15):
        h, o, s, st = H.verify_hits(idx, mh, mo, reads, max_indel=k)
        assert h.numel() == 0 and s.numel() == 0 and not o.any().item() and st["records_in"] == st["failed_identity"] == mh.numel() // 24 and st["reads_out"] == 0
        assert st == H.verify_hits_gapped_host(seqs, *sf.mapper.hits_to_numpy(mh, mo), reads, None, 900, False, k)[3]
    idx.close()


def test_errors(gpu):
    """tid >= M: SFGPU_ERR_RANGE naming the lowest such record, the outputs untouched; null pointers, a permille above 1000, a max_indel
    outside 1 .. 15 and mate 2 in a single-end batch: SFGPU_ERR_INVALID; the Python surface raises ValueError before any device work"""
    import torch
    import sailfish_amd as sf
    from sailfish_amd import _lib
    from sailfish_amd import hits as H
    case = corpus.cases()["edges_pe"]
    idx = _index(case, gpu)
    bad = dict(case)
    bad["hits"] = case["hits"].copy()
    bad["hits"]["tid"][[40, 17, 99]] = len(case["seqs"])
    d_hits, d_off = _device(bad, gpu)
    good_hits, _ = _device(case, gpu)
    s1, o1 = (t.to(gpu) for t in sf.mapper.pack_sequences(case["r1"]))
    s2, o2 = (t.to(gpu) for t in sf.mapper.pack_sequences(case["r2"]))
    R, n = len(case["r1"]), len(case["hits"])
    out_hits, out_off, scores = (torch.full((k,), 0x5A, dtype=torch.uint8, device=gpu) for k in (n * 24, (R + 1) * 4, n * 8))
    for k in (3, 15):
        rc, n_out, st = _raw(idx, s1, o1, s2, o2, R, d_hits, d_off, 900, False, k, out_hits, out_off, scores)
        assert rc == _lib.ERR_RANGE and b"record 17 " in _lib.lib().sfgpu_last_error()
        assert all(bool((t == 0x5A).all().item()) for t in (out_hits, out_off, scores))
    with pytest.raises(_lib.SfgpuError, match="record 17 "):
        H.verify_hits(idx, d_hits, d_off, case["r1"], case["r2"], max_indel=3)
    args = dict(idx=idx, s1=s1, o1=o1, s2=s2, o2=o2, n_reads=R, d_hits=good_hits, d_off=d_off, permille=900, kb=False, k=3, out_hits=out_hits, out_off=out_off, scores=scores)
    for change in (dict(index=False), dict(opts=False), dict(n_out=False), dict(stats=False), dict(out_off=None), dict(s1=None), dict(o1=None), dict(o2=None),
                   dict(d_off=None), dict(d_hits=None), dict(out_hits=None), dict(permille=1001), dict(k=0), dict(k=16), dict(k=0xFFFFFFFF),
                   dict(s2=None, o2=None)):                           # (the last: records name mate 2)
        rc, _, _ = _raw(**{**args, **change})
        assert rc == _lib.ERR_INVALID, change
    assert b"mate 2" in _lib.lib().sfgpu_last_error()
    assert all(bool((t == 0x5A).all().item()) for t in (out_hits, out_off, scores))
    rc, n_out, st = _raw(**args)
    assert rc == 0 and n_out == len(corpus.expected("edges_pe", 3, 900, False)[0])
    for k in (16, -1):
        with pytest.raises(ValueError):
            H.verify_hits(idx, good_hits, d_off, case["r1"], case["r2"], max_indel=k)
        with pytest.raises(ValueError):
            sf.mapper.quantify_reads(["t"], [b"ACGT" * 20], [b"ACGT" * 10], None, "U", "unused", validate_mappings=True, max_indel=k, device=gpu)
    idx.close()


def test_max_indel_0_is_the_ungapped_pass(gpu):
    """verify_hits(max_indel=0) returns exactly what verify_hits returned before the option existed: the old corpus's expected result"""
    from sailfish_amd import hits as H
    for name in ("pe_5pc", "se_3pc", "edges_pe"):
        case = old_corpus.cases()[name]
        idx = _index(case, gpu)
        d_hits, d_off = _device(case, gpu)
        for permille, kb in old_corpus.OPTIONS:
            h, o, s, st = H.verify_hits(idx, d_hits, d_off, case["r1"], case["r2"], min_identity=permille / 1000, keep_best=kb, max_indel=0)
            _same((*_numpy(h, o, s, H.SCORE_DTYPE), st), old_corpus.expected(name, permille, kb), (name, permille, kb))
        idx.close()


def _spliced_indel_reads(seed=7, n_reads=500):
    """the spliced synthetic transcriptome of tools/verify_probe.py (60 random exons, ten genes of four isoforms) with single-end reads
    of 100 bases from either strand, 1 % substitutions, and in every second read one insertion or deletion of 1 - 3 bases"""
    rng = np.random.default_rng(seed)
    exons = [bytes(rng.choice(old_corpus.ACGT, rng.integers(40, 221))) for _ in range(60)]
    seqs = []
    for gene in range(10):
        own = exons[6 * gene:6 * gene + 6]
        for _ in range(4):
            seqs.append(b"".join(e for i, e in enumerate(own) if i in (0, 5) or rng.random() < 0.6))
    reads = []
    while len(reads) < n_reads:
        t = seqs[int(rng.integers(0, len(seqs)))]
        if len(t) < 104:
            continue
        p = int(rng.integers(0, len(t) - 103))
        r = t[p:p + 104]
        if len(reads) % 2:
            r = corpus.with_indel(rng, r, 1, 3)
        r = old_corpus.with_errors(rng, [r[:100]], 0.01)[0]
        reads.append(r if rng.random() < 0.5 else old_corpus.revcomp(r))
    return ["tx%d" % i for i in range(len(seqs))], seqs, reads


def test_map_reads_and_quantify_with_gapped_validation(gpu, tmp_path):
    """map_reads(validate={"max_indel": 3}) is verify_hits applied to the plain map_reads; quantify_reads(validate_mappings=True,
    max_indel=3) keeps strictly more records than max_indel=0, reports them as rescued, and its quant.sf and aux/eq_classes.txt are those
    of quant.quantify fed the statement's survivors"""
    import torch
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    from sailfish_amd import quant
    names, seqs, reads = _spliced_indel_reads()
    batch = 200
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ph, po = idx.map_reads(reads)
    wh, wo, ws, wst = H.verify_hits(idx, ph, po, reads, max_indel=3, keep_best=True)
    h, o = idx.map_reads(reads, validate=dict(max_indel=3, keep_best=True))
    assert torch.equal(h, wh) and torch.equal(o, wo) and torch.equal(idx.last_scores, ws) and idx.last_verify_stats == wst and wst["rescued"] > 0
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)
    log = []
    sopt = lambda: sf.SailfishOpts(dumpEq=True, jointLog=lambda lvl, msg: log.append(msg))
    filtered, total = [], dict.fromkeys(H.VERIFYG_STATS, 0)
    for a in range(0, len(reads), batch):
        bh, bo = sf.mapper.hits_to_numpy(*idx.map_reads(reads[a:a + batch]))
        fh, fo, _, st = H.verify_hits_gapped_host(seqs, bh, bo, reads[a:a + batch], None, 900, False, 3)
        filtered.append((fh, fo))
        for key in total:
            total[key] += st[key]
    idx.close()
    assert total["rescued"] >= 50 and total["failed_identity"] > 0
    rc, _ = quant.quantify(names, ref_len, iter(filtered), "U", str(tmp_path / "want"), sopt(), device=gpu, cmd_options={"libType": "U"})
    assert rc == 0
    rc, exp = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "got"), sopt(), batch_reads=batch, device=gpu, cmd_options={"libType": "U"},
                                       validate_mappings=True, max_indel=3)
    assert rc == 0 and exp.verify_stats == total
    line = [m for m in log if m.startswith("validated mappings")]
    assert len(line) == 1 and "max indel 3" in line[0] and f"{total['rescued']} records kept only with gaps" in line[0]
    for rel in ("quant.sf", os.path.join("aux", "eq_classes.txt")):
        assert (tmp_path / "got" / rel).read_bytes() == (tmp_path / "want" / rel).read_bytes(), rel
    log.clear()
    rc, exp0 = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "ungapped"), sopt(), batch_reads=batch, device=gpu, cmd_options={"libType": "U"},
                                        validate_mappings=True, max_indel=0)
    assert rc == 0 and "rescued" not in exp0.verify_stats and "max indel" not in "".join(log)
    assert exp.verify_stats["records_out"] > exp0.verify_stats["records_out"] and exp.verify_stats["records_in"] == exp0.verify_stats["records_in"]
    assert exp.verify_stats["records_out"] - exp0.verify_stats["records_out"] == total["rescued"]


BOUNDARY_READS = (7, 8, 9, 15, 16, 17)          # a block holds 16 reads at 16 lanes a read and 8 at 32: on, before and after its edge


def _boundary_batch(n_reads=max(BOUNDARY_READS), seed=41):
    """three transcripts of about 200 bases and single-end reads of 20 - 40 bases from either strand: every read's first record is its
    true place, every second read has a second record on another transcript (it fails, but on transcript 1, a near copy of transcript
    0, where it passes at a higher cost and goes with keep_best), and every third read lacks one base in its middle (ungapped it fails
    at 0.9, with gaps it costs one edit).  The first n reads of the batch are a batch."""
    from sailfish_amd import hits as H
    rng = np.random.default_rng(seed)
    seqs = [bytes(rng.choice(old_corpus.ACGT, n)) for n in (197, 200, 211)]
    near = bytearray(seqs[0] + seqs[1][:3])                           # transcript 1: transcript 0 with every 13th base another one
    near[::13] = bytes(b"CGTA"[b"ACGT".index(b)] for b in near[::13])
    seqs[1] = bytes(near)
    reads, recs, off = [], [], [0]
    for r in range(n_reads):
        tid, n = r % 3, int(rng.integers(20, 41))
        p = int(rng.integers(0, len(seqs[tid]) - n - 1))
        read = seqs[tid][p:p + n + 1]
        read = read[:n // 2] + read[n // 2 + 1:] if r % 3 == 1 else read[:n]
        fwd = r % 4 < 2
        reads.append(read if fwd else old_corpus.revcomp(read))
        recs.append((tid, p, 0, 0, n, 0, int(fwd), 0, 0, 0))
        if r % 2:
            recs.append(((tid + 1) % 3, p if tid == 0 else int(rng.integers(0, 150)), 0, 0, n, 0, int(fwd), 0, 0, 0))
        off.append(len(recs))
    return seqs, reads, np.array(recs, dtype=H.HIT_DTYPE), np.array(off, np.uint32)


def test_last_group_next_to_a_block_boundary(gpu):
    """the group that owns r == n_reads writes cnt[n_reads]: read counts that put it at the end of a block, at the start of the next
    and beside either, for the ungapped pass and both widths of the gapped one, keep_best on and off; then the alignment of the
    survivors.  Everything equals the statements, and the inputs hold survivors, failed records and rescued ones"""
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    import test_gpu_aligng as A
    seqs, reads, recs, off = _boundary_batch()
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    seen = dict(records_out=0, failed_identity=0, rescued=0, dropped_not_best=0, jobs_traced=0)
    for n in BOUNDARY_READS:
        rd, o = reads[:n], off[:n + 1]
        h = recs[:o[-1]]
        for k in (0, 3, 8):
            for kb in (False, True):
                want = H.verify_hits_gapped_host(seqs, h, o, rd, None, 900, kb, k) if k else H.verify_hits_host(seqs, h, o, rd, None, 900, kb)
                gh, go, gs, gst = H.verify_hits(idx, h, o, rd, min_identity=0.9, keep_best=kb, max_indel=k)
                _same((*_numpy(gh, go, gs, H.GSCORE_DTYPE if k else H.SCORE_DTYPE), gst), want, (n, k, kb))
                for key in seen:
                    seen[key] += want[3].get(key, 0)
                if k:
                    pos, nm, op_off, ops, ast = H.align_hits(idx, gh, go, rd, max_indel=k)
                    want_a = H.align_hits_host(seqs, want[0], want[1], rd, None, k)
                    A._same((*A._numpy(pos, nm, op_off, ops), ast), want_a, (n, k, kb))
                    seen["jobs_traced"] += want_a[4]["jobs_traced"]
    idx.close()
    assert all(v > 0 for v in seen.values()), seen
