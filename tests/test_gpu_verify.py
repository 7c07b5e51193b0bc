"""Hit verification on the device (csrc/verify.hip: sfgpu_hits_verify; hits.verify_hits; QuasiIndex.map_reads(validate=);
validate_mappings= of mapper.quantify_reads / quantify_files) against the Python statement hits.verify_hits_host: record for record,
offsets, scores and stats over the shared corpus (tests/verify_corpus.py), the contract's errors, and end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import verify_corpus as corpus
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


def _numpy(h, o, s):
    from sailfish_amd import hits as H
    return h.cpu().numpy().view(O.HIT_DTYPE), o.cpu().numpy().view(np.uint32), s.cpu().numpy().view(H.SCORE_DTYPE)


def _same(got, want, what):
    h, o, s, st = got
    wh, wo, ws, wst = want
    assert np.array_equal(o, wo), what
    assert np.array_equal(h, wh), what
    assert np.array_equal(s, ws), what
    assert st == wst, (what, st, wst)


@pytest.mark.parametrize("name", ["pe_clean", "pe_2pc", "pe_5pc", "se_clean", "se_3pc", "se_5pc", "edges_pe", "edges_se", "long"])
def test_device_equals_the_statement(gpu, name):
    """every case of the corpus, permille 0 / 900 / 1000, keep_best on and off"""
    from sailfish_amd import hits as H
    case = corpus.cases()[name]
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    for permille, kb in corpus.OPTIONS:
        h, o, s, st = H.verify_hits(idx, d_hits, d_off, case["r1"], case["r2"], min_identity=permille / 1000, keep_best=kb)
        _same((*_numpy(h, o, s), st), corpus.expected(name, permille, kb), (name, permille, kb))
    idx.close()


def _raw(idx, s1, o1, s2, o2, n_reads, d_hits, d_off, permille, kb, out_hits, out_off, scores, n_out=True, stats=True, opts=True, index=True):
    """sfgpu_hits_verify itself -> (rc, n_out, stats)"""
    import torch
    from sailfish_amd import _lib
    o = _lib.VerifyOpts(permille, int(kb))
    st = _lib.VerifyStats()
    n = C.c_uint64(12345)
    with torch.cuda.device(idx.device):
        torch.cuda.synchronize()
        rc = _lib.lib().sfgpu_hits_verify(idx._h if index else None, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), n_reads, _lib.ptr(d_hits),
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
    name = "pe_2pc"
    case = corpus.cases()[name]
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    want = corpus.expected(name, 900, True)
    packs = []
    for reads, lead in ((case["r1"], b"xyz"), (case["r2"], b"NNNNNNN")):
        b, o = sf.mapper.pack_sequences([lead] + list(reads))
        assert any(int(x) % 16 for x in o)
        packs.append((b.to(gpu), o[1:].contiguous().to(gpu)))
    h, o, s, st = H.verify_hits(idx, d_hits, d_off, packs[0], packs[1], min_identity=0.9, keep_best=True)
    _same((*_numpy(h, o, s), st), want, "offset reads")
    # no scores wanted
    R, n = len(case["r1"]), len(case["hits"])
    out_hits, out_off = torch.zeros(n * 24, dtype=torch.uint8, device=gpu), torch.zeros(R + 1, dtype=torch.int32, device=gpu)
    rc, n_out, st = _raw(idx, *packs[0], *packs[1], R, d_hits, d_off, 900, True, out_hits, out_off, None)
    assert rc == 0 and n_out == len(want[0]) and st == want[3]
    assert np.array_equal(out_hits[: n_out * 24].cpu().numpy().view(O.HIT_DTYPE), want[0]) and np.array_equal(out_off.cpu().numpy().view(np.uint32), want[1])
    # no records at all
    none_h, none_o = torch.zeros(0, dtype=torch.uint8, device=gpu), torch.zeros(R + 1, dtype=torch.int32, device=gpu)
    h, o, s, st = H.verify_hits(idx, none_h, none_o, case["r1"], case["r2"])
    assert h.numel() == 0 and s.numel() == 0 and not o.any().item() and o.numel() == R + 1 and st == dict.fromkeys(H.VERIFY_STATS, 0)
    rc, n_out, st = _raw(idx, *packs[0], *packs[1], R, None, none_o, 900, False, None, out_off, None)
    assert rc == 0 and n_out == 0 and not out_off.any().item()
    # n_reads == 0
    one = torch.full((1,), 7, dtype=torch.int32, device=gpu)
    rc, n_out, st = _raw(idx, None, None, None, None, 0, None, None, 900, False, None, one, None)
    assert rc == 0 and n_out == 0 and one.item() == 0 and st == dict.fromkeys(H.VERIFY_STATS, 0)
    h, o, s, st = H.verify_hits(idx, none_h, none_o[:1], [], [])
    assert h.numel() == 0 and o.tolist() == [0] and st["records_in"] == 0
    idx.close()
    # nothing survives: reads that share one seed with a transcript
    rng = np.random.default_rng(32)
    seqs = corpus.clean_transcripts(rng)
    reads = corpus.planted_reads(rng, seqs, 120)
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    mh, mo = idx.map_reads(reads)
    assert mh.numel() // 24 >= len(reads)
    h, o, s, st = H.verify_hits(idx, mh, mo, reads)
    assert h.numel() == 0 and s.numel() == 0 and not o.any().item() and st["records_in"] == st["failed_identity"] == mh.numel() // 24 and st["reads_out"] == 0
    assert st == H.verify_hits_host(seqs, *sf.mapper.hits_to_numpy(mh, mo), reads, None, 900, False)[3]
    idx.close()


def test_errors(gpu):
    """tid >= M: SFGPU_ERR_RANGE naming the lowest such record, the outputs untouched; null pointers and a permille above 1000:
    SFGPU_ERR_INVALID; the Python surface raises ValueError for a min_identity outside 0 .. 1"""
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
    rc, n_out, st = _raw(idx, s1, o1, s2, o2, R, d_hits, d_off, 900, False, out_hits, out_off, scores)
    assert rc == _lib.ERR_RANGE and b"record 17 " in _lib.lib().sfgpu_last_error()
    assert all(bool((t == 0x5A).all().item()) for t in (out_hits, out_off, scores))
    with pytest.raises(_lib.SfgpuError, match="record 17 "):
        H.verify_hits(idx, d_hits, d_off, case["r1"], case["r2"])
    args = dict(idx=idx, s1=s1, o1=o1, s2=s2, o2=o2, n_reads=R, d_hits=good_hits, d_off=d_off, permille=900, kb=False, out_hits=out_hits, out_off=out_off, scores=scores)
    for change in (dict(index=False), dict(opts=False), dict(n_out=False), dict(stats=False), dict(out_off=None), dict(s1=None), dict(o1=None), dict(o2=None),
                   dict(d_off=None), dict(d_hits=None), dict(out_hits=None), dict(permille=1001), dict(s2=None, o2=None)):      # (the last: records name mate 2)
        rc, _, _ = _raw(**{**args, **change})
        assert rc == _lib.ERR_INVALID, change
    assert all(bool((t == 0x5A).all().item()) for t in (out_hits, out_off, scores))
    rc, n_out, st = _raw(**args)
    assert rc == 0 and n_out == len(corpus.expected("edges_pe", 900, False)[0])
    for mi in (-0.1, 1.2):
        with pytest.raises(ValueError):
            H.verify_hits(idx, good_hits, d_off, case["r1"], case["r2"], min_identity=mi)
        with pytest.raises(ValueError):
            sf.mapper.quantify_reads(["t"], [b"ACGT" * 20], [b"ACGT" * 10], None, "U", "unused", validate_mappings=True, min_identity=mi, device=gpu)
    idx.close()


def _noise_mix(seed=41, n_true=600, n_noise=300):
    """error-free pairs' first mates mixed with reads that share one seed with a transcript, single end"""
    rng = np.random.default_rng(seed)
    seqs = corpus.clean_transcripts(rng)
    reads = corpus.with_errors(rng, corpus.true_reads(rng, seqs, n_true, 70)[0], 0.02) + corpus.planted_reads(rng, seqs, n_noise)
    order = rng.permutation(len(reads))
    return ["tx%d" % i for i in range(len(seqs))], seqs, [reads[i] for i in order]


def test_map_reads_validate(gpu):
    """map_reads(validate=...) is verify_hits applied to the plain map_reads of the same batch, and leaves scores and stats on the
    index; without validate the call returns what it always did"""
    import torch
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    case = corpus.cases()["pe_5pc"]
    idx = _index(case, gpu)
    for r2 in (case["r2"], None):
        ph, po = idx.map_reads(case["r1"], r2)
        ph2, po2 = idx.map_reads(case["r1"], r2, validate=None)
        assert torch.equal(ph, ph2) and torch.equal(po, po2) and not hasattr(idx, "last_scores")
        for kw in ({}, dict(min_identity=0.95), dict(keep_best=True), dict(min_identity=0.8, keep_best=True)):
            wh, wo, ws, wst = H.verify_hits(idx, ph, po, case["r1"], r2, **kw)
            h, o = idx.map_reads(case["r1"], r2, validate=kw)
            assert torch.equal(h, wh) and torch.equal(o, wo) and torch.equal(idx.last_scores, ws) and idx.last_verify_stats == wst
            assert 0 < wst["records_out"] < wst["records_in"]
            del idx.last_scores, idx.last_verify_stats
        assert H.verify_hits(idx, ph, po, case["r1"], r2, min_identity=0.9)[3] == H.verify_hits(idx, ph, po, case["r1"], r2)[3]
    idx.close()


def test_quantify_with_validated_mappings(gpu, tmp_path):
    """quantify_reads / quantify_files(validate_mappings=True): quant.sf and aux/eq_classes.txt are those of quant.quantify fed the
    statement's filtered batches, and the mappings file holds exactly the lines samfile.write_sam writes for them"""
    import sailfish_amd as sf
    from sailfish_amd import quant, samfile
    names, seqs, reads = _noise_mix()
    batch = 250
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)
    log = []
    sopt = lambda: sf.SailfishOpts(dumpEq=True, jointLog=lambda lvl, msg: log.append(msg))
    for kw in (dict(min_identity=0.9, keep_best=False), dict(min_identity=0.85, keep_best=True)):
        tag = "best" if kw["keep_best"] else "all"
        permille = int(round(kw["min_identity"] * 1000))
        filtered, total = [], dict.fromkeys(sf.hits.VERIFY_STATS, 0)
        for a in range(0, len(reads), batch):
            h, o = sf.mapper.hits_to_numpy(*idx.map_reads(reads[a:a + batch]))
            fh, fo, _, st = sf.hits.verify_hits_host(seqs, h, o, reads[a:a + batch], None, permille, kw["keep_best"])
            filtered.append((fh, fo))
            for key in total:
                total[key] += st[key]
        assert total["failed_identity"] >= 300 and 0 < total["reads_out"] < total["reads_in"]
        want_dir = tmp_path / f"want_{tag}"
        rc, _ = quant.quantify(names, ref_len, iter(filtered), "U", str(want_dir), sopt(), device=gpu, cmd_options={"libType": "U"})
        assert rc == 0
        all_hits = np.concatenate([h for h, _ in filtered])
        all_off = np.concatenate([[0]] + [o[1:].astype(np.int64) + sum(len(h) for h, _ in filtered[:i]) for i, (_, o) in enumerate(filtered)]).astype(np.uint32)
        want_sam = tmp_path / f"want_{tag}.sam"
        samfile.write_sam(str(want_sam), names, ref_len, all_hits, all_off, seqs=reads)
        # from the reads
        got_dir, got_sam = tmp_path / f"reads_{tag}", tmp_path / f"reads_{tag}.sam"
        log.clear()
        rc, exp = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(got_dir), sopt(), batch_reads=batch, device=gpu, cmd_options={"libType": "U"},
                                           write_mappings=str(got_sam), validate_mappings=True, **kw)
        assert rc == 0 and exp.verify_stats == total
        assert sum(m.startswith("validated mappings") for m in log) == 1
        for rel in ("quant.sf", os.path.join("aux", "eq_classes.txt")):
            assert (got_dir / rel).read_bytes() == (want_dir / rel).read_bytes(), rel
        assert got_sam.read_bytes() == want_sam.read_bytes()
        # from files
        fa, fq = tmp_path / "transcripts.fasta", tmp_path / "reads.fastq"
        fa.write_bytes(b"".join(b">" + nm.encode() + b"\n" + s + b"\n" for nm, s in zip(names, seqs)))
        fq.write_bytes(b"".join(b"@frag.%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads)))
        samfile.write_sam(str(want_sam), names, ref_len, all_hits, all_off, seqs=reads, read_names=[b"frag.%d" % i for i in range(len(reads))])
        got_dir, got_sam = tmp_path / f"files_{tag}", tmp_path / f"files_{tag}.sam"
        rc, exp = sf.mapper.quantify_files(str(fa), str(fq), None, "U", str(got_dir), sopt(), batch_reads=batch, device=gpu, cmd_options={"libType": "U"},
                                           write_mappings=str(got_sam), validate_mappings=True, **kw)
        assert rc == 0 and exp.verify_stats == total
        for rel in ("quant.sf", os.path.join("aux", "eq_classes.txt")):
            assert (got_dir / rel).read_bytes() == (want_dir / rel).read_bytes(), rel
        assert got_sam.read_bytes() == want_sam.read_bytes()
    # the option off: the experiment says so and the output is the plain run's
    rc, exp = sf.mapper.quantify_reads(names, seqs, reads, None, "U", str(tmp_path / "plain"), sopt(), batch_reads=batch, device=gpu, cmd_options={"libType": "U"})
    assert rc == 0 and exp.verify_stats is None
    assert (tmp_path / "plain" / "quant.sf").read_bytes() != (tmp_path / "want_all" / "quant.sf").read_bytes()
    idx.close()
