"""Mate rescue on the device (csrc/rescue.hip: sfgpu_hits_rescue_mates; hits.rescue_mates; QuasiIndex.map_reads(rescue=);
rescue_mates= of mapper.quantify_reads) against the Python statement hits.rescue_mates_host: records, offsets, mism and stats over
the shared corpus (tests/rescue_corpus.py), the contract's errors, and end to end."""
import ctypes as C
import os

import numpy as np
import pytest

import rescue_corpus as corpus
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


def _numpy(h, o, m):
    return h.cpu().numpy().view(O.HIT_DTYPE), o.cpu().numpy().view(np.uint32), m.cpu().numpy().view(np.uint16)


def _same(got, want, what):
    h, o, m, st = got
    wh, wo, wm, wst = want
    assert np.array_equal(o, wo), what
    assert np.array_equal(h, wh), what
    assert np.array_equal(m, wm), what
    assert st == wst, (what, st, wst)


@pytest.mark.parametrize("name", ["strands", "clipping", "sizes", "budget", "letters", "ties", "lanes", "mates", "reads", "empty", "random_a", "random_b", "end_to_end"])
def test_device_equals_the_statement(gpu, name):
    """every case of the corpus at every (permille, window) it names"""
    from sailfish_amd import hits as H
    case = corpus.cases()[name]
    idx = _index(case, gpu)
    d_hits, d_off = _device(case, gpu)
    for permille, window in case["opts"]:
        h, o, m, st = H.rescue_mates(idx, d_hits, d_off, case["r1"], case["r2"], min_identity=permille / 1000, window=window)
        _same((*_numpy(h, o, m), st), corpus.expected(name, permille, window), (name, permille, window))
    idx.close()


def _raw(idx, s1, o1, s2, o2, n_reads, d_hits, d_off, permille, window, out_hits, out_off, mism, n_out=True, stats=True, opts=True, index=True):
    """sfgpu_hits_rescue_mates itself -> (rc, n_out, stats)"""
    import torch
    from sailfish_amd import _lib
    o = _lib.RescueOpts(permille, window)
    st = _lib.RescueStats()
    n = C.c_uint64(12345)
    with torch.cuda.device(idx.device):
        torch.cuda.synchronize()
        rc = _lib.lib().sfgpu_hits_rescue_mates(idx._h if index else None, _lib.ptr(s1), _lib.ptr(o1), _lib.ptr(s2), _lib.ptr(o2), n_reads, _lib.ptr(d_hits),
                                                _lib.ptr(d_off), C.byref(o) if opts else None, _lib.ptr(out_hits), _lib.ptr(out_off), _lib.ptr(mism),
                                                C.byref(n) if n_out else None, C.byref(st) if stats else None, _lib.current_stream_ptr())
        torch.cuda.synchronize()
    return rc, n.value, st.as_dict()


def test_errors_and_shapes_of_the_contract(gpu):
    """tid >= M: SFGPU_ERR_RANGE naming the lowest such record, the outputs untouched; a single-end batch, a permille above 1000, a
    window outside 1 .. 2^20 and null pointers: SFGPU_ERR_INVALID, the outputs untouched; d_mism_out == NULL; n_reads == 0"""
    import torch
    import sailfish_amd as sf
    from sailfish_amd import _lib
    from sailfish_amd import hits as H
    case, bad = corpus.cases()["reads"], corpus.bad_tid_case()
    idx = _index(case, gpu)
    d_hits, d_off = _device(bad, gpu)
    good_hits, _ = _device(case, gpu)
    s1, o1 = (t.to(gpu) for t in sf.mapper.pack_sequences(case["r1"]))
    s2, o2 = (t.to(gpu) for t in sf.mapper.pack_sequences(case["r2"]))
    R, n = len(case["r1"]), len(case["hits"])
    out_hits, out_off, mism = (torch.full((k,), 0x5A, dtype=torch.uint8, device=gpu) for k in (n * 24, (R + 1) * 4, n * 2))
    rc, n_out, st = _raw(idx, s1, o1, s2, o2, R, d_hits, d_off, 900, 500, out_hits, out_off, mism)
    assert rc == _lib.ERR_RANGE and b"record 4 " in _lib.lib().sfgpu_last_error()
    assert all(bool((t == 0x5A).all().item()) for t in (out_hits, out_off, mism))
    with pytest.raises(_lib.SfgpuError, match="record 4 "):
        H.rescue_mates(idx, d_hits, d_off, case["r1"], case["r2"])
    args = dict(idx=idx, s1=s1, o1=o1, s2=s2, o2=o2, n_reads=R, d_hits=good_hits, d_off=d_off, permille=900, window=500, out_hits=out_hits, out_off=out_off, mism=mism)
    for change in (dict(s2=None, o2=None), dict(s2=None), dict(o2=None), dict(permille=1001), dict(window=0), dict(window=(1 << 20) + 1), dict(index=False), dict(opts=False),
                   dict(n_out=False), dict(stats=False), dict(out_off=None), dict(s1=None), dict(o1=None), dict(d_off=None), dict(d_hits=None), dict(out_hits=None)):
        rc, _, _ = _raw(**{**args, **change})
        assert rc == _lib.ERR_INVALID, change
    assert all(bool((t == 0x5A).all().item()) for t in (out_hits, out_off, mism))
    with pytest.raises(ValueError):
        H.rescue_mates(idx, good_hits, d_off, case["r1"], None)
    wh, wo, wm, wst = corpus.expected("reads", 900, 500)
    rc, n_out, st = _raw(**{**args, "window": 1 << 20, "permille": 1000})
    assert rc == 0 and st == corpus.expected("reads", 1000, 500)[3]          # (the transcripts are shorter than either window)
    mism.fill_(0x5A)
    rc, n_out, st = _raw(**{**args, "mism": None})                           # no mism wanted
    assert rc == 0 and n_out == len(wh) and st == wst and bool((mism == 0x5A).all().item())
    assert np.array_equal(out_hits[: n_out * 24].cpu().numpy().view(O.HIT_DTYPE), wh) and np.array_equal(out_off.cpu().numpy().view(np.uint32), wo)
    one = torch.full((1,), 7, dtype=torch.int32, device=gpu)                 # n_reads == 0
    rc, n_out, st = _raw(idx, None, None, s2, o2, 0, None, None, 900, 500, None, one, None)
    assert rc == 0 and n_out == 0 and one.item() == 0 and st == dict.fromkeys(H.RESCUE_STATS, 0)
    none_h, none_o = torch.zeros(0, dtype=torch.uint8, device=gpu), torch.zeros(R + 1, dtype=torch.int32, device=gpu)      # reads without any record
    h, o, m, st = H.rescue_mates(idx, none_h, none_o, case["r1"], case["r2"])
    assert h.numel() == 0 and m.numel() == 0 and not o.any().item() and o.numel() == R + 1 and st == dict.fromkeys(H.RESCUE_STATS, 0)
    idx.close()


def test_map_reads_rescue(gpu):
    """map_reads(rescue=...) on the end-to-end reads is the device mapper's own output put through the statement, and leaves the
    pass's stats on the index; without the keyword the call returns what it always did"""
    import torch
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    names, seqs, r1, r2, src = corpus.end_to_end()
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ph, po = idx.map_reads(r1, r2)
    ph2, po2 = idx.map_reads(r1, r2, rescue=None)
    assert torch.equal(ph, ph2) and torch.equal(po, po2) and not hasattr(idx, "last_rescue_stats")
    mh, mo = sf.mapper.hits_to_numpy(ph, po)
    for kw, permille, window in (({}, 900, 1000), (dict(min_identity=0.95, window=400), 950, 400)):
        wh, wo, wm, wst = H.rescue_mates_host(seqs, mh, mo, r1, r2, permille, window)
        h, o = idx.map_reads(r1, r2, rescue=kw)
        assert np.array_equal(h.cpu().numpy().view(O.HIT_DTYPE), wh) and np.array_equal(o.cpu().numpy().view(np.uint32), wo)
        assert idx.last_rescue_stats == wst and np.array_equal(idx.last_rescue_mism.cpu().numpy().view(np.uint16), wm)
        print("map_reads(rescue=%r):" % (kw,), wst)
        assert wst["reads_rescued"] >= (10 if not kw else 1)                 # (the defaults: the figures of tests/test_rescue_cpu.py's end-to-end test)
    with pytest.raises(ValueError):
        idx.map_reads(r1, None, rescue={})
    idx.close()


def test_quantify_with_rescued_mates(gpu, tmp_path):
    """quantify_reads(rescue_mates=True): the mappings file is samfile._sam_text of the host-rescued records, `rescue_stats` the
    statement's sums, and numMappedFragments exceeds the plain run's by reads_rescued (allow_orphans at its default); rescue_mates=False
    writes the files of a run that omits the keyword; with validate_mappings=True no rescued record fails on its placed mate"""
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    from sailfish_amd import samfile
    names, seqs, r1, r2, src = corpus.end_to_end()
    idx = sf.mapper.QuasiIndex(seqs, device=gpu)
    ref_len = idx.ref_len.cpu().numpy().view(np.uint32)
    mh, mo = sf.mapper.hits_to_numpy(*idx.map_reads(r1, r2))
    idx.close()
    wh, wo, wm, wst = H.rescue_mates_host(seqs, mh, mo, r1, r2, 900, 1000)
    assert wst["reads_rescued"] >= 10
    log = []
    sopt = lambda: sf.SailfishOpts(dumpEq=True, jointLog=lambda lvl, msg: log.append(msg))
    run = lambda tag, **kw: sf.mapper.quantify_reads(names, seqs, r1, r2, "IU", str(tmp_path / tag), sopt(), device=gpu, cmd_options={"libType": "IU"},
                                                     write_mappings=str(tmp_path / (tag + ".sam")), **kw)
    rc, exp = run("rescued", rescue_mates=True)
    assert rc == 0 and exp.rescue_stats == wst and sum(m.startswith("rescued mates") for m in log) == 1
    assert (tmp_path / "rescued.sam").read_bytes() == samfile._sam_text(names, ref_len, wh, wo, None, list(zip(r1, r2)))
    log.clear()
    rc, plain = run("plain")
    assert rc == 0 and plain.rescue_stats is None and not any(m.startswith("rescued mates") for m in log)
    assert exp.numMappedFragments() == plain.numMappedFragments() + wst["reads_rescued"]
    assert (tmp_path / "plain.sam").read_bytes() == samfile._sam_text(names, ref_len, mh, mo, None, list(zip(r1, r2)))
    rc, off = run("off", rescue_mates=False)
    assert rc == 0 and off.rescue_stats is None
    for rel in ("off.sam", os.path.join("off", "quant.sf"), os.path.join("off", "aux", "eq_classes.txt")):
        assert (tmp_path / rel).read_bytes() == (tmp_path / rel.replace("off", "plain", 1)).read_bytes(), rel
    assert (tmp_path / "rescued" / "quant.sf").read_bytes() != (tmp_path / "plain" / "quant.sf").read_bytes()
    # a narrower window from the keyword, and from sopt.maxFragLen
    w300 = H.rescue_mates_host(seqs, mh, mo, r1, r2, 900, 300)[3]
    rc, exp = run("w300", rescue_mates=True, rescue_window=300)
    assert rc == 0 and exp.rescue_stats == w300 and w300["candidates"] < wst["candidates"]
    # validated at the same identity: the placed mate never fails, so what fails are anchors (and records the pass left alone)
    rc, exp = run("validated", rescue_mates=True, validate_mappings=True, min_identity=0.9)
    assert rc == 0 and exp.rescue_stats == wst
    _, _, score, _ = H.verify_hits_host(seqs, wh, wo, r1, r2, 0, False)      # permille 0 keeps every record: its scores
    failed = 0
    for r in range(len(r1)):
        orphans = {(int(v["tid"]), int(v["pos"]), int(v["fwd"])) for v in mh[mo[r]:mo[r + 1]] if v["mate_status"] == 1}
        was_orphan = mo[r + 1] > mo[r] and all(s in (1, 2) for s in mh[mo[r]:mo[r + 1]]["mate_status"].tolist())
        for i in range(wo[r], wo[r + 1]):
            v, s = wh[i], score[i]
            jobs = [(len(r2[r]) if v["mate_status"] == 2 else len(r1[r]), int(s["mism"]), int(s["over"]))]
            if v["mate_status"] == 3:
                jobs.append((len(r2[r]), int(s["mate_mism"]), int(s["mate_over"])))
            fails = [1000 * (n - mm - ov) < 900 * n for n, mm, ov in jobs]
            if v["mate_status"] == 3 and was_orphan:                         # a rescued pair: the placed mate is the one its orphan did not place
                placed = 1 if (int(v["tid"]), int(v["pos"]), int(v["fwd"])) in orphans else 0
                assert not fails[placed] and jobs[placed][2] == 0 and jobs[placed][1] == int(wm[i]), (r, i)
                failed += fails[1 - placed]
            else:
                failed += any(fails)
    assert exp.verify_stats["failed_identity"] == failed and exp.verify_stats["records_in"] == len(wh)
