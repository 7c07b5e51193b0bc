"""Mate rescue without a GPU: csrc/rescuefmt.h alone (tests/rescue_harness.cpp, g++ -Wall -Wextra -Werror; once more as a
stand-alone program under -fsanitize=address,undefined) -- byte by byte and as the kernel's wavefront searches -- against the Python
statement hits.rescue_mates_host over the shared corpus (tests/rescue_corpus.py); the statement itself against a brute-force judge
written from the rule's text; hand-computed outcomes of the corpus' named cases; the end-to-end data on the restated mapper
(oracle.mapper_oracle.scan_reads); and the ValueErrors of the Python surface."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rescue_corpus as corpus
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "rescue_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "tests")]
_P = C.c_void_p
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("rsh")), "librescue_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.rsh_window.restype = C.c_uint64
    L.rsh_window.argtypes = [C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.rsh_budget.restype = C.c_int64
    L.rsh_budget.argtypes = [C.c_uint64, C.c_uint32]
    L.rsh_job.restype = C.c_uint64
    L.rsh_job.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_int]
    L.rsh_rescue.restype = C.c_int64
    L.rsh_rescue.argtypes = [_P, _P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_uint32, C.c_int, _P, _P, _P, _P]
    return L


def _window(L, p, la, lb, tlen, f, W):
    lo, hi = C.c_int64(), C.c_int64()
    n = L.rsh_window(p, la, lb, tlen, f, W, C.byref(lo), C.byref(hi))
    return (n, lo.value, hi.value) if n else (0, None, None)


def test_hand_computed_windows_budgets_and_jobs(built, harness):
    """the expected values are written here, worked out from the rule by hand"""
    L = harness
    assert _window(L, 100, 40, 50, 600, 1, 400) == (351, 100, 450)         # forward anchor: x >= p, x + lb <= p + W
    assert _window(L, 400, 40, 50, 600, 0, 400) == (351, 40, 390)          # reverse anchor: x + lb <= p + la, x >= p + la - W
    assert _window(L, 30, 40, 50, 500, 0, 300) == (21, 0, 20)              # clipped by the start
    assert _window(L, 380, 40, 50, 500, 1, 300) == (71, 380, 450)          # ... by the end
    assert _window(L, -5, 40, 50, 500, 1, 60) == (6, 0, 5) and _window(L, -300, 40, 50, 500, 1, 200)[0] == 0
    assert _window(L, 480, 40, 50, 500, 0, 100) == (31, 420, 450) and _window(L, 900, 40, 50, 500, 0, 200)[0] == 0
    assert _window(L, 100, 40, 50, 600, 1, 50) == (1, 100, 100) and _window(L, 100, 40, 50, 600, 1, 49)[0] == 0
    assert _window(L, 0, 20, 60, 60, 1, 1000) == (1, 0, 0) and _window(L, 0, 20, 61, 60, 1, 1000)[0] == 0 and _window(L, 0, 20, 0, 60, 1, 1000)[0] == 0
    assert _window(L, 0, 20, 65535, 70000, 1, 1 << 20)[0] == 70000 - 65535 + 1 and _window(L, 0, 20, 65536, 70000, 1, 1 << 20)[0] == 0
    assert _window(L, 0, 65536, 20, 70000, 1, 1 << 20)[0] == 0 and _window(L, 0, 0, 20, 100, 0, 50) == (0, None, None)
    assert _window(L, 0, 0, 20, 100, 1, 1 << 20) == (81, 0, 80)
    assert [L.rsh_budget(50, p) for p in (900, 881, 880, 1000, 0)] == [5, 5, 6, 0, 50] and L.rsh_budget(19, 900) == 1 and L.rsh_budget(0, 0) == 0
    t = b"GATTACAGATTACACCCGGGTTTAAAGATTACA"                              # GATTACA at 0, 7 and 26
    for lanes in (0, 1):
        job = lambda m, mfwd, lo, hi, p: L.rsh_job(m, len(m), mfwd, t, len(t), lo, hi, p, lanes)
        assert job(b"GATTACA", 1, 0, 26, 1000) == 0 << 32 | 0              # three exact copies: the lowest
        assert job(b"GATTACA", 1, 1, 26, 1000) == 7 and job(b"GATTACA", 1, 8, 26, 1000) == 26 and job(b"GATTACA", 1, 8, 25, 1000) == NONE
        assert job(b"TGTAATC", 0, 0, 26, 1000) == 0                        # the reverse complement, read downwards
        assert job(b"GATTACC", 1, 0, 26, 1000) == NONE and job(b"GATTACC", 1, 0, 26, 850) == 1 << 32 | 0      # 6 000 >= 5 950
        assert job(b"GATTACC", 1, 0, 26, 858) == NONE                      # 6 000 < 6 006
        assert job(b"CATTACACC", 1, 0, 24, 0) == 1 << 32 | 7               # a later, better placement (0: 3 mismatches)
        assert job(b"GATNACA", 1, 0, 26, 850) == 1 << 32 | 0 and job(b"gattaca", 1, 5, 26, 1000) == 7
        assert job(b"NNNNNNN", 1, 0, 26, 0) == 7 << 32 | 0 and job(b"", 1, 0, 26, 0) == 0


def _run_harness(L, case, permille, window, lanes):
    ts, toff = corpus.packed(case["seqs"])
    tl = np.array([len(x) for x in case["seqs"]], np.uint32)
    s1, o1 = corpus.packed(case["r1"])
    s2, o2 = corpus.packed(case["r2"])
    n = len(case["hits"])
    oh, oo, om = np.zeros(max(n, 1), O.HIT_DTYPE), np.zeros(len(case["off"]), np.uint32), np.zeros(max(n, 1), np.uint16)
    st = np.zeros(8, np.uint64)
    p = lambda a: a.ctypes.data
    rc = L.rsh_rescue(p(ts), p(toff), p(tl), len(tl), p(s1), p(o1), p(s2), p(o2), len(case["r1"]), p(case["hits"]), p(case["off"]), permille, window, lanes,
                      p(oh), p(oo), p(om), p(st))
    return rc, oh, oo, om, st


def test_rescuefmt_both_forms_equal_the_statement(built, harness):
    """over the whole corpus at every (permille, window) a case names: the header, searching byte by byte and as the kernel's
    wavefront does, gives the statement's records, offsets, mism and stats"""
    from sailfish_amd import hits as H
    assert H.RESCUE_STATS == corpus.STATS
    rescued = 0
    for name, permille, window in corpus.runs():
        h, o, m, st = corpus.expected(name, permille, window)
        for lanes in (0, 1):
            rc, oh, oo, om, ost = _run_harness(harness, corpus.cases()[name], permille, window, lanes)
            what = (name, permille, window, lanes)
            assert rc == len(h), what
            assert np.array_equal(oo, o) and np.array_equal(oh[:rc], h) and np.array_equal(om[:rc], m), what
            assert ost.tolist() == [st[k] for k in H.RESCUE_STATS], what
        rescued += st["records_rescued"]
    assert rescued > 1000
    bad = corpus.bad_tid_case()
    assert _run_harness(harness, bad, 900, 500, 1)[0] == -(1 + 4)
    with pytest.raises(ValueError, match="record 4 "):
        H.rescue_mates_host(bad["seqs"], bad["hits"], bad["off"], bad["r1"], bad["r2"], 900, 500)
    c = corpus.cases()["reads"]
    with pytest.raises(ValueError, match="single-end"):
        H.rescue_mates_host(c["seqs"], c["hits"], c["off"], c["r1"], None, 900, 500)
    for p, w in ((1001, 500), (-1, 500), (900, 0), (900, (1 << 20) + 1), (900, 10.5)):
        with pytest.raises(ValueError):
            H.rescue_mates_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], p, w)


CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


def _judge_job(t, mate, f, p, la, W, permille):
    """from the rule's text: every integer x on the transcript is tried against the window's inequalities and scored column by column
    -> (candidates, the placement (mism, x) or None)"""
    lb = len(mate)
    if lb == 0 or lb > len(t) or lb > 65535 or la > 65535:
        return 0, None
    tc = np.array([CODE.get(c, 4) for c in t], np.int64)
    mc = [CODE.get(c, 4) for c in mate]
    if f == 1:                                                       # the missing mate is on the reverse strand: complemented, read backwards
        mc = [c if c == 4 else 3 - c for c in reversed(mc)]
    mc = np.array(mc, np.int64)
    n, best = 0, None
    for x in range(0, len(t) - lb + 1):
        inside = (x >= p and x + lb <= p + W) if f == 1 else (x + lb <= p + la and x >= p + la - W)
        if not inside:
            continue
        n += 1
        col = tc[x:x + lb]
        mism = int(((col == 4) | (mc == 4) | (col != mc)).sum())
        if 1000 * (lb - mism) >= permille * lb and (best is None or mism < best[0]):
            best = (mism, x)
    return n, best


def test_the_statement_against_a_brute_force_judge(built):
    """for every output pair the mate at its position has the recorded count, no candidate of the window has fewer, and none with as
    many lies lower; every eligible read that kept its orphans has no passing candidate; everything else passes through"""
    placed_total = kept_total = 0
    for name, permille, W in corpus.runs():
        if name in ("lanes", "mates") and permille == 0:
            continue                                                 # (the widest windows at every mate: the judge is slow; their other runs are judged)
        c = corpus.cases()[name]
        h, o, m, st = corpus.expected(name, permille, W)
        want_stats = dict.fromkeys(corpus.STATS, 0)
        for r in range(len(c["r1"])):
            recs = c["hits"][c["off"][r]:c["off"][r + 1]]
            outs, om = h[o[r]:o[r + 1]], m[o[r]:o[r + 1]]
            what = (name, permille, W, r)
            if not len(recs) or not all(int(s) in (1, 2) for s in recs["mate_status"]):
                assert np.array_equal(outs, recs) and not om.any(), what
                continue
            want_stats["reads_eligible"] += 1
            want_stats["records_orphan"] += len(recs)
            pairs = []
            for n, rec in enumerate(recs):
                st_, f, p, tid = int(rec["mate_status"]), int(rec["fwd"] != 0), int(rec["pos"]), int(rec["tid"])
                anchor, mate = (c["r1"][r], c["r2"][r]) if st_ == 1 else (c["r2"][r], c["r1"][r])
                ncand, best = _judge_job(c["seqs"][tid], mate, f, p, len(anchor), W, permille)
                want_stats["jobs_with_candidates"] += ncand > 0
                want_stats["candidates"] += ncand
                if best is None:
                    continue
                mism, x = best
                frag = max(p + len(anchor), x + len(mate)) - min(p, x)
                l1, l2 = len(c["r1"][r]), len(c["r2"][r])
                pair = (tid, p, x, frag, l1, l2, f, 1 - f, 3, 0) if st_ == 1 else (tid, x, p, frag, l1, l2, 1 - f, f, 3, 0)
                pairs.append(((tid, pair[6], n), pair, mism))
            if not pairs:
                assert np.array_equal(outs, recs) and not om.any(), what
                kept_total += 1
                continue
            pairs.sort(key=lambda v: v[0])
            assert outs.tolist() == [v[1] for v in pairs] and om.tolist() == [min(v[2], 65535) for v in pairs], what
            placed_total += len(pairs)
            want_stats["reads_rescued"] += 1
            want_stats["records_rescued"] += len(pairs)
            want_stats["records_dropped"] += len(recs) - len(pairs)
            want_stats["sum_mism"] += sum(v[2] for v in pairs)
        assert st == want_stats, (name, permille, W)
        assert len(o) == len(c["r1"]) + 1 and o[0] == 0 and len(h) == o[-1] <= len(c["hits"])
    assert placed_total > 500 and kept_total > 100


def _out(name, permille, W, r):
    """read r's output records and mism"""
    h, o, m, _ = corpus.expected(name, permille, W)
    return h[o[r]:o[r + 1]], m[o[r]:o[r + 1]].tolist()


def test_corpus_cases_behave_as_they_are_named(built):
    """the outcome each named case is there for, so that the comparisons cannot pass vacuously"""
    paired = lambda name, p, W, r: _out(name, p, W, r)[0]["mate_status"].tolist() == [3]
    # the four combinations of anchor strand and status
    h, o, m, st = corpus.expected("strands", 900, 400)
    assert h.tolist() == [(0, 100, 330, 280, 40, 50, 1, 0, 3, 0), (0, 400, 150, 290, 40, 50, 0, 1, 3, 0),          # status 1: forward anchor, reverse anchor
                          (0, 330, 100, 280, 50, 40, 0, 1, 3, 0), (0, 150, 400, 290, 50, 40, 1, 0, 3, 0)] and m.tolist() == [1, 1, 1, 1]      # status 2
    assert st == dict(reads_eligible=4, records_orphan=4, jobs_with_candidates=4, candidates=4 * 351, reads_rescued=4, records_rescued=4, records_dropped=0, sum_mism=4)
    assert corpus.expected("strands", 1000, 400)[3]["reads_rescued"] == 0
    # clipping: reads 0 .. 12 as the corpus lists them
    got = [paired("clipping", 1000, 200, r) for r in range(13)]
    assert got == [True, True, True, False, True, False, True, True, True, True, True, False, False]
    assert [paired("clipping", 1000, 199, r) for r in (6, 7)] == [False, False] and [paired("clipping", 1000, 49, r) for r in (2, 8)] == [False, False]
    assert [paired("clipping", 1000, 50, r) for r in (2, 8, 9)] == [True, True, False] and corpus.expected("clipping", 1000, 49)[3]["jobs_with_candidates"] == 0
    assert _out("clipping", 1000, 200, 0)[0]["mate_pos"][0] == 0 and _out("clipping", 1000, 200, 1)[0]["pos"][0] == 450
    assert _out("clipping", 1000, 200, 9)[0].tolist() == [(0, -5, 0, 55, 40, 50, 1, 0, 3, 0)]      # frag: 50 - (-5)
    assert _out("clipping", 1000, 200, 10)[0].tolist() == [(0, 450, 480, 70, 50, 40, 1, 0, 3, 0)]
    # sizes
    got = [paired("sizes", 900, 1000, r) for r in range(7)]
    assert got == [True, False, False, False, True, True, False] and paired("sizes", 0, 1000, 6) and _out("sizes", 900, 1000, 0)[1] == [1]
    # the budget: lb = 50 passes with up to 5 mismatches at 900 and 881, 6 at 880, none at 1000
    ks = (0, 1, 4, 5, 6, 10)
    for permille, most in ((900, 5), (881, 5), (880, 6), (1000, 0), (0, 50)):
        for i, k in enumerate(ks):
            for r in (2 * i, 2 * i + 1):
                assert paired("budget", permille, 300, r) == (k <= most), (permille, k, r)
                assert k > most or _out("budget", permille, 300, r)[1] == [k] or permille == 0
    assert [paired("budget", 900, 300, r) for r in (12, 13)] == [True, False]
    # letters
    assert [paired("letters", p, 300, 0) for p in (900, 940, 960)] == [True, True, False] and _out("letters", 900, 300, 0)[1] == [3]
    assert _out("letters", 900, 300, 1)[1] == [2] and _out("letters", 900, 300, 2)[1] == [1] and _out("letters", 900, 300, 3)[1] == [0]
    assert not paired("letters", 900, 300, 4) and _out("letters", 0, 300, 4)[1] == [50] and _out("letters", 0, 300, 4)[0]["mate_pos"][0] == 100
    # ties
    x = lambda name, p, W, r, field="mate_pos": int(_out(name, p, W, r)[0][field][0])
    assert x("ties", 1000, 2000, 0) == 100 and x("ties", 1000, 2000, 1, "pos") == 100 and x("ties", 900, 250, 0) == 100
    assert x("ties", 900, 2000, 2) == 201 and _out("ties", 900, 2000, 2)[1] == [0] and x("ties", 900, 2000, 3) == 201
    assert x("ties", 1000, 2000, 4) == 10 and x("ties", 1000, 2000, 5) == 0 and x("ties", 900, 2000, 6) == 10 and _out("ties", 900, 2000, 6)[1] == [1]
    assert x("ties", 1000, 2000, 7) == 30 and not paired("ties", 1000, 2000, 6)
    # lanes: the planted candidate is the window's last (forward) or first (reverse); found exactly from the window that reaches it
    c = corpus.cases()["lanes"]
    windows = [w for _, w in c["opts"][:-1]]
    for i, w in enumerate(windows):
        for W in windows:
            assert paired("lanes", 950, W, 2 * i) == (W >= w) and paired("lanes", 950, W, 2 * i + 1) == (W >= w), (w, W)
    assert sorted(set(w - 49 for w in windows)) == [63, 64, 65, 128, 1023, 1024, 1025, 1088, 2048, 2049]
    # mates on either side of the packed form's bound, and window = 2^20
    lens = [len(r) for r in corpus.cases()["mates"]["r2"][:10:2]]
    assert lens == [511, 512, 513, 528, 1200] and all(paired("mates", 900, 2500, r) for r in range(19))
    assert [paired("mates", 990, 1 << 20, r) for r in range(10, 19)] == [False] * 6 + [True] * 3      # one mismatch: 990 allows it from 100 bases on
    assert _out("mates", 900, 2500, 4)[1] == [len(range(5, 513, 97))] and _out("mates", 900, 2500, 9)[1] == [len(range(0, 1200, 61))]
    # what a read's records become
    h, o, m, st = corpus.expected("reads", 900, 500)
    assert np.diff(o).tolist() == [1, 0, 2, 2, 3, 1, 4, 2, 2, 1] and st["records_dropped"] == 2 and st["reads_eligible"] == 6 and st["reads_rescued"] == 5
    assert h[o[2]:o[3]].tolist() == [(0, 300, 200, 140, 40, 40, 0, 1, 3, 0), (0, 100, 400, 340, 40, 40, 1, 0, 3, 0)]
    assert h[o[4]:o[5]]["pos"].tolist() == [100, 70, 101] and h[o[4]:o[5]]["frag_len"].tolist() == [340, 370, 339]
    assert [(int(v["tid"]), int(v["fwd"]), int(v["pos"]), int(v["mate_pos"])) for v in h[o[6]:o[7]]] == [(0, 0, 300, 200), (0, 1, 100, 400), (0, 1, 100, 400), (1, 0, 300, 200)]
    assert np.array_equal(h[o[7]:o[8]], corpus.cases()["reads"]["hits"][15:17]) and h[o[9]:o[10]].tolist() == [(0, 100, 400, 340, 40, 40, 1, 0, 3, 0)]
    assert corpus.expected("reads", 900, 320)[3]["reads_rescued"] < 5
    h, o, m, st = corpus.expected("empty", 900, 1000)
    assert len(h) == 0 and o.tolist() == [0] and st == dict.fromkeys(corpus.STATS, 0)


def test_harness_runs_clean_under_sanitizers(built, tmp_path):
    """the same functions as a stand-alone program built with -fsanitize=address,undefined: every run of the corpus, every text in a
    block of exactly its size, so a 16-byte load that leaves a mate or a transcript is a report"""
    exe = str(tmp_path / "rescue_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRESCUE_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    path = tmp_path / "cases.bin"
    runs = corpus.runs()
    with open(path, "wb") as f:
        for name, permille, window in runs:
            f.write(corpus.blob(name, permille, window))
    r = subprocess.run([exe, str(path)], text=True, capture_output=True)
    assert r.returncode == 0 and f"rescue harness ok: {len(runs)} cases" in r.stdout, r.stdout + r.stderr


def test_end_to_end_reads_are_orphaned_and_rescued(built):
    """the spliced transcriptome's 400 pairs of 2 x 50 bases at 2 % substitutions, mapped by the restated scan contract: at least 10
    reads are orphan-only and at least 10 are rescued, each onto its source transcript -- the GPU test cannot pass on nothing"""
    names, seqs, r1, r2, src = corpus.end_to_end()
    c = corpus.cases()["end_to_end"]
    h, o, m, st = corpus.expected("end_to_end", *corpus.E2E_OPTS)
    print("end to end:", st)
    assert st["reads_eligible"] >= 10 and st["reads_rescued"] >= 10
    rescued = 0
    for r in range(len(r1)):
        recs, outs = c["hits"][c["off"][r]:c["off"][r + 1]], h[o[r]:o[r + 1]]
        if len(recs) and all(s in (1, 2) for s in recs["mate_status"].tolist()) and len(outs) and outs["mate_status"][0] == 3:
            rescued += 1
            assert src[r] in outs["tid"].tolist() and src[r] in recs["tid"].tolist(), r
    assert rescued == st["reads_rescued"]


def test_python_surface_raises_before_anything_is_indexed(built, monkeypatch):
    import sailfish_amd as sf
    from sailfish_amd import hits as H

    def no_index(*a, **k):
        raise AssertionError("indexed before the options were checked")
    monkeypatch.setattr(sf.mapper, "QuasiIndex", no_index)
    t, r = [b"ACGT" * 30], [b"ACGT" * 10]
    for kw, lib, r2 in ((dict(rescue_mates=True), "U", None), (dict(rescue_mates=True), "IU", None), (dict(rescue_mates=True), "OU", r), (dict(rescue_mates=True), "MSF", r),
                        (dict(rescue_mates=True, rescue_window=0), "IU", r), (dict(rescue_mates=True, rescue_window=(1 << 20) + 1), "ISF", r),
                        (dict(rescue_mates=True, min_identity=1.5), "ISR", r)):
        with pytest.raises(ValueError):
            sf.mapper.quantify_reads(["t"], t, r, r2, lib, "unused", **kw)
        with pytest.raises(ValueError):
            sf.mapper.quantify_files("unused.fa", "unused_1.fq", None if r2 is None else "unused_2.fq", lib, "unused", **kw)
    for lib in ("IU", "ISF", "ISR", (1, H.TOWARD, H.U)):                 # ... and these pass the checks: the index is the next thing asked for
        with pytest.raises(AssertionError, match="indexed"):
            sf.mapper.quantify_reads(["t"], t, r, r, lib, "unused", rescue_mates=True, rescue_window=300)
    run = sf.mapper._MappingsRun(True, None, "sam", False, False, False, 0.9, False, 0, False, False, None, False, True, None, "IU", sf.SailfishOpts(maxFragLen=800))
    assert run.rescue == dict(min_identity=0.9, window=800) and run.stats["rescue"] == dict.fromkeys(H.RESCUE_STATS, 0)
    assert sf.mapper._MappingsRun(True, None, "sam", False, False, False, 0.9, False, 0, False, False, None, False).rescue is None
    with pytest.raises(ValueError):
        H.rescue_mates(None, None, None, r, None)
    with pytest.raises(ValueError):
        H.rescue_mates(None, None, None, r, r, window=0)
