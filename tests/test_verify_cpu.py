"""Hit verification without a GPU: csrc/verifyfmt.h alone (tests/verify_harness.cpp, g++ -Wall -Wextra -Werror; once more as a
stand-alone program under -fsanitize=address,undefined) against the Python statement hits.verify_hits_host -- hand-computed cases with
their expected counts written out, the shared corpus (tests/verify_corpus.py) record for record, and what the statement promises on
the restated mapper (oracle.mapper_oracle.scan_reads)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import verify_corpus as corpus
from oracle import mapper_oracle as MO
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "verify_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("vfh")), "libverify_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.vfh_job.restype = None
    L.vfh_job.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64, C.c_int64, C.c_int, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.vfh_passes.restype = C.c_int
    L.vfh_passes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
    L.vfh_code.restype = C.c_uint32
    L.vfh_code.argtypes = [C.c_uint32]
    L.vfh_verify.restype = C.c_int64
    L.vfh_verify.argtypes = [_P, _P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_int, C.c_int, _P, _P, _P, _P]
    return L


def _job(L, read, fwd, t, pos):
    """(mism, over) of one job from the harness: byte by byte, and as groups of 16 and of 3 lanes count it"""
    got = []
    for windows, lanes in ((0, 1), (1, 16), (1, 3)):
        m, o = C.c_uint64(), C.c_uint64()
        L.vfh_job(read, len(read), int(fwd), t, len(t), pos, windows, lanes, C.byref(m), C.byref(o))
        got.append((m.value, o.value))
    assert got[0] == got[1] == got[2], got
    return got[0]


def _single(t, read, fwd, pos, permille):
    """the statement on one single-end record -> (mism, over, survives)"""
    from sailfish_amd import hits as H
    rec = np.array([(0, pos, 0, 0, len(read), 0, int(fwd), 0, 0, 0)], dtype=H.HIT_DTYPE)
    h, o, s, st = H.verify_hits_host([t], rec, [0, 1], [read], None, permille, False)
    assert st["records_in"] == 1 and st["records_out"] == len(h) == int(o[1]) and st["failed_identity"] == 1 - len(h)
    m, ov = _single.harness_job(read, fwd, t, pos)
    assert bool(_single.harness.vfh_passes(len(read), m, ov, permille)) == (len(h) == 1)
    if len(h):
        assert (int(s["mism"][0]), int(s["over"][0])) == (m, ov) and int(s["mate_mism"][0]) == int(s["mate_over"][0]) == 0
    return m, ov, len(h) == 1


T = b"ACGTACGTAGCTAGCTAGGATCCATTGACCAGTTAGGCAT"            # 40 bases


def _sub(read, *at):
    """the read with the bases at `at` replaced by another base"""
    b = bytearray(read)
    for i in at:
        b[i] = {65: 67, 67: 71, 71: 84, 84: 65}[b[i]]
    return bytes(b)


def test_hand_computed_cases(built, harness):
    """the expected (mism, over, survives) of each case is written here, worked out from the rules by hand"""
    from sailfish_amd import hits as H
    _single.harness, _single.harness_job = harness, lambda *a: _job(harness, *a)
    assert [harness.vfh_code(b) for b in b"ACGTacgtNn*"] == [0, 1, 2, 3, 0, 1, 2, 3, 4, 4, 4]
    m = T[5:25]                                                       # 20 bases
    assert _single(T, m, True, 5, 900) == (0, 0, True)
    assert _single(T, m, True, 5, 1000) == (0, 0, True)
    assert _single(T, _sub(m, 0, 9, 19), True, 5, 900) == (3, 0, False)      # 17 000 < 18 000
    assert _single(T, _sub(m, 0, 9, 19), True, 5, 850) == (3, 0, True)       # 17 000 >= 17 000
    rc = corpus.revcomp(m)
    assert _single(T, rc, False, 5, 1000) == (0, 0, True)                    # the same mate on the reverse strand
    assert _single(T, corpus.revcomp(_sub(m, 0, 9, 19)), False, 5, 900) == (3, 0, False)
    assert _single(T, rc, True, 5, 900)[2] is False                          # ... does not pass as a forward mate
    assert _single(T, b"GGGG" + T[:16], True, -4, 900) == (0, 4, False)      # pos = -4: four bases in front of the transcript
    assert _single(T, b"GGGG" + T[:16], True, -4, 800) == (0, 4, True)       # 16 000 >= 16 000
    assert _single(T, b"GGGG" + T[:16], True, -4, 801) == (0, 4, False)
    assert _single(T, T[27:] + b"AAAAAAA", True, 27, 900) == (0, 7, False)   # 7 bases past the end
    assert _single(T, T[27:] + b"AAAAAAA", True, 27, 650) == (0, 7, True)
    assert _single(T, corpus.revcomp(T[27:] + b"AAAAAAA"), False, 27, 650) == (0, 7, True)
    short = b"ACGTACGTAG"
    assert _single(short, b"TT" + short + b"CC", True, -2, 900) == (0, 4, False)     # a mate longer than its transcript
    assert _single(short, b"TT" + short + b"CC", True, -2, 714) == (0, 4, True)      # 10 000 >= 9 996
    assert _single(short, b"TT" + short + b"CC", True, -2, 715) == (0, 4, False)     # 10 000 < 10 010
    assert _single(short, short, True, 40, 0) == (0, 10, True)               # wholly off the transcript; 0 >= 0
    assert _single(short, short, True, -10, 1) == (0, 10, False)
    assert _single(b"ACGTTACGTA", b"ACGNTACGTA", True, 0, 1000) == (1, 0, False)     # N in the read
    assert _single(b"ACGNTACGTA", b"ACGNTACGTA", True, 0, 1000) == (1, 0, False)     # N against N is a mismatch, not a match
    assert _single(b"ACGNTACGTA", b"ACGNTACGTA", True, 0, 900) == (1, 0, True)       # 9 000 >= 9 000
    assert _single(b"ACGNTACGTA", corpus.revcomp(b"ACGNTACGTA"), False, 0, 900) == (1, 0, True)
    assert _single(T.lower(), m, True, 5, 1000) == (0, 0, True)              # a lower-case transcript
    assert _single(T, m.lower(), True, 5, 1000) == (0, 0, True)
    # every byte value: only A C G T a c g t are bases (8 of 256 match themselves; 2 match an A; on the reverse strand 2 pair with a T)
    every = bytes(range(256))
    assert _single(every, every, True, 0, 0) == (248, 0, True)
    assert _single(b"A" * 256, every, True, 0, 0) == (254, 0, True) and _single(b"t" * 256, every[::-1], False, 0, 0) == (254, 0, True)
    assert _single(b"ACGT" * 64, b"ACGT" * 64, False, 0, 1000) == (0, 0, True)       # ACGT is its own reverse complement
    # the thresholds at 1000 * matches == permille * len, on both sides
    ten = T[:10]
    assert _single(T, _sub(ten, 4), True, 0, 900) == (1, 0, True) and _single(T, _sub(ten, 4, 5), True, 0, 900) == (2, 0, False)
    assert _single(T, _sub(m, 3, 4), True, 5, 900) == (2, 0, True) and _single(T, _sub(m, 3, 4, 5), True, 5, 900) == (3, 0, False)
    assert _single(T, ten, True, 0, 1000) == (0, 0, True) and _single(T, _sub(ten, 9), True, 0, 1000) == (1, 0, False)
    assert _single(T, _sub(ten, *range(10)), True, 0, 0) == (10, 0, True) and _single(T, b"", True, 0, 1000) == (0, 0, True)
    # a pair record where only mate 2 fails: the record falls as a whole; its orphan twin with mate 1 alone survives
    m1, m2 = T[:20], corpus.revcomp(_sub(T[20:], 1, 2, 3))
    recs = np.array([(0, 0, 20, 40, 20, 20, 1, 0, 3, 0), (0, 0, 0, 0, 20, 20, 1, 0, 1, 0), (0, 20, 0, 0, 20, 20, 0, 0, 2, 0)], dtype=H.HIT_DTYPE)
    h, o, s, st = H.verify_hits_host([T], recs, [0, 3], [m1], [m2], 900, False)
    assert o.tolist() == [0, 1] and h.tolist() == [recs[1].tolist()] and s.tolist() == [(0, 0, 0, 0)]
    assert st == dict(records_in=3, records_out=1, reads_in=1, reads_out=1, failed_identity=2, dropped_not_best=0, sum_mism=0)
    h, o, s, st = H.verify_hits_host([T], recs, [0, 3], [m1], [m2], 850, False)
    assert o.tolist() == [0, 3] and s.tolist() == [(0, 0, 3, 0), (0, 0, 0, 0), (3, 0, 0, 0)] and st["sum_mism"] == 6
    h, o, s, st = H.verify_hits_host([T], recs, [0, 3], [m1], [m2], 850, True)
    assert h.tolist() == [recs[1].tolist()] and st["dropped_not_best"] == 2 and st["failed_identity"] == 0
    with pytest.raises(ValueError, match="record 1 "):
        bad = recs.copy(); bad["tid"][1:] = 1
        H.verify_hits_host([T], bad, [0, 3], [m1], [m2], 900, False)
    for p in (-1, 1001):
        with pytest.raises(ValueError):
            H.verify_hits_host([T], recs, [0, 3], [m1], [m2], p, False)


def _run_harness(L, case, permille, keep_best, windows):
    ts, toff = corpus.packed(case["seqs"])
    tl = np.array([len(x) for x in case["seqs"]], np.uint32)
    s1, o1 = corpus.packed(case["r1"])
    s2, o2 = corpus.packed(case["r2"]) if case["r2"] is not None else (None, None)
    n = len(case["hits"])
    oh, oo, os_ = np.zeros(max(n, 1), O.HIT_DTYPE), np.zeros(len(case["off"]), np.uint32), np.zeros(max(n, 1), np.uint64)
    st = np.zeros(7, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data
    rc = L.vfh_verify(p(ts), p(toff), p(tl), len(tl), p(s1), p(o1), p(s2), p(o2), len(case["r1"]), p(case["hits"]), p(case["off"]), permille, int(keep_best),
                      windows, p(oh), p(oo), p(os_), p(st))
    return rc, oh, oo, os_, st


def test_verifyfmt_serial_equals_the_statement(built, harness):
    """over the whole corpus, for permille 0 / 900 / 1000 with and without keep_best: the harness, counting byte by byte and sixteen
    bases at a time, gives the statement's records, offsets, scores and stats"""
    from sailfish_amd import hits as H
    total = 0
    for name, case in corpus.cases().items():
        for permille, kb in corpus.OPTIONS:
            h, o, s, st = corpus.expected(name, permille, kb)
            for windows in (0, 1):
                rc, oh, oo, os_, ost = _run_harness(harness, case, permille, kb, windows)
                assert rc == len(h), (name, permille, kb, windows)
                assert np.array_equal(oo, o) and np.array_equal(oh[:rc], h) and np.array_equal(os_[:rc], s.view(np.uint64)), (name, permille, kb, windows)
                assert ost.tolist() == [st[k] for k in H.VERIFY_STATS], (name, permille, kb, windows)
            total += len(h)
    assert total > 10000
    case = dict(corpus.cases()["edges_se"])
    bad = case["hits"].copy(); bad["tid"][[7, 3, 11]] = len(case["seqs"])
    case["hits"] = bad
    assert _run_harness(harness, case, 900, False, 1)[0] == -(1 + 3)


def test_corpus_covers_its_rules(built):
    """the shapes the corpus promises, so that the comparisons above cannot pass vacuously"""
    cs = corpus.cases()
    for name in ("edges_pe", "edges_se"):
        c = cs[name]
        assert sorted(set(len(r) for r in c["r1"])) == list(corpus.EDGE_LENGTHS)
        assert set(c["hits"]["mate_status"].tolist()) == ({1, 2, 3} if c["r2"] is not None else {0})
        h, o, s, st = corpus.expected(name, 0, False)
        assert len(h) == len(c["hits"]) > 100 and int((s["over"] > 0).sum()) > 20 and int((s["mism"] > 0).sum()) > 20
        rl = np.repeat([len(r) for r in c["r1"]], np.diff(c["off"]))
        assert int(((s["over"] == rl) & (rl > 0) & (h["mate_status"] < 2)).sum()) > 3          # wholly off the transcript
        assert 0 < len(corpus.expected(name, 900, False)[0]) < len(h)
    assert any(any(int(x) % 16 for x in np.cumsum([len(r) for r in cs[n]["r1"]])) for n in cs)
    for name in ("pe_2pc", "pe_5pc", "se_3pc", "se_5pc"):
        st = corpus.expected(name, 900, False)[3]
        assert st["records_out"] > 200 and st["failed_identity"] > 0, (name, st)
        st = corpus.expected(name, 900, True)[3]
        assert st["dropped_not_best"] > 0, (name, st)
    assert int((cs["pe_2pc"]["hits"]["mate_status"] == 3).sum()) > 300
    h, o, s, st = corpus.expected("long", 900, False)
    assert o.tolist() == [0, 1, 1, 1] and 600 < s["mism"][0] < 800 and s["over"][0] == 0 and st["sum_mism"] == int(s["mism"][0])
    h, o, s, st = corpus.expected("long", 0, False)
    assert o.tolist() == [0, 1, 3, 5] and s["over"].tolist() == [0, 100, 65535, 0, 65535] and s["mism"][3] == 65535 and st["sum_mism"] > 65535 + 40000
    assert corpus.expected("long", 1000, True)[3]["records_out"] == 0


def test_harness_runs_clean_under_sanitizers(built, tmp_path):
    """the same functions as a stand-alone program built with -fsanitize=address,undefined: every case of the corpus, every text in a
    block of exactly its size, so a 16-byte load that leaves a mate or a transcript is a report"""
    exe = str(tmp_path / "verify_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DVERIFY_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    path = tmp_path / "cases.bin"
    names = list(corpus.cases())
    with open(path, "wb") as f:
        for name in names:
            for permille, kb in corpus.OPTIONS:
                f.write(corpus.blob(name, permille, kb))
    r = subprocess.run([exe, str(path)], text=True, capture_output=True)
    assert r.returncode == 0 and f"verify harness ok: {len(names) * len(corpus.OPTIONS)} cases" in r.stdout, r.stdout + r.stderr


def test_error_free_reads_keep_every_record_with_zero_scores(built):
    from sailfish_amd import hits as H
    rng = np.random.default_rng(31)
    seqs = corpus.clean_transcripts(rng)
    r1, r2 = corpus.true_reads(rng, seqs, 250)
    si = MO.build_scan_index(seqs)
    for paired in (False, True):
        hits, off = MO.scan_reads(si, r1, r2 if paired else None, s=19)
        assert np.all(np.diff(off) > 0)
        h, o, s, st = H.verify_hits_host(seqs, hits, off, r1, r2 if paired else None, 1000, False)
        assert np.array_equal(h, hits) and np.array_equal(o, off) and not s.view(np.uint16).any()
        assert st["records_out"] == st["records_in"] == len(hits) and st["reads_out"] == len(r1) and st["sum_mism"] == 0


def test_reads_sharing_one_seed_with_a_transcript_map_and_are_dropped(built):
    """random 100-base reads that carry one 25-base segment of a transcript: the mapper's scan contract reports every one of them
    (asserted: the test cannot pass vacuously), verification at 0.9 keeps none"""
    from sailfish_amd import hits as H
    rng = np.random.default_rng(32)
    seqs = corpus.clean_transcripts(rng)
    reads = corpus.planted_reads(rng, seqs, 120)
    hits, off = MO.scan_reads(MO.build_scan_index(seqs), reads, None, s=19)
    assert np.all(np.diff(off) >= 1) and len(hits) >= len(reads)
    h, o, s, st = H.verify_hits_host(seqs, hits, off, reads, None, 900, False)
    assert len(h) == 0 and not o.any() and st["reads_out"] == 0 and st["failed_identity"] == len(hits) and st["reads_in"] == len(reads)
    assert len(H.verify_hits_host(seqs, hits, off, reads, None, 0, False)[0]) == len(hits)


def test_keep_best_keeps_the_minimum_cost_records(built):
    """with keep_best every surviving record of a read has the read's minimum cost among its passing records, and a read keeps at
    least one record whenever one passed"""
    from sailfish_amd import hits as H
    dropped = 0
    for name in ("pe_5pc", "se_5pc", "se_3pc", "edges_pe"):
        c = corpus.cases()[name]
        for permille in (0, 900):
            h, o, s, st = corpus.expected(name, permille, False)
            hb, ob, sb, stb = corpus.expected(name, permille, True)
            cost = lambda x: x.view(np.uint16).reshape(-1, 4).astype(np.int64).sum(1)         # (no field saturates in these cases)
            assert s.view(np.uint16).max() < 65535
            for r in range(len(o) - 1):
                plain, best = cost(s[o[r]:o[r + 1]]), cost(sb[ob[r]:ob[r + 1]])
                assert (len(plain) > 0) == (len(best) > 0)
                if len(plain):
                    assert np.all(best == plain.min()) and len(best) == int((plain == plain.min()).sum())
                    assert np.array_equal(hb[ob[r]:ob[r + 1]], h[o[r]:o[r + 1]][plain == plain.min()])
            assert stb["dropped_not_best"] == len(h) - len(hb) and stb["reads_out"] == st["reads_out"] and stb["failed_identity"] == st["failed_identity"]
            dropped += stb["dropped_not_best"]
    assert dropped > 100


def test_python_surface_checks_its_arguments(built):
    from sailfish_amd import hits as H
    assert [H._permille(x) for x in (0, 0.9, 0.8995, 1, 0.65)] == [0, 900, 900, 1000, 650]
    for bad in (-0.001, 1.0006, 90):
        with pytest.raises(ValueError):
            H._permille(bad)
    assert H.SCORE_DTYPE.itemsize == 8 and H.SCORE_DTYPE.names == ("mism", "over", "mate_mism", "mate_over")
