"""Gapped hit verification without a GPU: csrc/verifygfmt.h alone (tests/verifyg_harness.cpp, g++ -Wall -Wextra -Werror; once more as a
stand-alone program under -fsanitize=address,undefined) against the Python statement hits.gapped_edits_host /
hits.verify_hits_gapped_host over the shared corpus (tests/verifyg_corpus.py), hand-computed jobs, and what the statement promises:
k = 0 is the ungapped pass, edits never rise with k, edits <= mism + over, and a full-matrix DP restricted to the band agrees."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import verify_corpus as old_corpus
import verifyg_corpus as corpus
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "verifyg_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p
T = corpus.T


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("vgh")), "libverifyg_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.vgh_job.restype = C.c_uint64
    L.vgh_job.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_char_p, C.c_uint64, C.c_int64, C.c_uint32, C.c_int, C.c_uint64]
    L.vgh_verify.restype = C.c_int64
    L.vgh_verify.argtypes = [_P, _P, _P, C.c_uint64, _P, _P, _P, _P, C.c_uint32, _P, _P, C.c_uint32, C.c_int, C.c_uint32, C.c_int, _P, _P, _P, _P]
    return L


def _single(t, read, fwd, pos, k):
    """the statement on one single-end job -> (edits, mism + over)"""
    from sailfish_amd import hits as H
    rec = np.array([(0, pos, 0, 0, len(read) & 0xFFFF, 0, int(fwd), 0, 0, 0)], dtype=H.HIT_DTYPE)
    e, u = H.gapped_edits_host([t], rec, [0, 1], [read], None, k)
    return int(e[0, 0]), int(u[0, 0])


def _job(L, t, read, fwd, pos, k):
    """... and the harness on the same job, in plain loops and as a group of lanes; the three agree"""
    want = _single(t, read, fwd, pos, k)[0]
    assert L.vgh_job(read, len(read), int(fwd), t, len(t), pos, k, 0, 0) == want
    assert L.vgh_job(read, len(read), int(fwd), t, len(t), pos, k, 1, len(read)) == want
    if want:                                                          # one edit fewer allowed: the group reports the failure
        assert L.vgh_job(read, len(read), int(fwd), t, len(t), pos, k, 1, want - 1) == 2 ** 64 - 1
    return want


def test_hand_computed_jobs(built, harness):
    """the expected edits of each job are written here, worked out from the rule by hand"""
    from sailfish_amd import hits as H
    L = harness
    m = T[5:25]
    assert _job(L, T, m, True, 5, 3) == 0 and _job(L, T, old_corpus.revcomp(m), False, 5, 3) == 0
    assert _job(L, T, m, True, 7, 3) == 0 and _job(L, T, m, True, 2, 3) == 0           # the start diagonal is free: 2 or 3 off costs nothing
    assert _single(T, m, True, 7, 0)[0] == _single(T, m, True, 7, 0)[1] > 5            # ... where the one diagonal alone pays for its bases
    # the deletion in the middle: 2 transcript bases skipped, recorded on the first half's diagonal
    dele = T[:20] + T[22:]
    assert _single(T, dele, True, 0, 0)[0] >= 10
    assert [_job(L, T, dele, True, 0, k) for k in (2, 3, 15)] == [2, 2, 2] and _job(L, T, dele, True, 0, 1) > 2      # (k = 1 cannot reach the far half)
    assert _job(L, T, old_corpus.revcomp(dele), False, 0, 3) == 2
    assert _job(L, T, dele, True, 2, 3) == 2                                           # recorded on the far half's diagonal instead
    ins = T[:20] + b"GG" + T[20:]                                                      # 2 read bases more than the transcript has
    assert [_job(L, T, ins, True, 0, k) for k in (2, 3)] == [2, 2] and _job(L, T, ins, True, 0, 1) > 2 and _job(L, T, ins, True, -2, 2) == 2
    # N matches nothing, in either text, and is one edit either way; lower case is a base
    assert _job(L, T, m[:9] + b"N" + m[10:], True, 5, 3) == 1 and _job(L, T[:14] + b"N" + T[15:], m, True, 5, 3) == 1
    assert _job(L, T.lower(), m, True, 5, 2) == 0 and _job(L, T, m.lower(), True, 5, 2) == 0
    assert _job(L, b"N" * 40, b"N" * 20, True, 5, 3) == 20
    # off the transcript: every base is an edit, a read hanging over an end pays for the overhang once the band cannot reach
    assert _job(L, T, m, True, -1000, 15) == 20 and _job(L, T, m, True, 1 << 20, 15) == 20
    assert _job(L, T, b"GGGG" + T[:16], True, -4, 3) == 4 and _job(L, T, T[30:] + b"AAAAAAA", True, 30, 3) == 7
    assert _job(L, T, T[:16], True, -3, 3) == 0 and _job(L, T, T[:16], True, -4, 3) > 0
    assert _job(L, b"A", b"A", True, 0, 15) == 0 and _job(L, b"A", b"C", True, 0, 15) == 1 and _job(L, b"A", b"CCACC", True, 0, 15) == 4
    assert _job(L, T, b"", True, 0, 3) == 0
    # records: the 2-base deletion fails ungapped at 0.9 and survives with 2 edits at max_indel = 3
    rec = np.array([(0, 0, 0, 0, 38, 0, 1, 0, 0, 0)], dtype=H.HIT_DTYPE)
    assert len(H.verify_hits_host([T], rec, [0, 1], [dele], None, 900, False)[0]) == 0
    h, o, s, st = H.verify_hits_gapped_host([T], rec, [0, 1], [dele], None, 900, False, 3)
    assert o.tolist() == [0, 1] and s.tolist() == [(2, _single(T, dele, True, 0, 0)[1], 0, 0)]
    assert st == dict(records_in=1, records_out=1, reads_in=1, reads_out=1, failed_identity=0, dropped_not_best=0, sum_edits=2, rescued=1)
    assert len(H.verify_hits_gapped_host([T], rec, [0, 1], [dele], None, 950, False, 3)[0]) == 0      # 36 000 < 36 100
    with pytest.raises(ValueError, match="record 0 "):
        bad = rec.copy(); bad["tid"] = 1
        H.verify_hits_gapped_host([T], bad, [0, 1], [dele], None, 900, False, 3)
    for k in (0, 16, -1):
        with pytest.raises(ValueError):
            H.verify_hits_gapped_host([T], rec, [0, 1], [dele], None, 900, False, k)


def test_corpus_exercises_the_feature(built):
    cs = corpus.cases()
    got = corpus.check_coverage()
    assert got["rescued"] >= 50 and got["k3_not_k1"] >= 10 and got["mapped_never"] >= 10 and got["best_drops"] >= 1
    for name in ("edges_pe", "edges_se"):
        c = cs[name]
        assert set(c["hits"]["mate_status"].tolist()) == ({1, 2, 3} if c["r2"] is not None else {0})
        assert {1, 10, 16, 17} <= set(len(s) for s in c["seqs"])
    assert set(corpus.EDGE_LENGTHS) <= set(len(r) for r in cs["edges_se"]["r1"]) | set(len(r) for r in cs["edges_pe"]["r1"])
    assert max(np.diff(cs["indels_se"]["off"])) == 70 and int((np.diff(cs["indels_se"]["off"]) == 0).sum()) >= 3
    # an indel of exactly k passes at k, one of k + 1 does not become cheaper than at k + 1
    c = cs["indels_se"]
    for j, k in enumerate(corpus.KS):
        e = corpus.edits("indels_se", k)[0][:, 0]
        first = 8 * j                                                 # per k: (k, k + 1) x (deletion, insertion) x (forward, reverse)
        assert e[first:first + 4].max() <= k, (k, e[first:first + 8])
        if k < 15:
            assert e[first + 4:first + 8].min() > e[first:first + 4].max(), (k, e[first:first + 8])
    # the pair with one mate rescued and the other failing: the pair falls, the orphan record of the rescued mate survives
    c = cs["indels_pe"]
    r = next(r for r in range(len(c["r1"])) if c["off"][r + 1] - c["off"][r] == 2 and c["hits"][c["off"][r]]["mate_status"] == 3 and
             corpus.edits("indels_pe", 3)[0][c["off"][r], 1] > 50)
    h, o, s, st = corpus.expected("indels_pe", 3, 900, False)
    assert o[r + 1] - o[r] == 1 and h[o[r]]["mate_status"] == 1 and s[o[r]]["edits"] == 2 and s[o[r]]["ungapped"] > 10
    # the long mate: three indels and 1 % substitutions; its score saturates nowhere but the all-N mate's does at permille 0
    h, o, s, st = corpus.expected("long", 3, 0, False)
    assert o.tolist() == [0, 1, 2, 3] and 600 < s["edits"][0] < 800 and s["edits"][0] == s["edits"][1] and s["ungapped"][0] > 30000      # (46 000 bases lie on shifted diagonals)
    assert s["edits"][2] == 65535 and s["ungapped"][2] == 65535 and st["sum_edits"] == 70000 + 2 * int(s["edits"][0])
    assert corpus.expected("long", 1, 900, False)[3]["records_out"] == 0 and corpus.expected("long", 3, 900, False)[3]["rescued"] == 2


def _run_harness(L, case, permille, keep_best, k, lanes):
    ts, toff = old_corpus.packed(case["seqs"])
    tl = np.array([len(x) for x in case["seqs"]], np.uint32)
    s1, o1 = old_corpus.packed(case["r1"])
    s2, o2 = old_corpus.packed(case["r2"]) if case["r2"] is not None else (None, None)
    n = len(case["hits"])
    oh, oo, os_ = np.zeros(max(n, 1), O.HIT_DTYPE), np.zeros(len(case["off"]), np.uint32), np.zeros(max(n, 1), np.uint64)
    st = np.zeros(8, np.uint64)
    p = lambda a: None if a is None else a.ctypes.data
    rc = L.vgh_verify(p(ts), p(toff), p(tl), len(tl), p(s1), p(o1), p(s2), p(o2), len(case["r1"]), p(case["hits"]), p(case["off"]), permille, int(keep_best),
                      k, lanes, p(oh), p(oo), p(os_), p(st))
    return rc, oh, oo, os_, st


def test_verifygfmt_equals_the_statement(built, harness):
    """over the whole corpus, k in 1 2 3 7 8 15, permille 0 / 900 / 1000 with and without keep_best: the harness, in plain loops and as
    groups of 16 and 32 lanes with their early stop, gives the statement's records, offsets, scores and stats"""
    from sailfish_amd import hits as H
    total = 0
    for name, case in corpus.cases().items():
        for k in corpus.KS:
            for permille, kb in corpus.OPTIONS:
                if name == "long" and (kb or k in (2, 7)):
                    continue                                          # (the sanitizer program below runs these too)
                h, o, s, st = corpus.expected(name, k, permille, kb)
                for lanes in (0, 1):
                    rc, oh, oo, os_, ost = _run_harness(harness, case, permille, kb, k, lanes)
                    what = (name, k, permille, kb, lanes)
                    assert rc == len(h), what
                    assert np.array_equal(oo, o) and np.array_equal(oh[:rc], h) and np.array_equal(os_[:rc], s.view(np.uint64)), what
                    assert ost.tolist() == [st[key] for key in H.VERIFYG_STATS], what
                total += len(h)
    assert total > 50000
    case = dict(corpus.cases()["edges_se"])
    bad = case["hits"].copy(); bad["tid"][[7, 3, 11]] = len(case["seqs"])
    case["hits"] = bad
    assert _run_harness(harness, case, 900, False, 3, 1)[0] == -(1 + 3)


def test_harness_runs_clean_under_sanitizers(built, tmp_path):
    """the same functions as a stand-alone program built with -fsanitize=address,undefined: every case of the corpus over the whole
    grid, every text in a block of exactly its size, so a 16-byte load that leaves a mate or a transcript is a report"""
    exe = str(tmp_path / "verifyg_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DVERIFYG_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    path = tmp_path / "cases.bin"
    n = 0
    with open(path, "wb") as f:
        for name in corpus.cases():
            for k in corpus.KS:
                for permille, kb in corpus.OPTIONS:
                    f.write(corpus.blob(name, k, permille, kb)); n += 1
    r = subprocess.run([exe, str(path)], text=True, capture_output=True)
    assert r.returncode == 0 and f"verifyg harness ok: {n} cases" in r.stdout, r.stdout + r.stderr


def test_k0_is_the_ungapped_pass_on_the_old_corpus(built):
    """gapped_edits_host with k = 0 is mism + over of verify_hits_host, record for record, on the ungapped pass's own corpus"""
    from sailfish_amd import hits as H
    n = 0
    for name, c in old_corpus.cases().items():
        e, u = H.gapped_edits_host(c["seqs"], c["hits"], c["off"], c["r1"], c["r2"], 0)
        assert np.array_equal(e, u), name
        h, o, s, st = old_corpus.expected(name, 0, False)             # permille 0: every record survives, in order
        assert len(h) == len(c["hits"])
        two = c["hits"]["mate_status"] == 3
        whole = (s["mism"] < 65535) & (s["over"] < 65535)             # (a saturated field no longer tells the count)
        assert np.array_equal(e[whole, 0], (s["mism"].astype(np.int64) + s["over"])[whole]) and whole.sum() >= len(h) - 3, name
        assert np.array_equal(e[two, 1], s["mate_mism"][two].astype(np.int64) + s["mate_over"][two]) and not e[~two, 1].any(), name
        n += len(h)
    assert n > 5000


def test_edits_fall_with_k_and_stay_below_the_ungapped_count(built):
    for name in corpus.cases():
        prev = None
        for k in corpus.KS:
            e, u = corpus.edits(name, k)
            assert np.all(e <= u) and np.all(e >= 0), (name, k)
            if prev is not None:
                assert np.all(e <= prev), (name, k)
            prev = e
    e1, u1 = corpus.edits("pe_indel", 1)
    assert int((e1 < u1).sum()) > 100 and int((corpus.edits("pe_indel", 3)[0] < e1).sum()) > 50


def _brute(a, b_of, pos, k):
    """a full (len + 1) x (columns + 1) edit-distance matrix with a free start and end column, cells outside the band forbidden: a
    path from (row 0, any column in the band) to (row len, any column in the band); diagonal of (i, x) = x - pos - i within -k .. k"""
    n = len(a)
    INF = 10 ** 9
    lo, hi = pos - k - 1, pos + n + k + 1
    W = hi - lo + 1
    # cell (i, x): i read bases consumed, the next transcript position is x; its diagonal is x - pos - i
    prev = [0 if -k <= (lo + c) - pos <= k else INF for c in range(W)]
    for i in range(n):
        cur = [INF] * W
        for c in range(W):
            x = lo + c
            if not -k <= x - pos - (i + 1) <= k:
                continue
            best = INF
            if c > 0 and prev[c - 1] < INF:                           # read base i against transcript position x - 1
                bx = b_of(x - 1)
                best = prev[c - 1] + (0 if a[i] <= 3 and bx == a[i] else 1)
            if prev[c] < INF:                                         # read base i unaligned: same x, one row down
                best = min(best, prev[c] + 1)
            cur[c] = best
        for c in range(1, W):                                         # transcript bases skipped
            if -k <= (lo + c) - pos - (i + 1) <= k and cur[c - 1] + 1 < cur[c]:
                cur[c] = cur[c - 1] + 1
        prev = cur
    return min(prev)


def test_brute_force_band_agrees_on_short_jobs(built):
    """200 short jobs: the statement equals a full-matrix DP restricted to the band"""
    from sailfish_amd import hits as H
    rng = np.random.default_rng(91)
    for _ in range(200):
        tl, n, k = int(rng.integers(1, 40)), int(rng.integers(1, 30)), int(rng.integers(0, 16))
        alphabet = np.frombuffer(b"ACGTAACCNacgt", np.uint8)
        t, read = bytes(rng.choice(alphabet, tl)), bytes(rng.choice(alphabet, n))
        if rng.random() < 0.6 and tl > 6:                             # a read that is mostly the transcript's
            a = int(rng.integers(0, tl - 3)); read = corpus.with_indel(rng, t[a:a + n] or read, 1, 3)
        fwd = bool(rng.integers(0, 2))
        pos = int(rng.integers(-n - 3, tl + 3))
        code = H._BASE_CODE[np.frombuffer(read, np.uint8)]
        a = [int(v) for v in (code if fwd else np.where(code > 3, 4, 3 - code)[::-1])]
        tc = H._BASE_CODE[np.frombuffer(t, np.uint8)]
        want = _brute(a, lambda x: int(tc[x]) if 0 <= x < tl else 5, pos, k)
        assert _single(t, read, fwd, pos, k)[0] == want, (t, read, fwd, pos, k)


def test_python_surface_checks_max_indel(built):
    """verify_hits raises for max_indel = 16 and -1 before any device work (there is no device here), and _validation before indexing"""
    import sailfish_amd as sf
    from sailfish_amd import hits as H
    assert H.GSCORE_DTYPE.itemsize == 8 and H.GSCORE_DTYPE.names == ("edits", "ungapped", "mate_edits", "mate_ungapped")
    assert H.VERIFYG_STATS == ("records_in", "records_out", "reads_in", "reads_out", "failed_identity", "dropped_not_best", "sum_edits", "rescued")
    for bad in (16, -1, 2.5):
        with pytest.raises(ValueError):
            H.verify_hits(None, None, None, None, max_indel=bad)
        with pytest.raises(ValueError):
            sf.mapper._validation(True, 0.9, False, bad)
        with pytest.raises(ValueError):
            sf.mapper.quantify_reads(["t"], [b"ACGT" * 20], [b"ACGT" * 10], None, "U", "unused", validate_mappings=True, max_indel=bad, device="cuda")
    assert sf.mapper._validation(True, 0.9, False, 0) == (dict(min_identity=0.9, keep_best=False), dict.fromkeys(H.VERIFY_STATS, 0))
    assert sf.mapper._validation(True, 0.9, True, 3) == (dict(min_identity=0.9, keep_best=True, max_indel=3), dict.fromkeys(H.VERIFYG_STATS, 0))
    assert sf.mapper._validation(False, 0.9, True, 3) == (None, None)
