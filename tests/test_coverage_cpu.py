"""The coverage pass and the bedGraph file without a GPU: csrc/coverfmt.h alone (tests/coverage_harness.cpp, g++ -Wall -Wextra -Werror;
once more as a stand-alone program under -fsanitize=address,undefined) against the Python statement hits.coverage_host over the shared
corpus (tests/coverage_corpus.py), in the runs, the bits of the summary, the counters and the bytes of the text; the rule's small
cases worked by hand; the proof that the corpus tells the wrong rules apart; the result's independence of the batches; and the
options' ValueErrors.  Every comparison is equality of integers or bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coverage_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "coverage_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p
RESULT = ("reads", "records", "lines", "intervals", "empty_intervals", "bases_added", "runs", "bases_covered", "residue")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("covh")), "libcoverage_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.ch_open.restype = _P
    L.ch_open.argtypes = [_P, C.c_uint64]
    L.ch_close.argtypes = [_P]
    L.ch_add.restype = C.c_int64
    L.ch_add.argtypes = [_P, _P, _P, C.c_uint32, _P, _P, _P, _P]
    L.ch_finish.argtypes = [_P, _P]
    L.ch_runs.argtypes = [_P] * 5
    L.ch_summary.argtypes = [_P, _P]
    L.ch_text.restype = C.c_uint64
    L.ch_text.argtypes = [_P] * 4
    L.ch_weight.restype = C.c_uint64
    L.ch_weight.argtypes = [C.c_double]
    L.ch_p_bad.argtypes = [C.c_double]
    L.ch_div128.restype = C.c_uint64
    L.ch_div128.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    L.ch_depth.restype = C.c_double
    L.ch_depth.argtypes = [C.c_uint64]
    return L


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _harness_add(L, c, batch):
    h, o, p, aln = batch
    h, o = np.ascontiguousarray(h), np.ascontiguousarray(o, np.uint32)
    p = None if p is None else np.ascontiguousarray(p, np.float64)
    a = (None, None, None) if aln is None else (np.ascontiguousarray(aln[0], np.int32), np.ascontiguousarray(aln[1], np.uint64),
                                                np.ascontiguousarray(np.concatenate([aln[2], [0]]), np.uint32))
    return L.ch_add(c, _ptr(h), _ptr(o), len(o) - 1, _ptr(p), _ptr(a[0]), _ptr(a[1]), _ptr(a[2]))


def _harness_result(L, c, ref_len, names):
    st = np.zeros(9, np.uint64)
    L.ch_finish(c, _ptr(st))
    n, M = int(st[6]), len(ref_len)
    tid, start, end, total = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint64)
    L.ch_runs(c, _ptr(tid), _ptr(start), _ptr(end), _ptr(total))
    cols = np.zeros(3 * M)
    L.ch_summary(c, _ptr(cols))
    blob = np.frombuffer(b"".join(names) + b"\0", np.uint8).copy()
    off = np.zeros(M + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in names])
    size = L.ch_text(c, _ptr(blob), _ptr(off), None)
    text = np.zeros(size + 1, np.uint8)
    assert L.ch_text(c, _ptr(blob), _ptr(off), _ptr(text)) == size
    return (tid, start, end, total), (cols[:M], cols[M:2 * M], cols[2 * M:]), dict(zip(RESULT, st.tolist())), text[:size].tobytes()


def _same(got, want):
    (g_runs, g_sum, g_st), (w_runs, w_sum, w_st) = got, want
    assert all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(g_runs, w_runs))
    assert all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(g_sum, w_sum))
    assert {k: g_st[k] for k in RESULT} == {k: w_st[k] for k in RESULT}


def _hits(rows):
    """rows of (tid, pos, read_len[, mate_pos, mate_len]) -> HIT_DTYPE records; five fields: a mate_status 3 pair"""
    h = np.zeros(len(rows), corpus.HIT_DTYPE)
    for i, r in enumerate(rows):
        h[i]["tid"], h[i]["pos"], h[i]["read_len"] = r[:3]
        if len(r) == 5:
            h[i]["mate_status"], h[i]["mate_pos"], h[i]["mate_len"] = 3, r[3], r[4]
    return h


def test_the_rule_worked_by_hand(built):
    """two transcripts of 8 and 4 bases, three records, counted on paper; the weight's edges; the alignment walk; the errors"""
    from sailfish_amd import coverage as cov, hits as H
    assert H.HIT_DTYPE == corpus.HIT_DTYPE
    h = _hits([(0, -2, 5), (0, 3, 10, 4, 3), (1, 0, 4)])
    (tid, start, end, total), (frac, mean, maxd), st = H.coverage_host([8, 4], [(h, [0, 2, 3], [1.0, 0.5, 2.0 ** -32], None)])
    # transcript 0: [0, 3) at 2^32; [3, 8) and the mate's [4, 7) at 2^31 each.  transcript 1: [0, 4) at q = 1
    assert tid.tolist() == [0, 0, 0, 0, 1] and start.tolist() == [0, 3, 4, 7, 0] and end.tolist() == [3, 4, 7, 8, 4]
    assert total.tolist() == [1 << 32, 1 << 31, 1 << 32, 1 << 31, 1]
    assert frac.tolist() == [1.0, 1.0] and mean.tolist() == [7 / 8, float((4 // 4)) * 2.0 ** -32] and maxd.tolist() == [1.0, 2.0 ** -32]
    assert st == dict(reads=2, records=3, lines=4, intervals=4, empty_intervals=0, bases_added=15, runs=5, bases_covered=12, bases_total=12, residue=0)
    assert cov.coverage_text_host(["a", b"b"], (tid, start, end, total)) == b"a\t0\t3\t1\na\t3\t4\t0.5\na\t4\t7\t1\na\t7\t8\t0.5\nb\t0\t4\t2.32831e-10\n"
    # uniform: the read of two records weighs 2^31 a record, the read of one 2^32
    runs, _, _ = H.coverage_host([8, 4], [(h, [0, 2, 3], None, None)])
    assert runs[1].tolist() == [0, 4, 7, 0] and runs[3].tolist() == [1 << 31, 1 << 32, 1 << 31, 1 << 32]
    assert H.coverage_host([8], [(_hits([(0, 0, 8)] * 3), [0, 3], None, None)])[0][3].tolist() == [3 * ((1 << 32) // 3)]
    # the alignment: 5M | 2S 3M 2D, the mate 3M | 4M; slot 1 is no line and is never read
    aln = ([0, 99, 3, 4, 0, 99], [0, 1, 1, 4, 5, 6, 6], [5 << 4, 2 << 4 | 4, 3 << 4, 2 << 4 | 2, 3 << 4, 4 << 4])
    runs, (frac, _, maxd), st = H.coverage_host([8, 4], [(h, [0, 2, 3], None, aln)])
    assert runs[1].tolist() == [0, 3, 4, 5, 6, 0] and runs[2].tolist() == [3, 4, 5, 6, 7, 4]
    assert runs[3].tolist() == [1 << 31, 2 << 31, 3 << 31, 2 << 31, 1 << 31, 1 << 32] and frac[0] == 7 / 8 and maxd[0] == 1.5
    # the weight: truncated; 2^-32 is 1, 2^-33 is 0, the largest double below 1 is 2^32 - 1
    assert [H.coverage_weight(p) for p in (0.0, 1.0, 2.0 ** -32, 2.0 ** -33, 0.3, 1.0 - 2.0 ** -53)] == [0, 1 << 32, 1, 0, 1288490188, (1 << 32) - 1]
    # empty intervals are counted, never an error; a transcript of no bases takes none
    _, _, st = H.coverage_host([8, 0], [(_hits([(0, 8, 5), (0, -5, 5), (0, 2, 0), (1, 0, 3), (0, 7, 1)]), [0, 5], None, None)])
    assert (st["intervals"], st["empty_intervals"], st["bases_added"], st["runs"]) == (1, 4, 1, 1)
    # no transcripts, no reads
    assert H.coverage_host([], [(_hits([]), [0], None, None)])[2]["runs"] == 0
    assert H.coverage_host([3], [(_hits([]), [0, 0, 0], None, None)])[2]["reads"] == 2
    with pytest.raises(ValueError, match="record 1 names transcript >= 2"):
        H.coverage_host([8, 4], [(_hits([(0, 0, 1), (2, 0, 1), (5, 0, 1)]), [0, 3], None, None)])
    for bad in (float("nan"), -2.0 ** -1074, 1.0 + 2.0 ** -52, float("inf")):
        with pytest.raises(ValueError, match="posterior of record 2 "):
            H.coverage_host([8], [(_hits([(0, 0, 1)] * 4), [0, 4], [0.5, 1.0, bad, bad], None)])


def test_coverfmt_equals_the_statement(built, harness):
    """over the corpus the header equals coverage_host in the runs, in the bits of the three columns, in every counter and in the bytes
    of the file -- with posteriors, with uniform weights and with alignments; and adding the corpus in 1, 2 and 7 batches gives the same
    result in both"""
    from sailfish_amd import coverage as cov, hits as H
    L = harness
    for mode in corpus.MODES:
        want = corpus.expected(mode)
        assert want[2]["residue"] == 0 and want[2]["runs"] > 4000 and want[2]["empty_intervals"] >= 5
        text = cov.coverage_text_host(corpus.names(), want[0])
        for k in (1, 2, 7):
            batches = corpus.mode_batches(mode, k)
            if k > 1:
                _same(H.coverage_host(corpus.REF_LEN, batches), want)
            c = L.ch_open(_ptr(corpus.REF_LEN), corpus.M)
            assert all(_harness_add(L, c, b) == 0 for b in batches)
            *got, got_text = _harness_result(L, c, corpus.REF_LEN, corpus.names())
            assert _harness_add(L, c, batches[0]) == -(1 << 63) + 1          # after finish
            L.ch_close(c)
            _same(got, want)
            assert got_text == text, (mode, k)
    # the scalar pieces, against Python's integers
    rng = np.random.default_rng(3)
    for p in [0.0, 1.0, 2.0 ** -32, 2.0 ** -33, 0.3, 1.0 - 2.0 ** -53] + rng.random(2000).tolist():
        assert L.ch_weight(p) == H.coverage_weight(p) == int(p * (1 << 32)) and not L.ch_p_bad(p)
    assert all(L.ch_p_bad(p) for p in (float("nan"), -1e-300, 1.0000000000000002, float("inf")))
    for _ in range(2000):
        d = int(rng.integers(1, 1 << 32))
        s = int(rng.integers(0, 1 << 63)) * int(rng.integers(0, 2 * d)) % (d << 64)
        assert L.ch_div128(s >> 64, s & ((1 << 64) - 1), d) == s // d
    for v in rng.integers(0, 1 << 63, 2000).tolist() + [(1 << 64) - 1, (1 << 53) + 1, (1 << 54) + 2, (1 << 54) + 6]:
        assert L.ch_depth(2 * v + 1 if v < 1 << 63 else v) == float(2 * v + 1 if v < 1 << 63 else v) * 2.0 ** -32


def test_the_headers_errors_name_the_statements_offenders(built, harness):
    """a bad tid before a bad p, the lowest record of either, and nothing added: the next finish equals the run without the bad call"""
    from sailfish_amd import hits as H
    L = harness
    good = corpus.mode_batches("posterior", 2)
    h, o, p, _ = good[1]
    bad_tid, bad_p = h.copy(), p.copy()
    bad_tid["tid"][[40, 7, 300]] = corpus.M
    bad_p[[90, 33]] = [float("nan"), 1.5]
    c = L.ch_open(_ptr(corpus.REF_LEN), corpus.M)
    assert _harness_add(L, c, good[0]) == 0
    assert _harness_add(L, c, (bad_tid, o, bad_p, None)) == -(1 + 7)
    assert _harness_add(L, c, (h, o, bad_p, None)) == 1 + 33
    assert _harness_add(L, c, (h, o, None, None)) == 0       # (uniform weights: the refused p is not read)
    got = _harness_result(L, c, corpus.REF_LEN, corpus.names())[:3]
    L.ch_close(c)
    _same(got, H.coverage_host(corpus.REF_LEN, [good[0], (h, o, None, None)]))
    with pytest.raises(ValueError, match="record 7 "):
        H.coverage_host(corpus.REF_LEN, [good[0], (bad_tid, o, bad_p, None)])
    with pytest.raises(ValueError, match="record 33 "):
        H.coverage_host(corpus.REF_LEN, [good[0], (h, o, bad_p, None)])


def test_the_corpus_tells_the_wrong_rules_apart(built):
    """each wrong rule -- q rounded instead of truncated, D counted as covered, no clip at len_t, S in 64 bits -- changes at least one
    expected value: else the equalities of the other tests would prove nothing"""
    h, o, p, (a_pos, a_off, a_ops) = corpus.batch()
    runs, (frac, mean, maxd), st = corpus.expected("posterior")
    tid, start, end, total = runs
    # rounding: 0.3 2^32 = 1288490188.8; the pile of transcript 8 holds 10 000 of them
    q_trunc, q_round = (p * 2.0 ** 32).astype(np.uint64), np.rint(p * 2.0 ** 32).astype(np.uint64)
    assert (q_trunc != q_round).sum() > 10000
    pile = total[tid == 8]
    assert pile.tolist() == [10000 * 1288490188] and 10000 * 1288490189 != int(pile[0])
    # D as covered: the aligned corpus has a 5D between covered stretches and a 300D that would run over the transcript
    a_runs, _, a_st = corpus.expected("aligned")
    d_words = [(int(w) >> 4) for w in a_ops if int(w) & 15 == corpus.D_OP]
    assert sorted(d_words) == [5, 300]
    # 10M 5D 20= from base 10 covers [10, 20) and [25, 45), and no other line of transcript 10 reaches [20, 25): a hole a covered D would fill
    t10 = a_runs[0] == 10
    assert not any(s < 25 and e > 20 for s, e in zip(a_runs[1][t10].tolist(), a_runs[2][t10].tolist()))
    assert 20 in a_runs[2][t10].tolist() and 25 in a_runs[1][t10].tolist() and a_st["empty_intervals"] == st["empty_intervals"] + 2
    # ... while the same records on the diagonal cover base 22
    t10p = tid == 10
    assert any(s <= 22 < e for s, e in zip(start[t10p].tolist(), end[t10p].tolist()))
    # no clip at len_t: lines run over the end of transcripts 2, 5, 9 and 10; unclipped they would reach the next transcript's slots
    over = (h["pos"].astype(np.int64) + h["read_len"] > corpus.REF_LEN[h["tid"]]) & (h["pos"] < corpus.REF_LEN[h["tid"]].astype(np.int64))
    assert set(h["tid"][over].tolist()) >= {2, 5, 9, 10}
    assert int(end[tid == 2].max()) == 2 and int(end[tid == 5].max()) == 100 and st["residue"] == 0
    unclipped = int((np.minimum(h["pos"].astype(np.int64) + h["read_len"], 1 << 40) - np.maximum(h["pos"].astype(np.int64), 0)).clip(0).sum())
    assert unclipped > st["bases_added"]
    # S in 64 bits: 70 000 records of 65 535 bases at 2^32 each
    S = 70000 * 65535 * (1 << 32)
    assert S >= 1 << 64 and mean[11] == 70000.0 and float((S % (1 << 64)) // 65535) * 2.0 ** -32 != mean[11]
    assert maxd[11] == 70000.0 and frac[11] == 1.0
    # the staircase: every base of transcript 7 starts a run
    assert start[tid == 7].tolist() == list(range(64)) and total[tid == 7].tolist() == [1288490188 * (i + 1) for i in range(64)]
    # q = 0 adds nothing but is an interval; the neighbours 0, 1, 2 and the interval that ends at len_t beside one that starts at 0
    assert (start[tid == 3].tolist(), end[tid == 3].tolist(), start[tid == 4].tolist()) == ([40], [50], [0]) and not (tid == 1).any()
    assert end[tid == 0].tolist() == [1] and end[tid == 2].tolist() == [1, 2]


def test_the_standalone_harness_under_sanitizers(built, tmp_path):
    """the same header in a program of its own, with -fsanitize=address,undefined, over the corpus as a file, every array in a block of
    exactly its size: whole, then read by read"""
    exe = str(tmp_path / "coverage_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DCOVERAGE_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    for mode in corpus.MODES:
        path = tmp_path / (mode + ".bin")
        path.write_bytes(corpus.blob(mode))
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 0 and "coverage harness ok" in r.stdout, (mode, r.stdout, r.stderr)


def test_the_option_errors(built):
    """an unknown coverage_weights and coverage_compress without write_coverage are ValueErrors before anything is indexed: the
    transcripts here are not even sequences"""
    import sailfish_amd as sf
    for fn, args in ((sf.mapper.quantify_reads, (["t"], [None], [b"ACGT"], None, "U", "/nonexistent/out")),
                     (sf.mapper.quantify_files, ("/nonexistent/tx.fa", "/nonexistent/r.fq", None, "U", "/nonexistent/out"))):
        with pytest.raises(ValueError, match="coverage_weights"):
            fn(*args, write_coverage="/nonexistent/c.bedgraph", coverage_weights="rsem")
        with pytest.raises(ValueError, match="coverage_weights"):
            fn(*args, coverage_weights="Posterior")
        with pytest.raises(ValueError, match="coverage_compress"):
            fn(*args, coverage_compress=True)
        with pytest.raises(ValueError, match="write_coverage"):
            fn(*args, write_coverage=17)
