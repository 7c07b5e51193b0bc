"""Library-format detection without a GPU: csrc/libdetfmt.h alone (tests/libdet_harness.cpp, g++ -Wall -Wextra -Werror; once more as
a stand-alone program under -fsanitize=address,undefined) against the Python statement hits.library_kinds_host over the shared corpus
(tests/libdet_corpus.py), in every counter, in one call and in calls of 100 reads; the decision worked by hand; the compatibility
mask against compatibleHit restated here; the text of lib_format_counts.json; six simulated protocols mapped with the restated scan
and decided by the statement; and the options' ValueErrors."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import libdet_corpus as corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sailfish_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "libdet_harness.cpp")
WARN = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC]
_P = C.c_void_p


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("libdeth")), "liblibdet_harness.so")
    subprocess.check_call(["g++", "-O2"] + WARN + ["-shared", "-fPIC", SRC, "-o", so])
    L = C.CDLL(so)
    L.lh_library_kinds.restype = None
    L.lh_library_kinds.argtypes = [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_int] * 6 + [C.POINTER(C.c_int64), _P]
    L.lh_kind.restype = C.c_uint32
    L.lh_kind.argtypes = [_P, C.c_int]
    L.lh_compat_mask.restype = C.c_uint32
    L.lh_compat_mask.argtypes = [C.c_int] * 3
    L.lh_vote.restype = C.c_uint32
    L.lh_vote.argtypes = [C.c_uint32, C.c_int]
    L.lh_decide.restype = C.c_int32
    L.lh_decide.argtypes = [_P, C.c_int, C.c_uint32, C.c_uint64]
    return L


def _serial(L, h, o, calls, paired, dovetail, budget, fmt):
    from sailfish_amd import hits as H
    t = H.LIBRARY_FORMATS[fmt] if fmt else (0, 0, 0)
    st, rem = np.zeros(45, np.uint64), C.c_int64(budget)
    for a, b in calls:
        L.lh_library_kinds(h.ctypes.data, o.ctypes.data, a, b - a, corpus.MAX_READ_OCCS, int(paired), int(dovetail), int(fmt is not None), *t, C.byref(rem), st.ctypes.data)
    return rem.value, st


def test_names_and_kinds_of_the_corpus(built, harness):
    """the published names; every named record and every hitType edge is of the kind the corpus says, by the statement and by the
    header; the batch holds what the issue lists"""
    from sailfish_amd import hits as H
    assert H.LIBDET_KINDS == corpus.KINDS and H.LIBDET_STATS == corpus.STATS and tuple(H.LIBRARY_FORMATS) == corpus.FORMATS
    one = lambda r: np.array([r], dtype=corpus.HIT_DTYPE)
    for k in corpus.KINDS:
        for dovetail in (False, True):
            assert corpus.KINDS[H.record_kinds_host(one(corpus.rec(k)), dovetail)[0]] == k
            assert corpus.KINDS[harness.lh_kind(one(corpus.rec(k)).ctypes.data, dovetail)] == k
    for r, plain, dove in corpus.EDGES:
        got = [corpus.KINDS[H.record_kinds_host(one(r), d)[0]] for d in (False, True)]
        assert got == [plain, dove] == [corpus.KINDS[harness.lh_kind(one(r).ctypes.data, d)] for d in (0, 1)], r
    assert {p != d for _, p, d in corpus.EDGES} == {True, False}
    h, o, r0, h0 = corpus.batch()
    n = np.diff(o.astype(np.int64))
    assert 2900 <= len(n) <= 3200 and (n == 0).sum() > 100 and n.max() == corpus.LONG_READ > 1536
    assert {corpus.MAX_READ_OCCS, corpus.MAX_READ_OCCS + 1} <= set(n.tolist()) and 0 < r0 < len(n) and o[r0] == h0
    _, st = corpus.expected(True, False, 0)
    assert all(st["reads_kind"]) and all(st["records_kind"]) and st["reads_mixed"] > 100 and st["reads_over_occs"] == 4
    assert st["reads"] == len(n) and st["reads_mapped"] + st["reads_over_occs"] + int((n == 0).sum()) == len(n)
    assert st["votes"] == 0 and not any(st["votes_kind"])
    for mask, paired, want in ((1, True, 0), (1 << 5, True, 5), (1 << 6, True, 255), (1 << 10, True, 255), (1 << 10, False, 10), (1 << 11, False, 11),
                               (1, False, 255), (3, True, 255), (0, True, 255), (1 << 12, True, 255), (1 << 12, False, 255), (3 << 10, False, 255)):
        assert harness.lh_vote(mask, paired) == want, (mask, paired)


@pytest.mark.parametrize("paired", [True, False])
def test_header_equals_the_statement(built, harness, paired):
    """every counter and the rest of the budget, in one call and in calls of 100 reads with remaining_votes carried, for a budget of 0,
    1, one that ends inside a block, exactly the voters and more; with and without dovetailing and an expected format"""
    h, o, _, _ = corpus.batch()
    for dovetail, fmt in ((False, None), (True, "ISF" if paired else "SR"), (False, "OU" if paired else "U")):
        budgets = corpus.budgets(paired, dovetail)
        assert 150 < budgets[3]
        for budget in budgets:
            rem, st = corpus.expected(paired, dovetail, budget, fmt)
            assert st["votes"] == min(budget, budgets[3]) == budget - rem == sum(st["votes_kind"])
            for calls in corpus.splits():
                got_rem, got = _serial(harness, h, o, calls, paired, dovetail, budget, fmt)
                assert got_rem == rem and np.array_equal(got, corpus.stats_vector(st)), (dovetail, fmt, budget, len(calls))
    _, a = corpus.expected(paired, False, 0, None)
    _, b = corpus.expected(paired, True, 0, None)
    assert a["records_kind"] != b["records_kind"]                       # dovetailing moves records between O and I


def test_statement_accumulates_and_slices(built):
    """the statement itself in calls of 100 reads equals the statement at once, and adds to the stats it is given"""
    from sailfish_amd import hits as H
    h, o, _, _ = corpus.batch()
    want_rem, want = corpus.expected(True, True, 150, "ISR")
    rem, st = 150, None
    for a, b in corpus.splits()[1]:
        hh, oo = corpus.slice_batch(h, o, a, b)
        rem, st = H.library_kinds_host(hh, oo, paired_library=True, max_read_occs=corpus.MAX_READ_OCCS, allow_dovetail=True, remaining_votes=rem, expected="ISR", stats=st)
    assert (rem, st) == (want_rem, want)
    assert H.library_kinds_host(h[:0], o[:1], paired_library=True) == (0, H._libdet_stats())


def test_harness_runs_clean_under_sanitizers(built, tmp_path):
    """the same functions as a stand-alone program built with -fsanitize=address,undefined and run directly"""
    exe = str(tmp_path / "libdet_harness")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLIBDET_HARNESS_MAIN"] + WARN + [SRC, "-o", exe])
    path = tmp_path / "batch.bin"
    path.write_bytes(corpus.blob())
    r = subprocess.run([exe, str(path)], text=True, capture_output=True)
    h, o, _, _ = corpus.batch()
    assert r.returncode == 0 and f"libdet harness ok: {len(o) - 1} reads, {len(h)} records, {len(corpus.blob_cases())} cases" in r.stdout, r.stdout + r.stderr


def _votes(**kw):
    return [kw.get(k, 0) for k in corpus.KINDS]


def test_the_decision_worked_by_hand(built, harness):
    """the tie order, 699 / 700 / 701 per mille, min_votes - 1, both single-end calls; the header agrees with the statement on each;
    a min_fraction outside 0.501 .. 1 is a ValueError"""
    from sailfish_amd import hits as H
    table = [
        (_votes(ISF=700, ISR=300), True, "ISF"), (_votes(ISF=699, ISR=301), True, "IU"), (_votes(ISF=701, ISR=299), True, "ISF"),
        (_votes(ISF=300, ISR=700), True, "ISR"), (_votes(ISF=301, ISR=699), True, "IU"), (_votes(ISF=299, ISR=701), True, "ISR"),
        (_votes(ISF=100, OSF=100, MSF=100), True, "ISF"),                 # a three-way tie: inward
        (_votes(ISF=100, ISR=50, OSR=150, MSR=150), True, "IU"),          # ... and the strand is then inward's own: 100 : 50 is 66.7 %
        (_votes(OSF=10, OSR=140, MSF=150, ISF=149), True, "OSR"),         # outward ties with matching: outward
        (_votes(MSF=151, OSR=150, ISF=10), True, "MSF"), (_votes(MSR=200), True, "MSR"), (_votes(MSF=100, MSR=100), True, "MU"),
        (_votes(OSF=150, OSR=50), True, "OSF"), (_votes(OSF=100, OSR=100), True, "OU"),
        (_votes(ISF=199), True, None), (_votes(ISF=100, OSR=99), True, None), (_votes(ISF=100, OSR=100), True, "ISF"), (_votes(), True, None),
        (_votes(ISF=1000, SF=5, LF=7, other=9), True, "ISF"),             # only the pair kinds enter a paired decision
        (_votes(SF=140, SR=60), False, "SF"), (_votes(SF=60, SR=140), False, "SR"), (_votes(SF=139, SR=61), False, "U"), (_votes(SF=100, SR=99), False, None),
        (_votes(ISF=1000, SF=199), False, None),
    ]
    for votes, paired, want in table:
        got, detail = H.decide_library_format(votes, paired)
        assert got == want, (votes, paired, got, want)
        assert detail["permille"] == 700 and detail["min_votes"] == 200
        fid = harness.lh_decide(np.array(votes, np.uint64).ctypes.data, int(paired), 700, 200)
        assert (None if fid < 0 else H._FORMAT_NAMES[H.format_from_id(fid)]) == want, (votes, paired, fid)
    assert H.decide_library_format(dict(votes_kind=_votes(ISF=10)), True, min_votes=10)[0] == "ISF"
    assert H.decide_library_format(_votes(ISF=501, ISR=499), True, min_fraction=0.501)[0] == "ISF"
    assert H.decide_library_format(_votes(ISF=999, ISR=1), True, min_fraction=1.0)[0] == "IU"
    assert H.decide_library_format(_votes(), True, min_votes=0)[0] is None and harness.lh_decide(np.zeros(13, np.uint64).ctypes.data, 1, 700, 0) == -1
    for bad in (0.5, 0.5004, 1.0006, 0.0, 2.0, -0.7):
        with pytest.raises(ValueError, match="min_fraction"):
            H.decide_library_format(_votes(ISF=500), True, min_fraction=bad)
    with pytest.raises(ValueError, match="13"):
        H.decide_library_format([1, 2, 3], True)


def _compatible_hit(fmt, kind):
    """compatibleHit (src/SailfishUtils.cpp:157-229) over a kind's name, restated: the pair form compares the observed format with the
    expected one; the single form looks at the mate status, the strand and the expected strandedness"""
    from sailfish_amd import hits as H
    _, eo, es = H.LIBRARY_FORMATS[fmt]
    if kind == "other":
        return False
    if kind[0] in "IOM":
        oo = {"I": H.TOWARD, "O": H.AWAY, "M": H.SAME}[kind[0]]
        os_ = {"ISF": H.SA, "OSF": H.SA, "ISR": H.AS, "OSR": H.AS, "MSF": H.S, "MSR": H.A}[kind]
        return eo == oo and (es == H.U or es == os_)
    fwd = kind[1] == "F"
    sense, anti = es in (H.U, H.S), es in (H.U, H.A)
    if kind[0] == "S":
        return sense if fwd else anti
    if eo == H.SAME:
        return es == H.U or (es == H.S and fwd) or (es == H.A and not fwd)
    if kind[0] == "L":
        return sense if fwd else anti
    return anti if fwd else sense


def test_compat_mask_is_compatible_hit(built, harness):
    """ld_compat_mask and the statement's mask equal the restated compatibleHit for all twelve formats and thirteen kinds"""
    from sailfish_amd import hits as H
    seen = set()
    for fmt in corpus.FORMATS:
        want = sum(1 << k for k, name in enumerate(corpus.KINDS) if _compatible_hit(fmt, name))
        assert H.library_compat_mask(fmt) == want == harness.lh_compat_mask(*H.LIBRARY_FORMATS[fmt]), fmt
        assert not want >> 12 and want
        seen.add(want)
    assert len(seen) == 12
    assert H.library_compat_mask("ISF") == 1 << 0 and H.library_compat_mask("SF") == 1 << 10 | 1 << 6 | 1 << 9


def test_counts_text_of_a_hand_counted_batch(built):
    """writer.lib_format_counts_text for a batch small enough to count: exact bytes, keys in their order"""
    from sailfish_amd import hits as H
    from sailfish_amd import writer
    recs = [corpus.rec("ISF")] * 3 + [corpus.rec("ISR")] + [corpus.rec("ISF"), corpus.rec("OSF")] + [corpus.rec("LF")] + [corpus.rec("ISF")] * 5
    h = np.array(recs, dtype=corpus.HIT_DTYPE)
    o = np.array([0, 1, 1, 3, 4, 6, 7, 12], np.uint32)                  # ISF, none, ISF x 2, ISR, ISF + OSF, LF, ISF x 5 (over 4)
    rem, votes = H.library_kinds_host(h, o, paired_library=True, max_read_occs=4, remaining_votes=2)
    _, counts = H.library_kinds_host(h, o, paired_library=True, max_read_occs=4, expected="ISF")
    assert rem == 0 and votes["votes_kind"][:2] == [2, 0]
    text = writer.lib_format_counts_text("isf", counts, votes=votes, detected=None, fallback=True)
    zero = {k: 0 for k in corpus.KINDS}
    want = dict(expected_format="ISF", detected=None, fallback=True, num_votes=2, votes=dict(zero, ISF=2), num_reads=7, num_mapped=5, num_over_occs=1,
                num_consistent=4, num_mixed=1, num_compatible=3, compatible_fragment_ratio=0.6, strand_mapping_bias=1 / 3,
                records=dict(zero, ISF=4, ISR=1, OSF=1, LF=1), reads=dict(zero, ISF=2, ISR=1, LF=1))
    assert text == json.dumps(want, indent=4)
    assert list(json.loads(text)) == ["expected_format", "detected", "fallback", "num_votes", "votes", "num_reads", "num_mapped", "num_over_occs", "num_consistent",
                                      "num_mixed", "num_compatible", "compatible_fragment_ratio", "strand_mapping_bias", "records", "reads"]
    assert text.startswith('{\n    "expected_format": "ISF",\n    "detected": null,\n    "fallback": true,\n    "num_votes": 2,\n    "votes": {\n        "ISF": 2,\n')
    empty = json.loads(writer.lib_format_counts_text("SR", H._libdet_stats()))
    assert empty["compatible_fragment_ratio"] == 0.0 and empty["strand_mapping_bias"] == 0.0 and empty["detected"] is None and empty["num_votes"] == 0
    _, se = H.library_kinds_host(np.array([corpus.rec("SF")] * 3 + [corpus.rec("SR")], dtype=corpus.HIT_DTYPE), [0, 1, 2, 3, 4], paired_library=False, expected="SF")
    assert json.loads(writer.lib_format_counts_text("SF", se, detected="SF"))["strand_mapping_bias"] == 0.25


@pytest.mark.parametrize("protocol", corpus.PROTOCOLS)
def test_simulated_protocols_are_decided_as_themselves(built, protocol):
    """400 reads of 50 bases with 2 % substitutions, mapped by the restated scan (s = 19), voted on and decided by the statement: each
    library is named as its protocol, with at least 300 voters; the unstranded libraries split well inside 30 .. 70 %"""
    from oracle import mapper_oracle as MO
    from sailfish_amd import hits as H
    _, seqs, r1, r2 = corpus.simulated(protocol)
    paired = r2 is not None
    hits, off = MO.scan_reads(MO.build_scan_index(seqs), r1, r2, s=19)
    rem, st = H.library_kinds_host(hits, off, paired_library=paired, remaining_votes=50_000)
    assert st["reads"] == corpus.SIM_READS and st["votes"] >= 300 and rem == 50_000 - st["votes"]
    name, detail = H.decide_library_format(st, paired)
    assert name == protocol, (st["votes_kind"], detail)
    if protocol in ("IU", "U"):
        assert 0.4 * detail["total"] < detail["sense"] < 0.6 * detail["total"]
    _, counts = H.library_kinds_host(hits, off, paired_library=paired, expected=name)
    assert counts["reads_compatible"] >= st["votes"]


def test_lib_format_a_value_errors(built, tmp_path):
    """"A" without paired_library, with rescue_mates, a quantify_sam("A") without paired=, a min_fraction out of range: ValueError
    before anything is written or indexed (there is no device here)"""
    import sailfish_amd as sf
    out = tmp_path / "never"
    with pytest.raises(ValueError, match="paired_library"):
        sf.quant.quantify(["t"], np.array([80], np.uint32), [], "A", str(out), device="cuda")
    with pytest.raises(ValueError, match="min_fraction"):
        sf.quant.quantify(["t"], np.array([80], np.uint32), [], "A", str(out), paired_library=True, detect_min_fraction=0.4, device="cuda")
    with pytest.raises(ValueError, match="detect_votes"):
        sf.quant.quantify(["t"], np.array([80], np.uint32), [], "a", str(out), paired_library=False, detect_votes=10, device="cuda")
    with pytest.raises(ValueError, match="rescue_mates"):
        sf.mapper.quantify_reads(["t"], [b"ACGT" * 20], [b"ACGT" * 10], [b"ACGT" * 10], "A", str(out), rescue_mates=True, device="cuda")
    with pytest.raises(ValueError, match="rescue_mates"):
        sf.mapper.quantify_files("no.fa", "no_1.fq", "no_2.fq", "A", str(out), rescue_mates=True, device="cuda")
    with pytest.raises(ValueError, match="paired"):
        sf.quant.quantify_sam("no.sam", "A", str(out))
    with pytest.raises(ValueError, match="contradicts"):
        sf.quant.quantify_sam("no.sam", "IU", str(out), paired=False)
    assert not out.exists()
