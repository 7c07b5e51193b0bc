"""tests/mapper_corpus.py holds the shapes it claims (no GPU): every case is shown, with the oracle alone, to reach the edge of
csrc/mapper.hip that it exists for; the oracle's own records pass the independent brute-force judge; the vectorised index
statement equals MO.build_scan_index entry for entry."""
import numpy as np
import pytest

import mapper_corpus as MC
from oracle import mapper_oracle as MO

SMALL = tuple(n for n in MC.CASE_NAMES if n not in MC.BIG)


def _bits(n_valid, k):
    """the bucket table's width as sfgpu_index_build states it: ~8 k-mers per bucket, between 2^8 and min(2^26, 4^k) buckets"""
    bits = 8
    while bits < 26 and bits < 2 * k and (1 << bits) * 8 < n_valid:
        bits += 1
    return bits


def _recs(name, r, paired=True):
    h, o = MC.expected_for(name, paired)
    return [(int(x["tid"]), int(x["fwd"]), int(x["pos"]), int(x["mate_status"])) for x in h[o[r]:o[r + 1]]]


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_the_oracle_passes_the_independent_judge(name):
    """the restated contract's records are sound and complete by the brute-force judge, paired and single end"""
    c = MC.case(name)
    assert c.why
    h, o = MC.expected(name)
    applied = MC.judge(c, h, o, c.reads2 is not None)
    if c.reads2 is not None:
        applied += MC.judge(c, *MC.expected_for(name, False), False)
    assert applied >= min(len(c.truth), 1) and (not c.truth or applied >= len(c.truth) // 2), (applied, len(c.truth))


def test_the_judge_rejects_false_records():
    """the judge is not vacuous: a shifted position, a flipped strand, a wrong transcript, a wrong fragment length, a dropped
    record and records out of order are all refused"""
    c = MC.case("pairs_end")
    h, o = MC.expected("pairs_end")
    MC.judge(c, h, o, True)
    r = c.props["mate_inside"]
    for field, value in (("pos", 21), ("fwd", 0), ("tid", 3), ("frag_len", 61), ("mate_pos", 36), ("read_len", 59)):
        bad = h.copy(); bad[field][o[r]] = value
        with pytest.raises(AssertionError):
            MC.judge(c, bad, o, True)
    r = c.props["cross_product"]
    bad = h.copy(); bad[o[r]:o[r] + 2] = h[o[r]:o[r] + 2][::-1]
    with pytest.raises(AssertionError):
        MC.judge(c, bad, o, True)
    c = MC.case("m1_end")
    h, o = MC.expected("m1_end")
    o2 = o.copy(); o2[1:] -= 1
    with pytest.raises(AssertionError):
        MC.judge(c, h[1:], o2, False)                        # the first read's record is gone: incomplete


@pytest.mark.parametrize("name", SMALL)
def test_vectorised_table_is_the_scan_index(name):
    c = MC.case(name)
    want, _, k = MO.build_scan_index(c.transcripts, c.k)
    t = MC.table(name)
    assert k == c.k and t[0:len(t)] == want
    idx = MO.build_index(c.transcripts, c.k, c.max_occ)
    vi = MC.VecIndex(t, c.max_occ)
    assert all(vi.get(key) == occ for key, occ in idx.items()) and vi.get(1 << 62) == ()


@pytest.mark.parametrize("name", MC.BIG)
def test_vectorised_table_of_the_large_cases_is_sorted_and_true(name):
    """the large tables are judged without the pure-Python index: sorted by (key, t, p), one entry per clean k-mer position, and
    120 sampled entries spell their key on the transcript"""
    c = MC.case(name)
    t = MC.table(name)
    key = t.keys.astype(object)
    order = list(zip(t.keys.tolist(), t.t.tolist(), t.p.tolist()))
    assert order == sorted(order) and len(set(order)) == len(order)
    clean = sum(int((~(np.lib.stride_tricks.sliding_window_view(MC.FOLD[np.frombuffer(s, np.uint8)], c.k) > 3).any(axis=1)).sum())
                for s in c.transcripts if len(s) >= c.k)
    assert len(t) == clean
    for i in np.random.default_rng(1).integers(0, len(t), 120):
        w = bytes(c.transcripts[int(t.t[i])][int(t.p[i]):int(t.p[i]) + c.k]).upper()
        assert len(w) == c.k and int(key[i]) == int("".join(str(b"ACGT".index(x)) for x in w), 4)


# ---- the shapes --------------------------------------------------------------------------------------------------------------
def test_mode_cases_cover_every_k_and_mode():
    assert {(MC.case(n).k, MC.case(n).seeds, MC.case(n).seed_len) for n in MC.MODE_CASES} == \
        {(k, S, None) for k in MC.KS for S in (2, 3, 8)} | {(k, None, s) for k in MC.KS for s in {8, min(19, k), k}}
    for n in MC.MODE_CASES:
        c = MC.case(n)
        S = c.seeds or 2
        assert 2500 < sum(len(s) for s in c.transcripts) < 3600
        assert {0, 1, c.k - 1, c.k, c.k + 1, c.k + S - 2, c.k + S - 1} <= {len(r) for r in c.reads1}
        assert any(len(s) == c.k - 1 for s in c.transcripts) and any(b"N" in s for s in c.transcripts) and any(s.islower() for s in c.transcripts)
        h, o = MC.expected(n)
        assert len(h) > len(c.reads1) and (h["mate_status"] == 3).sum() > 10 and (h["fwd"] == 0).sum() > 10 and (h["fwd"] == 1).sum() > 10


@pytest.mark.parametrize("S", [3, 8])
def test_a_read_barely_longer_than_k_repeats_a_seed_offset(S):
    """len - k < S - 1: two seeds share an offset and the second is dropped -- the reads of k + S - 2 bases have that, those of
    k + S - 1 bases do not; with the duplicate kept, a transcript would collect a vote twice from one window"""
    k = 16
    assert len(MO.seed_offsets(k + S - 2, k, S)) == S - 1 and len(MO.seed_offsets(k + S - 1, k, S)) == S
    assert MO.seed_offsets(k, k, S) == [(0, 0)] and [o for _, o in MO.seed_offsets(k + 1, k, S)] == [0, 1]


def test_bucket_table_shapes():
    c = MC.case("tiny_k8_scan")
    assert _bits(len(MC.table("tiny_k8_scan")), 8) == 8
    for n in ("shift0_k8_end", "shift0_k8_scan"):
        c = MC.case(n)
        nv = len(MC.table(n))
        assert c.k == 8 and nv > 262144 and _bits(nv, 8) == 16 == 2 * c.k            # shift 0
    c = MC.case("span_k20_s8")
    nv = len(MC.table("span_k20_s8"))
    assert c.k == 20 > 8 and nv > 524288 and _bits(nv, 20) == 17 > 2 * c.seed_len    # a 16-bit prefix spans two 17-bit buckets
    for n in MC.MODE_CASES:                                                            # the small cases stay below the prefix: bits <= 16
        assert _bits(len(MC.table(n)), MC.case(n).k) in (9, 10)


def test_many_transcripts_case_sits_on_the_grid_fold():
    c = MC.case("many_transcripts_end")
    M = len(c.transcripts)
    assert M == 32771 and c.props["bearing"] == (0, 5, 32767, 32768, M - 1)
    assert [t for t, s in enumerate(c.transcripts) if len(s) >= c.k] == list(c.props["bearing"])
    h, o = MC.expected("many_transcripts_end")
    hs, _ = MC.expected("many_transcripts_scan")
    for hh in (h, hs):
        assert sorted(set(hh["tid"].tolist())) == list(c.props["bearing"])             # every bearing transcript is hit, on both strands
        assert set(zip(hh["tid"].tolist(), hh["fwd"].tolist())) == {(t, f) for t in c.props["bearing"] for f in (0, 1)}


def test_stride_case_has_reads_on_the_second_pass():
    c = MC.case("stride_end")
    assert [len(s) - c.k + 1 for s in c.transcripts] == [1023, 1024, 1025, 2500]
    h, o = MC.expected("stride_end")
    got = set(zip(h["tid"].tolist(), h["pos"].tolist()))
    assert {(1, 1023), (2, 1023), (2, 1024), (3, 1023), (3, 1024), (3, 2499), (0, 1022)} <= got and (0, 1023) not in got
    assert np.array_equal(h, MC.expected("stride_scan")[0])


def test_degenerate_indexes():
    for n in ("all_short_end", "all_short_scan"):
        assert MC.n_positions(MC.case(n)) == 0 and len(MC.expected(n)[0]) == 0
    for n in ("all_N_end", "all_N_scan"):
        assert MC.n_positions(MC.case(n)) == 85 and len(MC.table(n)) == 0 and len(MC.expected(n)[0]) == 0
    c = MC.case("len_k_end")
    assert [len(s) for s in c.transcripts[:2]] == [c.k, c.k - 1] and len(MC.table("len_k_end")) == 1 + 0 + 35 + 1
    assert _recs("len_k_end", 0) == [(0, 1, 0, 0)] and _recs("len_k_end", 1) == [(0, 0, 0, 0)] and _recs("len_k_end", 2) == []
    assert _recs("len_k_end", 6) == [(0, 1, -1, 0)] and _recs("len_k_end", 7) == [(0, 1, 0, 0)]
    c = MC.case("n_one_kmer_end")
    t = MC.table("n_one_kmer_end")
    assert sorted(p for _, tt, p in t[0:len(t)] if tt == 0) == [0, c.k + 1] and len(t) == c.props["n_kmers"]
    c = MC.case("all_bytes_end")
    assert sorted(c.transcripts[0][60:316]) == list(range(256))
    clean = sorted(p for _, tt, p in MC.table("all_bytes_end")[0:10 ** 6] if tt == 0)
    assert clean == list(range(0, 45)) + list(range(316, 316 + 45))                    # only the flanks hold k-mers
    assert not any(tt == 2 and 4 < p < 37 for _, tt, p in MC.table("all_bytes_end")[0:10 ** 6])      # 0xC1, 0x01, 0x21 ... are not bases
    for n in ("all_bytes_end", "all_bytes_scan"):
        assert _recs(n, 5) == [] and _recs(n, 7) == [] and _recs(n, 0) == [(0, 1, 20, 0)]


def test_end_seed_edges():
    for S in (2, 3, 8):
        n = f"end_edges_S{S}"
        p = MC.case(n).props
        for strand, f in (("fwd", 1), ("rc", 0)):
            for where in ("seed0", "seed1", "middle"):
                assert _recs(n, p[f"N_{where}_{strand}"]) == [(0, f, 50, 0)]
        assert _recs(n, p["negative_pos"]) == [(0, 1, -7, 0)] and _recs(n, p["negative_pos_rc"]) == [(0, 0, -7, 0)]
        assert _recs(n, p["overhang"]) == [(0, 1, 184, 0)] and 184 + 25 > 200
        assert _recs(n, p["palindrome"]) == [(1, 0, 30, 0), (1, 1, 30, 0)]
        r = MC.case(n).reads1[p["palindrome"]]
        assert MC.rc(r) == r
        assert _recs(n, p["seeds_disagree"]) == [(2, 1, 0, 0)] and _recs(n, p["seeds_disagree_rc"]) == [(2, 0, 0, 0)]      # seed 1 alone says 4
        c = MC.case(n)
        D = c.reads1[p["shared_offset"]]
        assert len(D) == c.k + max(S, 3) - 2 and len(MO.seed_offsets(len(D), c.k, S)) == (S - 1 if S > 2 else 2)
        assert _recs(n, p["shared_offset"]) == [(3, 1, 12, 0), (4, 1, 10 - (len(D) - c.k), 0)]      # one vote each: both kept
        assert _recs(n, p["shared_offset_rc"]) == [(3, 0, 12, 0), (4, 0, 10 - (len(D) - c.k), 0)]
        idx = MO.build_index(c.transcripts, c.k, c.max_occ)
        U = c.reads1[p["seeds_disagree"]]
        assert MO.map_read(idx, b"A" * 0 + U[-c.k:], c.k, 2) == [(2, 1, 16 + 9)]


def test_maxocc_triple_counts_and_cut_order():
    c = MC.case("maxocc_triple_end")
    words, counts = c.props["words"], c.props["counts"]
    assert c.max_occ == MC.OCC and counts == [MC.OCC - 1, MC.OCC, MC.OCC + 1]
    t = MC.table("maxocc_triple_end")
    occ = []
    for w, n in zip(words, counts):
        key = int("".join(str(b"ACGT".index(x)) for x in w), 4)
        lo, hi = t.prefix_range(key, key + 1)
        assert hi - lo == n
        assert sum(len(MC._find_all(s, w)) + len(MC._find_all(s, MC.rc(w))) for s in c.transcripts) == n
        occ.append([tt for _, tt, _ in t[lo:hi]])
    assert occ[2] == [0, 1, 1, 2, 3] and len(set(occ[0])) < len(occ[0])                # a transcript holds two; the cut drops transcript 3
    for r in (2, 8):
        assert [x[0] for x in _recs("maxocc_triple_end", r)] == [0, 1, 2]              # end seeds: the first max_occ in (t, p) order
        assert _recs("maxocc_triple_scan", r) == []                                    # scan: a miss
    assert [x[0] for x in _recs("maxocc_triple_end", 7)] == [0, 1, 3] == [x[0] for x in _recs("maxocc_triple_scan", 7)]     # exactly max_occ: all kept
    assert [x[0] for x in _recs("maxocc_triple_scan", 6)] == [1, 3]
    assert MC.case("maxocc1_end").max_occ == 1
    assert _recs("maxocc1_end", 0) == [(0, 1, 10, 0)] and _recs("maxocc1_scan", 0) == [] and _recs("maxocc1_scan", 1) == [(1, 1, 37, 0)]


def test_scan_cap_case_has_eight_groups_and_a_ninth_available():
    c = MC.case("scan_cap")
    for key in ("nine", "nine_rc"):
        read = c.reads1[c.props[key]]
        g8, g9, gmore = (MC.scan_groups("scan_cap", read, m) for m in (MO.MAX_GROUPS, 9, 20))
        assert len(g8) == 8 and len(g9) == 9 == len(gmore) and g9[:8] == g8
        assert sorted(g[0] for g in g9) == [0] * 4 + [1] * 5 or sorted(g[0] for g in g9) == [0] * 5 + [1] * 4
        assert min(sum(g[0] for g in g8), 8 - sum(g[0] for g in g8)) == 4              # both strands hold groups: the cap is shared
        assert len({(occ[0][0], g[0]) for g in g9 for occ in [g[3]]}) == 9             # nine different (transcript, strand)
        assert len(_recs("scan_cap", c.props[key])) == 8
        assert len(MO.scan_vote(g9)) == 9                                              # the ninth would have been a ninth record
    assert len(MC.scan_groups("scan_cap", c.reads1[c.props["five"]], 20)) == 5 == len(_recs("scan_cap", c.props["five"]))


def test_scan_edges():
    n = "scan_edges"
    c = MC.case(n)
    p = c.props
    g = MC.scan_groups(n, c.reads1[p["whole_fwd"]])
    assert len(g) == 1 and g[0][:3] == (1, 0, 60)                                      # one lookup, the other strand never walked
    g = MC.scan_groups(n, c.reads1[p["whole_rev_after_fwd_partial"]])
    assert [x[:3] for x in g] == [(1, 0, c.seed_len + 3), (0, 0, 40)]                  # a forward partial group, then the reverse whole-read match
    assert _recs(n, p["whole_rev_after_fwd_partial"]) == [(3, 0, 30, 0), (4, 1, 20, 0)]
    r = c.reads1[p["palindrome"]]
    assert MC.rc(r) == r and _recs(n, p["palindrome"]) == [(2, 1, 25, 0)]              # the forward whole-read match ends both walks
    assert _recs(n, p["tail_only"]) == [] == _recs(n, p["tail_only_rc"]) and c.reads1[p["tail_only"]] in c.transcripts[0]
    assert [x[:3] for x in MC.scan_groups(n, c.reads1[p["stop_read_end"]])] == [(1, 0, 25)]
    assert [x[:3] for x in MC.scan_groups(n, c.reads1[p["stop_transcript_end"]])] == [(1, 0, 30)]
    assert [x[:3] for x in MC.scan_groups(n, c.reads1[p["stop_read_N"]])] == [(1, 0, 25), (1, 26, 14)]
    assert [x[:3] for x in MC.scan_groups(n, c.reads1[p["stop_transcript_N"]])] == [(1, 0, 30), (1, 31, 29)]
    assert [x[:3] for x in MC.scan_groups(n, c.reads1[p["lower_case_run"]])] == [(1, 0, 80)]
    assert [x[:3] for x in MC.scan_groups(n, c.reads1[p["lower_case_read"]])] == [(1, 0, 80)]
    assert MC.scan_groups(n, c.reads1[p["N_every_s_minus_1"]]) == [] and c.reads1[p["N_every_s_minus_1"]].count(b"N") == 9
    assert [x[:3] for x in MC.scan_groups(n, c.reads1[p["one_window_at_the_end"]])] == [(1, 80, 10)]
    assert [x[:3] for x in MC.scan_groups(n, c.reads1[p["one_window_at_the_end_rc"]])] == [(0, 80, 10)]
    assert _recs(n, p["shorter_than_s"]) == [] and _recs(n, p["exactly_s"]) == [(0, 1, 5, 0)]


@pytest.mark.parametrize("n", ["pairs_end", "pairs_scan"])
def test_pairing_cases(n):
    c = MC.case(n)
    p = c.props
    h, o = MC.expected(n)

    def rec(key):
        return [tuple(int(x[f]) for f in ("tid", "fwd", "pos", "mate_fwd", "mate_pos", "frag_len", "read_len", "mate_len", "mate_status"))
                for x in h[o[p[key]]:o[p[key] + 1]]]
    assert rec("cross_product") == [(0, 0, 155, 1, 127, 78, 50, 50, 3), (0, 1, 20, 0, 55, 85, 50, 50, 3)]       # left-major: left (A, 0) first
    left = {x[:2] for x in _recs(n, p["cross_product"], False)}
    assert left == {(0, 0), (0, 1)}                                                    # the left mate alone lies on both strands of A
    assert rec("same_strand") == [(4, 1, 10, 0, 0, 0, 40, 40, 1), (4, 1, 90, 0, 0, 0, 40, 40, 2)]
    assert rec("same_strand_rc") == [(4, 0, 10, 0, 0, 0, 40, 40, 1), (4, 0, 90, 0, 0, 0, 40, 40, 2)]
    assert rec("left_BD_right_BC") == [(1, 1, 30, 0, 130, 140, 40, 40, 3)]
    assert {x[0] for x in _recs(n, p["left_BD_right_BC"], False)} == {1, 3}
    assert rec("mate_inside") == [(4, 1, 20, 0, 35, 60, 60, 30, 3)] and rec("mate_inside_swapped") == [(4, 0, 35, 1, 20, 60, 30, 60, 3)]
    assert rec("negative_and_overhang") == [(4, 1, -9, 0, 125, 170, 34, 36, 3)] and 125 + 36 > 150             # 161 - (-9)
    assert rec("negative_and_overhang_swapped") == [(4, 0, 125, 1, -9, 170, 36, 34, 3)]
    assert rec("left_only") == [(4, 1, 30, 0, 0, 0, 40, 40, 1)] and rec("right_only") == [(4, 0, 30, 0, 0, 0, 40, 40, 2)]
    assert rec("both_unmapped") == []
    assert rec("different_transcripts") == [(4, 1, 30, 0, 0, 0, 40, 30, 1), (2, 0, 90, 0, 0, 0, 30, 40, 2)]
    assert rec("different_lengths") == [(4, 1, 10, 0, 60, 130, 17, 80, 3)]
    assert rec("empty_left") == [(4, 0, 60, 0, 0, 0, 40, 0, 2)] and rec("short_right") == [(4, 1, 60, 0, 0, 0, 40, 4, 1)]


def test_capacity_case_exceeds_the_first_guess():
    for n in ("capacity_end", "capacity_scan"):
        c = MC.case(n)
        h, o = MC.expected(n)
        assert len(h) == 1200 > max(4 * len(c.reads1), 1024) and (np.diff(o) == 40).all()
    for n in ("no_candidate_end", "no_candidate_scan"):
        assert len(MC.expected(n)[0]) == 0 and len(MC.expected_for(n, False)[0]) == 0


@pytest.mark.parametrize("n", ["long_mate_end", "long_mate_scan"])
def test_long_mate_rule(n):
    """65 535 bases: records with the true lengths and fragment; 65 536: no records for the read, whichever mate it is"""
    c = MC.case(n)
    assert [len(r) for r in c.reads1] == [65535, 65536, 50, 50, 65535, 65536] and [len(r) for r in c.reads2] == [50, 50, 65535, 65536, 50, 50]
    h, o = MC.expected(n)
    assert np.diff(o).tolist() == [1, 0, 1, 0, 1, 0] and (h["mate_status"] == 3).all()
    assert h["frag_len"].tolist() == [65950 - 100] * 3 and h["read_len"].tolist() == [65535, 50, 65535] and h["mate_len"].tolist() == [50, 65535, 50]
    h, o = MC.expected_for(n, False)
    assert np.diff(o).tolist() == [1, 0, 1, 1, 1, 0] and h["read_len"].tolist() == [65535, 50, 50, 65535]
    assert MO.pair_records([(0, 1, 5)], None, 65536, 0) == [] and len(MO.pair_records([(0, 1, 5)], None, 65535, 0)) == 1
    assert MO.pair_records([(0, 1, 5)], [], 10, 65536) == [] and len(MO.pair_records([(0, 1, 5)], [], 10, 65535)) == 1
