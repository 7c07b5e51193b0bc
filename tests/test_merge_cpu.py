"""The corpus of the class-table exchange tests (tests/merge_corpus.py) holds what it promises, its numpy statement of the four
exchange primitives gives the single-builder table, and the driver's fallback from the disjoint concatenation to the all-gather
fold (DistributedQuant._merge) gives the unforced result.  No GPU: tests/test_gpu_merge.py compares csrc/merge.hip with the same
corpus."""
import numpy as np

import merge_corpus as MC


def _key32(c):
    """the 64-bit sort key of sfgpu_eqvec_merge_disjoint: (first id << 32) | (hash >> 32)"""
    return (c[0][0] << 32) | (c[1] >> 32)


def _union(parts):
    return [c for p in parts for c in MC.classes_of(p)]


def _runs(sorted_keys):
    """[(start, length)] of the runs of equal keys longer than one"""
    out, i = [], 0
    while i < len(sorted_keys):
        j = i
        while j + 1 < len(sorted_keys) and sorted_keys[j + 1] == sorted_keys[i]:
            j += 1
        if j > i:
            out.append((i, j - i + 1))
        i = j + 1
    return out


def test_corpus_covers_its_rules(built):
    # ---- the real tables
    s3 = MC.shards3()
    shards, whole = s3["shards"], s3["whole"]
    from oracle import oracle as O
    for t in shards + [whole]:
        assert np.array_equal(t[3], O.xxh64_lists(t[1], t[0].astype(np.uint64)))                    # the labels' XXH64
        assert MC.classes_of(t) == sorted(MC.classes_of(t), key=MC.canonical_key)
        assert 1 <= np.diff(t[0]).min() and np.diff(t[0]).max() <= 6 and t[1].max() < 50
    held = [{c[0] for c in MC.classes_of(t)} for t in shards]
    times = {lab: sum(lab in h for h in held) for lab in set().union(*held)}
    assert all(sum(1 for v in times.values() if v == k) >= 10 for k in (1, 2, 3))                  # labels in one, two and three shards
    for t, want in zip(shards, MC.BIG_LABEL_COUNTS):
        assert dict((c[0], c[2]) for c in MC.classes_of(t))[MC.BIG_LABEL] == want
        assert 3000 <= int(t[2].sum()) - want + 1 <= 3001
    assert dict((c[0], c[2]) for c in MC.classes_of(whole))[MC.BIG_LABEL] == (1 << 33) + 4
    assert MC.n_ids(whole) > MC.n_classes(whole) > 100

    # ---- the owner cases
    cases = MC.owner_cases()
    assert set(cases) == set(MC.OWNER_CASE_NAMES)
    for n in MC.OWNER_NS:
        sizes = dict((k, MC.owner_expected(f"{k}{n}")[1]) for k in ("last", "mid", "rr"))
        assert all(len(s) == n for s in sizes.values())
        assert [c for c, _ in sizes["last"]] == [0] * (n - 1) + [300]
        if n > 2:
            assert sizes["mid"][0] == sizes["mid"][-1] == (0, 0) and all(c >= 2 for c, _ in sizes["mid"][1:-1])
        else:
            assert MC.n_classes(cases[f"mid{n}"][0]) == 0
        assert max(c for c, _ in sizes["rr"]) - min(c for c, _ in sizes["rr"]) <= 1 and min(c for c, _ in sizes["rr"]) >= 2
        t = cases[f"rr{n}"][0]
        assert np.array_equal(MC.owner_of(t[3], n), np.arange(601) % n)
        assert t[1].max() >= 1 << 31 and t[2].max() >= 1 << 62 and (t[3] >> np.uint64(63)).any() and not (t[3] >> np.uint64(63)).all()
    pairs = cases["pairs3"][0]
    hs = pairs[3].reshape(16, 5)
    assert sorted(int(x) for x in hs[0, 1:] ^ hs[0, 0]) == sorted(MC.PAIR_XORS) and 1 << 63 in MC.PAIR_XORS
    assert all(x == 1 << 63 or x < 1 << 33 for x in MC.PAIR_XORS)
    for n in (3, 7, 256):
        own = MC.owner_of(pairs[3], n).reshape(16, 5)
        assert (own == own[:, :1]).all() and len(set(own[:, 0].tolist())) > 1
    for C in (0, 1, 255, 256, 257):
        t = cases[f"C{C}"][0]
        assert MC.n_classes(t) == C == MC.n_ids(t)
    pad = lambda c, l: MC.block_bytes(c, l) - (12 * c + 4 * l)
    t = cases["pad4_1"][0]
    assert sorted(np.diff(t[0]).tolist()) == [1, 3000] and MC.n_ids(t) % 2 == 1
    assert [pad(*s) for s in MC.owner_expected("pad4_1")[1]] == [4]
    assert MC.owner_expected("pad4_2")[1] == [(1, 3000), (1, 1)] and [pad(*s) for s in MC.owner_expected("pad4_2")[1]] == [4, 0]
    assert [pad(*s) for s in MC.owner_expected("pad0_1")[1]] == [0] and MC.owner_expected("pad0_1")[1][0][0] == 2
    assert sorted(cases["counts"][0][2].tolist()) == [1, 1 << 32, 1 << 62]
    for name in MC.OWNER_CASE_NAMES:                                                                # sizes and bytes agree
        raw, sizes = MC.owner_expected(name)
        t, n = cases[name]
        assert len(raw) == MC.block_offsets(sizes)[-1] and sum(c for c, _ in sizes) == MC.n_classes(t) and sum(l for _, l in sizes) == MC.n_ids(t)
        assert (raw, sizes) == MC.pack_by_owner_vectorised(t, n) and sizes == MC.owner_sizes_vectorised(t, n)      # the reference of `big`
    big = MC.big()
    assert MC.n_classes(big) == 300_000 > 1024 * 256 and MC.n_ids(big) == 300_000
    assert all(c > 40_000 for c, _ in MC.big_expected()[1]) and MC.big_expected()[1] == MC.owner_sizes_vectorised(big, MC.BIG_OWNERS)

    # ---- the merge cases: parts canonical on their own, labels distinct
    mc = MC.merge_cases()
    assert set(mc) == set(MC.MERGE_EQUAL + MC.MERGE_NONE)
    for name, parts in mc.items():
        for p in parts:
            assert MC.classes_of(p) == sorted(MC.classes_of(p), key=MC.canonical_key), name
        labs = [c[0] for c in _union(parts)]
        assert len(labs) == len(set(labs)), name
        assert (MC.merge_expected(name) is None) == (name in MC.MERGE_NONE), name

    def stable(parts):
        """the union in the order a stable sort on the 64-bit key leaves it in"""
        return sorted(_union(parts), key=_key32)

    def full(parts):
        return sorted(_union(parts), key=MC.canonical_key)

    # a: the tied classes share first id and hash >> 32, and the stable key order is not the canonical one
    a = [c for c in _union(mc["a"]) if c[0][0] == 5 and c[1] >> 32 == 0xABCD]
    assert len(a) == 2 and a[0][1] > a[1][1] and a[0][0] in [c[0] for c in MC.classes_of(mc["a"][0])]
    assert stable(mc["a"]) != full(mc["a"])
    # b: one run of five over three parts, scrambled
    kb = [_key32(c) for c in stable(mc["b"])]
    assert [n for _, n in _runs(kb)] == [5] and len(mc["b"]) == 3
    run = [c for c in stable(mc["b"]) if _key32(c) == (8 << 32 | 0x1234)]
    assert [c[1] & 0xFFFFFFFF for c in run] == [10, 50, 20, 30, 40]
    # c: runs at sorted position 0, at 255 .. 257 and at the last two positions
    kc = [_key32(c) for c in stable(mc["c"])]
    assert _runs(kc) == [(0, 2), (255, 3), (len(kc) - 2, 2)]
    assert sum(1 for c in _union(mc["c"]) if c[0][0] < 1000) >= 255
    assert stable(mc["c"])[255:258] != full(mc["c"])[255:258] and stable(mc["c"])[:2] != full(mc["c"])[:2] and stable(mc["c"])[-2:] != full(mc["c"])[-2:]
    # d: two labels, one (first id, hash)
    d = [c for c in _union(mc["d"]) if c[0][0] == 7]
    assert len(d) == 2 and d[0][1] == d[1][1] and d[0][0] != d[1][0] and len(mc["d"]) == 2
    # e: the equal pair is not adjacent in the key-stable order and is adjacent in the full order
    se, fe = stable(mc["e"]), full(mc["e"])
    assert [n for _, n in _runs([_key32(c) for c in se])] == [3]
    assert not any(x[0][0] == y[0][0] and x[1] == y[1] for x, y in zip(se, se[1:]))
    assert sum(1 for x, y in zip(fe, fe[1:]) if x[0][0] == y[0][0] and x[1] == y[1]) == 1
    # f: equal hashes and equal high halves under different first ids: no run
    uf = _union(mc["f"])
    assert _runs(sorted(_key32(c) for c in uf)) == []
    assert any(x[1] == y[1] and x[0][0] != y[0][0] for x in uf for y in uf)
    assert any(x[1] != y[1] and x[1] >> 32 == y[1] >> 32 and x[0][0] != y[0][0] for x in uf for y in uf)
    # g: bit 31 everywhere, next to values without it
    ug = _union(mc["g"])
    for field in (lambda c: c[0][0], lambda c: c[1] >> 32, lambda c: c[1] & 0xFFFFFFFF):
        assert {field(c) >> 31 for c in ug} == {0, 1}
    as_signed = lambda c: tuple(x - (1 << 32) if x >> 31 else x for x in (c[0][0], c[1] >> 32, c[1] & 0xFFFFFFFF))
    assert sorted(ug, key=as_signed) != full(mc["g"]) and stable(mc["g"]) != full(mc["g"])
    # h: the dense draws
    for name, n_keys in (("dense", 12), ("dense_dup", 12)):
        u = _union(mc[name])
        assert len(u) == 5000 and len(mc[name]) == 8 and len({c[0][0] for c in u}) == 4 and len({c[1] >> 32 for c in u}) == 3
        assert len({_key32(c) for c in u}) == n_keys
    lows = [c[1] & 0xFFFFFFFF for c in _union(mc["dense"])]
    assert len(set(lows)) == 5000
    runs = _runs(sorted(_key32(c) for c in _union(mc["dense_many"])))
    assert len(runs) > 1000 and len({n for _, n in runs}) >= 5
    # i: the layouts
    lay = MC.layouts()
    assert set(lay) == set(MC.LAYOUT_NAMES)
    assert [len(lay[k][0]) for k in ("one", "two", "three", "eight", "sixtyfour")] == [1, 2, 3, 8, 64]
    n64 = [MC.n_classes(p) for p in lay["sixtyfour"][0]]
    assert 0 in n64 and sum(n64) == MC.n_classes(whole) and sum(1 for x in n64 if x) > 32
    empty = lambda name: [MC.n_classes(p) == 0 for p in lay[name][0]]
    assert empty("leading") == [True, True, False, False] and empty("interior") == [False, True, True, False]
    assert empty("trailing") == [False, False, True] and empty("all_empty") == [True] * 3 and empty("one_empty") == [True]
    for name in MC.LAYOUT_NAMES:                                                                  # the numpy merge of every layout
        parts, want = lay[name]
        assert MC.same_table(MC.merge_disjoint(*MC.merge_case(parts)), want), name


def test_numpy_chain_on_three_shards_gives_the_single_builder_table(built):
    """pack by owner (w = 3), fold at each owner in rank order, export, merge: rowptr, ids, counts and hashes of one O.EqBuilder"""
    s3 = MC.shards3()
    packed, parts = MC.numpy_chain(s3["shards"], 3)
    assert all(MC.n_classes(p) > 0 for p in parts)
    merged = MC.merge_disjoint(*MC.merge_case(parts))
    assert merged is not None
    for got, want in zip(merged, s3["whole"]):
        assert np.array_equal(got.astype(np.uint64), want.astype(np.uint64))
    assert (1 << 33) + 4 in merged[2].tolist()
    # and through one owner (the all-gather route): every shard whole, folded into one table
    _, (one,) = MC.numpy_chain(s3["shards"], 1)
    assert MC.same_table(one, s3["whole"])


def test_driver_falls_back_to_the_allgather_fold_when_the_concatenation_is_refused(built):
    """DistributedQuant._merge with merge="owner": _concat_disjoint returns None (here on every rank, through an engine whose
    merge_disjoint always refuses), so _merge_allgather(part) folds the owners' partitions -- the three ranks must pass what
    test_two_rank_quant_matches_single_process asserts of the unforced run"""
    from test_distributed_cpu import quant_matches_single_process
    res = quant_matches_single_process("sharded", False, "owner", 3, refuse_concat=True)
    assert [r[13] for r in res] == [1, 1, 1]
