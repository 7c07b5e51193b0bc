"""Tables and blocks for the class-table exchange tests (tests/test_merge_cpu.py, tests/test_gpu_merge.py) and the numpy statement of
the four exchange primitives of csrc/merge.hip -- pack_by_owner, fold_block, export_block, merge_disjoint -- with the library's block
formats (include/sfgpu.h, "the class-table exchange").  tests/test_distributed_cpu.py's CheckerEngine drives its control-flow tests
with the same four functions.

A table is (rowptr int64[C + 1], ids uint32[L], counts uint64[C], hashes uint64[C]).  The calls take the hashes as data (nothing is
hashed again), so the crafted tables carry whatever hashes steer a class down the branch under test; only the real tables
(shards3) carry their labels' XXH64.  Everything is built once per process."""
import functools

import numpy as np

U64 = np.uint64
MASK64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the formats and the four primitives
def block_bytes(c, l):
    """SFGPU_BLOCK_BYTES: [counts u64[c] | lens u32[c] | ids u32[l]] padded to 8 bytes"""
    return (12 * c + 4 * l + 7) & ~7


def gather_bytes(c, l):
    """SFGPU_GATHER_BYTES: [counts u64[c] | hashes u64[c] | lens u32[c] | ids u32[l]]"""
    return 20 * c + 4 * l


def owner_of(h, n):
    """the owner of a class among n: bits 33 .. 62 of its hash, mod n (h: int or uint64 array)"""
    if isinstance(h, np.ndarray):
        return ((h >> U64(33)) & U64(0x3FFFFFFF)) % U64(n)
    return ((int(h) >> 33) & 0x3FFFFFFF) % n


def table(rowptr, ids, counts, hashes):
    return (np.asarray(rowptr, np.int64), np.asarray(ids, np.uint32), np.asarray(counts, np.uint64), np.asarray(hashes, np.uint64))


def empty_table():
    return table(np.zeros(1), np.zeros(0), np.zeros(0), np.zeros(0))


def n_classes(t):
    return len(t[0]) - 1


def n_ids(t):
    return int(t[0][-1])


def table_from_classes(classes):
    """[(label tuple, hash, count)] in the given order"""
    rowptr = np.zeros(len(classes) + 1, np.int64)
    rowptr[1:] = np.cumsum([len(c[0]) for c in classes])
    return table(rowptr, np.array([x for c in classes for x in c[0]], np.uint32), np.array([c[2] for c in classes], np.uint64),
                 np.array([c[1] for c in classes], np.uint64))


def classes_of(t):
    rp, ids, cnt, hs = t
    return [(tuple(ids[rp[c]:rp[c + 1]].tolist()), int(hs[c]), int(cnt[c])) for c in range(len(rp) - 1)]


def canonical_key(c):
    """(first id, hash, length, label): the order of a finished table, unsigned throughout"""
    return (c[0][0], c[1], len(c[0]), c[0])


def same_table(a, b):
    return all(np.array_equal(np.asarray(x).astype(np.uint64), np.asarray(y).astype(np.uint64)) for x, y in zip(a, b))


def pack_by_owner(t, n):
    """-> (the n blocks [counts | lens | ids | pad] back to back, [(classes, ids)] per owner); classes keep their order"""
    rp, ids, cnt, hs = t
    owner = owner_of(hs, n) if len(hs) else np.zeros(0, U64)
    parts, sizes = [], []
    for d in range(n):
        sel = np.flatnonzero(owner == d)
        lens = (rp[sel + 1] - rp[sel]).astype("<u4")
        idl = np.concatenate([ids[rp[c]:rp[c + 1]] for c in sel]).astype("<u4") if len(sel) else np.zeros(0, "<u4")
        blk = cnt[sel].astype("<u8").tobytes() + lens.tobytes() + idl.tobytes()
        parts.append(blk + b"\0" * (block_bytes(len(sel), len(idl)) - len(blk)))
        sizes.append((len(sel), len(idl)))
    return b"".join(parts), sizes


def pack_by_owner_vectorised(t, n):
    """pack_by_owner without a Python loop over the classes (for `big`)"""
    rp, ids, cnt, hs = t
    owner = owner_of(hs, n)
    lens_all = np.diff(rp)
    parts, sizes = [], []
    for d in range(n):
        sel = np.flatnonzero(owner == d)
        lens = lens_all[sel]
        tot = int(lens.sum())
        start = np.zeros(len(sel), np.int64)
        start[1:] = np.cumsum(lens)[:-1]
        src = np.repeat(rp[sel] - start, lens) + np.arange(tot)
        blk = cnt[sel].astype("<u8").tobytes() + lens.astype("<u4").tobytes() + ids[src].astype("<u4").tobytes()
        parts.append(blk + b"\0" * (block_bytes(len(sel), tot) - len(blk)))
        sizes.append((len(sel), tot))
    return b"".join(parts), sizes


def owner_sizes_vectorised(t, n):
    rp, ids, cnt, hs = t
    owner = owner_of(hs, n).astype(np.int64)
    return list(zip(np.bincount(owner, minlength=n).tolist(), np.bincount(owner, weights=np.diff(rp), minlength=n).astype(np.int64).tolist()))


def block_offsets(sizes):
    off = [0]
    for c, l in sizes:
        off.append(off[-1] + block_bytes(c, l))
    return off


def parse_block(b, c, l):
    """one [counts | lens | ids] block -> (counts u64[c], offsets int64[c + 1], ids u32[l])"""
    cnt = np.frombuffer(b[:8 * c], "<u8"); lens = np.frombuffer(b[8 * c:12 * c], "<u4"); ids = np.frombuffer(b[12 * c:12 * c + 4 * l], "<u4")
    off = np.zeros(c + 1, np.int64); off[1:] = np.cumsum(lens)
    return cnt, off, ids


def fold_block(d, b, c, l):
    """upsert the classes of one [counts | lens | ids] block into the dictionary label -> count"""
    if c == 0:
        return
    cnt, off, ids = parse_block(b, c, l)
    for r in range(c):
        lab = tuple(ids[off[r]:off[r + 1]].tolist())
        if lab:
            d[lab] = d.get(lab, 0) + int(cnt[r])


def table_from_dict(d):
    """what finish() makes of label -> count: the canonical order under the labels' XXH64"""
    from oracle import oracle as O
    labs = list(d)
    off = np.zeros(len(labs) + 1, np.uint64); off[1:] = np.cumsum([len(x) for x in labs])
    hs = O.xxh64_lists(np.array([x for lab in labs for x in lab], np.uint32), off) if labs else []
    return table_from_classes(sorted(((lab, int(h), d[lab]) for lab, h in zip(labs, hs)), key=canonical_key))


def export_block(t):
    """the table as one [counts | hashes | lens | ids] block"""
    rp, ids, cnt, hs = t
    return cnt.astype("<u8").tobytes() + hs.astype("<u8").tobytes() + np.diff(rp).astype("<u4").tobytes() + ids.astype("<u4").tobytes()


def parse_export(b, c, l):
    cnt = np.frombuffer(b[:8 * c], "<u8"); hs = np.frombuffer(b[8 * c:16 * c], "<u8"); lens = np.frombuffer(b[16 * c:20 * c], "<u4")
    ids = np.frombuffer(b[20 * c:20 * c + 4 * l], "<u4")
    o = np.zeros(c + 1, np.int64); o[1:] = np.cumsum(lens)
    return [(tuple(ids[o[k]:o[k + 1]].tolist()), int(hs[k]), int(cnt[k])) for k in range(c)]


def merge_disjoint(blocks, sizes):
    """disjoint partitions in export_block format -> the union in canonical order, or None if two labels share first id and hash"""
    rows = []
    for b, (c, l) in zip(blocks, sizes):
        rows += parse_export(b, c, l)
    rows.sort(key=canonical_key)
    if any(a[0][0] == b[0][0] and a[1] == b[1] for a, b in zip(rows, rows[1:])):
        return None
    return table_from_classes(rows)


def merge_case(parts):
    """parts: tables -> (blocks, sizes) as sfgpu_eqvec_merge_disjoint takes them"""
    return [export_block(p) for p in parts], [(n_classes(p), n_ids(p)) for p in parts]


def split_by_owner(t, n):
    """the table cut into n parts by owner; every part keeps the order of the table"""
    cl = classes_of(t)
    return [table_from_classes([c for c in cl if owner_of(c[1], n) == d]) for d in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------------
# real tables: three shards from one label pool, and the table of all their reads
BIG_LABEL_COUNTS = ((1 << 32) - 1, 1 << 32, 5)         # the per-shard counts of the label that all three shards hold
BIG_LABEL = (3, 17, 41)


@functools.lru_cache(maxsize=None)
def shards3():
    """-> dict(shards=[table] * 3, whole=table): M = 50, 150 labels of 1 to 6 ids, every shard draws ~3 000 reads from its own 100
    of them, so labels occur in one, two or three shards.  BIG_LABEL is read once in every shard and its count is then set to
    BIG_LABEL_COUNTS[shard]: the shards are tables of weighted groups, which is what the exchange is handed.  `whole` is one
    O.EqBuilder over all reads, BIG_LABEL's count set to the sum."""
    from oracle import oracle as O
    rng = np.random.default_rng(20240)
    M, P = 50, 150
    pool = set()
    while len(pool) < P:
        lab = tuple(rng.integers(0, M, rng.integers(1, 7)).tolist())
        if lab != BIG_LABEL:
            pool.add(lab)
    pool = sorted(pool)
    whole = O.EqBuilder()

    def set_big(t, value):
        rp, ids, cnt, hs = t
        hit = [c for c in range(len(cnt)) if tuple(ids[rp[c]:rp[c + 1]].tolist()) == BIG_LABEL]
        assert len(hit) == 1
        cnt = cnt.copy(); cnt[hit[0]] = value
        return table(rp, ids, cnt, hs)

    shards = []
    for s in range(3):
        mine = rng.choice(P, 100, replace=False)
        reads = [pool[p] for p in mine[rng.integers(0, 100, 3000)]] + [BIG_LABEL]
        off = np.zeros(len(reads) + 1, np.uint64); off[1:] = np.cumsum([len(r) for r in reads])
        ids = np.array([x for r in reads for x in r], np.uint32)
        b = O.EqBuilder(); b.add_batch(ids, off); whole.add_batch(ids, off)
        shards.append(set_big(table(*b.finish()), BIG_LABEL_COUNTS[s]))
    return dict(shards=shards, whole=set_big(table(*whole.finish()), sum(BIG_LABEL_COUNTS)))


def numpy_chain(shards, w):
    """pack by owner with w owners, fold at each owner in rank order, finish -> the owners' partitions"""
    packed = [pack_by_owner(s, w) for s in shards]
    parts = []
    for o in range(w):
        d = {}
        for buf, sizes in packed:
            start = block_offsets(sizes)[o]
            fold_block(d, buf[start:start + block_bytes(*sizes[o])], *sizes[o])
        parts.append(table_from_dict(d))
    return packed, parts


# ---------------------------------------------------------------------------------------------------------------------------------
# crafted tables for the owner calls
OWNER_NS = (1, 2, 3, 7, 8, 255, 256)


def _hash_for_owner(rng, d, n):
    """a hash that owner_of(., n) sends to d; bit 63 and the low 33 bits are random"""
    k = int(rng.integers(0, ((1 << 30) - 1 - d) // n + 1))
    return (int(rng.integers(0, 2)) << 63) | ((d + n * k) << 33) | int(rng.integers(0, 1 << 33))


def _random_classes(rng, owners, n, max_len=4):
    """one class per entry of `owners`: 1 .. max_len ids of the whole uint32 range, counts of the whole uint64 range"""
    out = []
    for d in owners:
        lab = tuple(rng.integers(0, 1 << 32, rng.integers(1, max_len + 1)).tolist())
        out.append((lab, _hash_for_owner(rng, d, n), int(rng.integers(1, 1 << 63))))
    return table_from_classes(out)


def _single_id_table(rng, C):
    return table(np.arange(C + 1), rng.integers(0, 1 << 32, C), rng.integers(1, 1000, C), rng.integers(0, 1 << 64, C, dtype=np.uint64))


PAIR_XORS = (1 << 63, (1 << 33) - 1, 1, 1 << 32)        # bit 63 alone, and three patterns inside the low 33 bits


@functools.lru_cache(maxsize=None)
def owner_cases():
    """name -> (table, n_owners).  `last`: every class at owner n - 1; `mid`: owners 0 and n - 1 empty and every owner between them
    full (n <= 2 has none between: the table is empty); `rr`: class c at owner c mod n"""
    rng = np.random.default_rng(7)
    cases = {}
    for n in OWNER_NS:
        cases[f"last{n}"] = (_random_classes(rng, [n - 1] * 300, n), n)
        mid = list(range(1, n - 1))
        cases[f"mid{n}"] = (_random_classes(rng, [mid[c % len(mid)] for c in range(600)] if mid else [], n), n)
        cases[f"rr{n}"] = (_random_classes(rng, [c % n for c in range(601)], n), n)
    # hashes that differ only in bit 63 or only in the low 33 bits belong to one owner
    base = [int(x) for x in rng.integers(0, 1 << 64, 16, dtype=np.uint64)]
    pairs = table_from_classes([((i, j), h ^ x, 1 + i) for i, h in enumerate(base) for j, x in enumerate((0,) + PAIR_XORS)])
    for n in (3, 7, 256):
        cases[f"pairs{n}"] = (pairs, n)
    for C in (0, 1, 255, 256, 257):
        cases[f"C{C}"] = (_single_id_table(rng, C), 3)
    # a label of 1 id and one of 3 000: 3 001 ids in all.  One owner: 12 * 2 + 4 * 3001 leaves 4 bytes of padding.  Two owners: the
    # long label's block (owner 0, 4 bytes of padding) is followed by the short label's (owner 1, none)
    long_lab = tuple(rng.integers(0, 1 << 32, 3000).tolist())
    for n in (1, 2):
        cases[f"pad4_{n}"] = (table_from_classes([(long_lab, _hash_for_owner(rng, 0, n), 3), ((9,), _hash_for_owner(rng, n - 1, n), 4)]), n)
    cases["pad0_1"] = (table_from_classes([((1, 2, 3), 99 << 33, 3), ((9,), 5 << 33, 4)]), 1)
    cases["counts"] = (table_from_classes([((1,), _hash_for_owner(rng, 1, 2), 1), ((2, 3), _hash_for_owner(rng, 0, 2), 1 << 32),
                                           ((4,), _hash_for_owner(rng, 1, 2), 1 << 62)]), 2)
    return cases


OWNER_CASE_NAMES = tuple([f"{k}{n}" for n in OWNER_NS for k in ("last", "mid", "rr")] + ["pairs3", "pairs7", "pairs256"] +
                         [f"C{C}" for C in (0, 1, 255, 256, 257)] + ["pad4_1", "pad4_2", "pad0_1", "counts"])
BIG_OWNERS = 7


@functools.lru_cache(maxsize=None)
def big():
    """300 000 single-id classes with random hashes: more than 1024 blocks of 256, where the size kernel strides its grid"""
    return _single_id_table(np.random.default_rng(8), 300_000)


@functools.lru_cache(maxsize=None)
def owner_expected(name):
    t, n = owner_cases()[name]
    return pack_by_owner(t, n)


@functools.lru_cache(maxsize=None)
def big_expected():
    return pack_by_owner_vectorised(big(), BIG_OWNERS)


# ---------------------------------------------------------------------------------------------------------------------------------
# crafted parts for merge_disjoint: export-block format, distinct labels, every part in canonical order on its own
def H(hi, lo):
    return ((hi & 0xFFFFFFFF) << 32) | (lo & 0xFFFFFFFF)


def _parts(assigned, n_parts):
    """[(part, class)] -> the parts, each sorted into canonical order"""
    return [table_from_classes(sorted((c for p, c in assigned if p == q), key=canonical_key)) for q in range(n_parts)]


def _dense(rng, n, n_parts, firsts, highs, low_space, unique_lows):
    if unique_lows:
        lows = rng.choice(low_space, n, replace=False)
    else:
        lows = rng.integers(0, low_space, n)
    assigned = []
    for k in range(n):
        first = int(firsts[rng.integers(0, len(firsts))]); hi = int(highs[rng.integers(0, len(highs))])
        assigned.append((int(rng.integers(0, n_parts)), ((first, k), H(hi, int(lows[k])), 1 + k)))      # (first, k): labels are distinct
    return _parts(assigned, n_parts)


@functools.lru_cache(maxsize=None)
def merge_cases():
    """name -> parts (tables).  The expected result is merge_disjoint(*merge_case(parts)): a table, or None for d, e and dense_dup"""
    rng = np.random.default_rng(9)
    cases = {}
    fill = lambda first, k=0: ((first, 77 + k), int(rng.integers(0, 1 << 64, dtype=np.uint64)), 10 + k)
    # a: one key, two low halves, the larger one in part 0 -- the key sort is stable, so it comes out first
    cases["a"] = _parts([(0, ((5, 1), H(0xABCD, 0x90000000), 1)), (1, ((5, 2), H(0xABCD, 0x10), 2)), (0, fill(4)), (1, fill(4, 1)), (0, fill(6)),
                         (1, fill(5, 2))], 2)
    # b: a run of five with scrambled low halves over three parts (union order of the lows: 10 50 20 30 40)
    cases["b"] = _parts([(p, ((8, lo), H(0x1234, lo), lo)) for p, lo in ((0, 50), (1, 20), (2, 40), (0, 10), (1, 30))] +
                        [(2, fill(8, 1)), (0, fill(7)), (1, fill(9))], 3)
    # c: runs at union position 0, at sorted positions 255 .. 257 (253 classes of smaller first id and the first run in front of it:
    # the head of the run is the last thread of block 0, its tail is in block 1) and at the last two positions
    c = [(1, ((0, 1), H(0, 7), 1)), (2, ((0, 2), H(0, 3), 2))]
    c += [(k % 3, fill(k)) for k in range(1, 254)]
    c += [(0, ((1000, 1), H(5, 30), 3)), (1, ((1000, 2), H(5, 10), 4)), (2, ((1000, 3), H(5, 20), 5))]
    c += [(k % 3, fill(2000 + k)) for k in range(40)]
    c += [(0, ((0xFFFFFFF0, 1), H(0xFFFFFFFF, 0xFFFFFFFF), 6)), (2, ((0xFFFFFFF0, 2), H(0xFFFFFFFF, 0xFFFFFFFE), 7))]
    cases["c"] = _parts(c, 3)
    # d: two labels, one first id, one full hash
    cases["d"] = _parts([(0, ((7, 1), H(0x55, 0x66), 1)), (1, ((7, 2), H(0x55, 0x66), 2)), (0, fill(6)), (1, fill(8))], 2)
    # e: one key in three parts, full hashes h1 h2 h1: the equal pair meets only once the run is in full-hash order
    h1, h2 = H(0x77, 0x500), H(0x77, 0x900)
    cases["e"] = _parts([(0, ((7, 1), h1, 1)), (1, ((7, 2), h2, 2)), (2, ((7, 3), h1, 3)), (0, fill(6)), (2, fill(8))], 3)
    # f: one full hash, and one high half, under different first ids: no ties
    cases["f"] = _parts([(0, ((3, 1), H(0x99, 0x11), 1)), (1, ((4, 1), H(0x99, 0x11), 2)), (1, ((3, 2), H(0x42, 0x5), 3)), (0, ((4, 2), H(0x42, 0x1), 4)),
                         (0, ((5, 1), H(0x42, 0x9), 5))], 2)
    # g: bit 31 of the first id, of the high half (bit 63 of the hash) and of the low half: the order is unsigned
    g, k = [], 0
    for first in (0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 1):
        for hi in (0x80000000, 0x7FFFFFFF):
            for lo in (0xFFFFFFFF, 0, 0x80000000, 0x7FFFFFFF):
                g.append((k % 3, ((first, k), H(hi, lo), 1 + k))); k += 1
    cases["g"] = _parts(g, 3)
    # h: 5 000 classes over 8 parts, first ids from 4 values, high halves from 3: twelve long runs; dense_many draws from 40 and 50
    # values: some two thousand runs of one to a dozen classes.  dense_dup draws the low halves from 64 values: full duplicates
    cases["dense"] = _dense(rng, 5000, 8, (2, 9, 0x80000001, 0xFFFFFFFE), (0, 0x7FFFFFFF, 0xFFFFFFFF), 1 << 32, True)
    cases["dense_many"] = _dense(rng, 5000, 8, rng.choice(1 << 32, 40, replace=False), rng.choice(1 << 32, 50, replace=False), 1 << 32, True)
    cases["dense_dup"] = _dense(rng, 5000, 8, (2, 9, 0x80000001, 0xFFFFFFFE), (0, 0x7FFFFFFF, 0xFFFFFFFF), 64, False)
    return cases


MERGE_EQUAL = ("a", "b", "c", "f", "g", "dense", "dense_many")
MERGE_NONE = ("d", "e", "dense_dup")


@functools.lru_cache(maxsize=None)
def merge_expected(name):
    return merge_disjoint(*merge_case(merge_cases()[name]))


LAYOUT_NAMES = ("one", "two", "three", "eight", "sixtyfour", "leading", "interior", "trailing", "one_empty", "all_empty")


@functools.lru_cache(maxsize=None)
def layouts():
    """name -> (parts, expected table): the real table of shards3 cut by owner, with empty parts put around the cuts"""
    whole = shards3()["whole"]
    E = empty_table()
    two = split_by_owner(whole, 2)
    out = {"one": ([whole], whole)}
    for name, n in (("two", 2), ("three", 3), ("eight", 8), ("sixtyfour", 64)):
        out[name] = (split_by_owner(whole, n), whole)
    out["leading"] = ([E, E] + two, whole)
    out["interior"] = ([two[0], E, E, two[1]], whole)
    out["trailing"] = (two + [E], whole)
    out["one_empty"] = ([E], E)
    out["all_empty"] = ([E, E, E], E)
    return out
