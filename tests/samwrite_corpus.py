"""Hit batches for the SAM writer tests (tests/test_samwrite_cpu.py, tests/test_gpu_samwrite.py) and what samfile._sam_text -- the
statement both writers are judged by -- says about them.  A case is a dict: names / ref_len (the transcripts), hits (HIT_DTYPE),
offsets (uint32), paired, read_names (list of bytes) and seqs (per read: bytes, or a (mate 1, mate 2) pair).  Every case is used
with and without its read names and with and without its bases (`variants`)."""
import numpy as np

from sailfish_amd.hits import HIT_DTYPE

# transcript names of every length class: empty, short, at and past the writers' short-copy bound (48), long
NAMES = [b"t0", b"", b"ENST00000456328.2|ENSG00000223972.5|-|OTTHUMT00000362751.1", b"x" * 48, b"y" * 49, b"t5", b"z" * 700, b"NM_001"]
REF_LEN = [1000, 5, 2 ** 31 - 1, 70000, 12, 99, 100000, 1]
EDGES = [0, 8, 9, 98, 99, 998, 999, 9998, 9999, 99998, 99999, 999998, 999999, 9999998, 9999999, 99999998, 99999999, 999999998, 999999999,
         2 ** 31 - 2, 2 ** 31 - 1]                        # pos: POS = pos + 1 stands at every decimal width edge
FRAG_EDGES = [0, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000,
              999999999, 1000000000, 2 ** 32 - 1]
LEN_EDGES = [1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 65535]


def rec(tid, pos, mate_pos=0, frag_len=0, read_len=50, mate_len=0, fwd=1, mate_fwd=0, status=0):
    return (tid, pos, mate_pos, frag_len, read_len, mate_len, fwd, mate_fwd, status, 0)


def _case(paired, reads):
    """reads: [(name, seq or (seq1, seq2), [records])]"""
    hits = np.array([r for _, _, recs in reads for r in recs], HIT_DTYPE)
    off = np.concatenate([[0], np.cumsum([len(recs) for _, _, recs in reads])]).astype(np.uint32)
    return dict(names=NAMES, ref_len=REF_LEN, hits=hits, offsets=off, paired=paired, read_names=[q for q, _, _ in reads],
                seqs=[s for _, s, _ in reads])


def _seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), n).tobytes())


def corner(paired, long_seqs=(9000,)):
    """every rule of csrc/samwfmt.h at its edges; long_seqs: the lengths of the long SEQs (one read each)"""
    rng = np.random.default_rng(7)
    sq = (lambda a, b=None: (_seq(rng, a), _seq(rng, a if b is None else b))) if paired else (lambda a, b=None: _seq(rng, a))
    reads = []
    if paired:
        P = lambda tid, pos, mpos, frag=200, fwd=1, mfwd=0, rl=50, ml=60: rec(tid, pos, mpos, frag, rl, ml, fwd, mfwd, 3)
        O = lambda tid, pos, status, fwd=1, rl=50: rec(tid, pos, 0, 0, rl, 0, fwd, 0, status)
        reads += [(b"none", sq(100), []),
                  (b"one", sq(100), [P(0, 10, 150)]),
                  (b"three", sq(100), [P(0, 7, 7, 50), P(2, 300, 100, 250, 0, 1), P(5, 100, 300, 250, 0, 0)]),
                  (b"strands", sq(1), [P(0, 1, 2, 3, f, m) for f in (0, 1) for m in (0, 1)]),
                  (b"orph", sq(0, 100), [O(0, 5, 1), O(3, 6, 1, 0), O(7, 0, 2), O(4, 2, 2, 0)]),
                  (b"left", sq(100, 0), [O(5, 98, 1, 0)]),
                  (b"right", sq(100), [O(6, 99, 2)]),
                  (b"", sq(100), [P(0, 0, -1, 59), P(0, -1, 0, 61)]),
                  (b"clip", sq(50, 60), [P(3, -49, -59, 60, 1, 0), P(3, 0, -59, 109), O(3, -49, 1), O(3, -1, 2, 0)]),
                  (b"Q" * 300, sq(100), [P(6, 20, 40)]),
                  (b"Q" * 48, sq(48), [P(3, 20, 40)]), (b"Q" * 49, sq(49), [P(4, 20, 40)]),
                  (b"name with spaces", sq(100), [])]
        reads += [(b"pos%d" % i, sq(1), [P(2, p, EDGES[-1 - i], FRAG_EDGES[i % len(FRAG_EDGES)])]) for i, p in enumerate(EDGES)]
        reads += [(b"frag%d" % i, sq(1), [P(0, 5, 4, f), P(0, 4, 5, f)]) for i, f in enumerate(FRAG_EDGES)]
        reads += [(b"len%d" % i, sq(1), [P(6, 0, 0, 1, 1, 1, n, LEN_EDGES[-1 - i]), P(6, -(n - 1), -(LEN_EDGES[-1 - i] - 1), 1, 1, 1, n, LEN_EDGES[-1 - i]),
                                            O(6, -(n - 1), 1 + i % 2, 1, n)]) for i, n in enumerate(LEN_EDGES)]
        reads += [(b"long%d" % n, (_seq(rng, n), _seq(rng, 1)), [P(0, 1, 2)]) for n in long_seqs]
        reads += [(b"longnone", (_seq(rng, 3), _seq(rng, long_seqs[0])), [])]
    else:
        S = lambda tid, pos, fwd=1, rl=50: rec(tid, pos, 0, 0, rl, 0, fwd, 0, 0)
        reads += [(b"none", sq(100), []),
                  (b"one", sq(100), [S(0, 10)]),
                  (b"three", sq(100), [S(0, 7, 0), S(2, 300), S(5, 100, 0)]),
                  (b"", sq(0), [S(1, 0), S(1, -1), S(1, -49)]),
                  (b"Q" * 300, sq(1), [S(6, 20)]),
                  (b"Q" * 48, sq(48), [S(3, 20)]), (b"Q" * 49, sq(49), [S(4, 20, 0)]),
                  (b"name with spaces", sq(100), [])]
        reads += [(b"pos%d" % i, sq(1), [S(2, p, i & 1)]) for i, p in enumerate(EDGES)]
        reads += [(b"len%d" % i, sq(1), [S(6, 0, 1, n), S(6, -(n - 1), 0, n)]) for i, n in enumerate(LEN_EDGES)]
        reads += [(b"long%d" % n, _seq(rng, n), [S(0, 1)]) for n in long_seqs]
        reads += [(b"longnone", _seq(rng, long_seqs[0]), [])]
    return _case(paired, reads)


def random_case(seed, paired, n_reads=300, long_seqs=()):
    """n_reads reads with 0 .. 4 records (a few with 40), names and bases of mixed lengths; long_seqs as in corner"""
    rng = np.random.default_rng(1000 + seed)
    reads = []
    for i in range(n_reads):
        k = int(rng.choice([0, 1, 1, 1, 2, 3, 4])) if rng.random() > 0.01 else 40
        n1, n2 = (int(rng.choice([0, 1, 30, 48, 49, 75, 100, 151, 250])) for _ in range(2))
        if i < len(long_seqs):
            n1 = long_seqs[i]
        recs = []
        status = int(rng.choice([1, 2, 3, 3, 3])) if paired else 0
        for _ in range(k):
            rl, ml = int(rng.integers(1, 300)), int(rng.integers(1, 300))
            pos = int(rng.integers(-(rl - 1), 10 ** int(rng.integers(1, 10))))
            mpos = int(rng.integers(-(ml - 1), 10 ** int(rng.integers(1, 10))))
            st = status if status == 3 else (int(rng.choice([1, 2])) if paired else 0)
            recs.append(rec(int(rng.integers(0, len(NAMES))), pos, mpos if st == 3 else 0, int(rng.integers(0, 2000)) if st == 3 else 0, rl,
                            ml if st == 3 else 0, int(rng.integers(0, 2)), int(rng.integers(0, 2)) if st == 3 else 0, st))
        name = b"read.%d/%s" % (i, b"n" * int(rng.choice([0, 0, 0, 5, 60])))
        reads.append((name, (_seq(rng, n1), _seq(rng, n2)) if paired else _seq(rng, n1), recs))
    return _case(paired, reads)


def failing(paired):
    """[(case, read, record, kind)]: batches that cannot be written and the lowest offender (kind 1: no base on the transcript,
    2: tid is no transcript)"""
    st = 3 if paired else 0
    ok = rec(0, 5, 9 if paired else 0, 54 if paired else 0, 50, 50 if paired else 0, 1, 0, st)
    bad_pos = rec(0, -50, 9 if paired else 0, 0, 50, 50 if paired else 0, 1, 0, st)
    bad_tid = rec(len(NAMES), 5, 9 if paired else 0, 54 if paired else 0, 50, 50 if paired else 0, 1, 0, st)
    both = rec(len(NAMES) + 7, -51, 0, 0, 50, 50 if paired else 0, 1, 0, st)
    s = (b"ACGT", b"TTGA") if paired else b"ACGT"
    mk = lambda lists: _case(paired, [(b"q%d" % i, s, recs) for i, recs in enumerate(lists)])
    out = [(mk([[ok], [], [ok, ok, bad_pos, bad_pos], [bad_pos], [bad_tid]]), 2, 2, 1),
           (mk([[ok], [ok, bad_tid], [bad_pos]]), 1, 1, 2),
           (mk([[ok] * 300 + [both, bad_tid]] + [[bad_pos]] * 3), 0, 300, 1),
           (mk([[]] * 400 + [[ok, ok], [bad_tid, bad_pos]]), 401, 0, 2)]
    if paired:
        out.append((mk([[ok], [rec(0, 5, -50, 0, 50, 50, 1, 0, 3)]]), 1, 0, 1))             # the mate has no base on the transcript
        out.append((mk([[ok, rec(0, 5, 0, 0, 50, 0, 1, 0, 1), rec(0, -50, 0, 0, 50, 0, 1, 0, 2)]]), 0, 2, 1))
    return out


def variants(case):
    """the case with and without read names, with and without bases"""
    return [dict(case, read_names=case["read_names"] if q else None, seqs=case["seqs"] if s else None) for q in (True, False) for s in (True, False)]


def expected(case, first_read=0):
    """the alignment lines of _sam_text for the case with case['paired'] in force, default names counted from first_read"""
    from sailfish_amd import samfile
    n = len(case["offsets"]) - 1
    seqs, names = case["seqs"], case["read_names"]
    if seqs is None and case["paired"]:
        seqs = [(b"*", b"*")] * n                         # the same text, and _sam_text takes the batch as paired without a pair record
    if names is None and first_read:
        names = [b"r%d" % (first_read + r) for r in range(n)]
    text = samfile._sam_text(case["names"], case["ref_len"], case["hits"], case["offsets"], names, seqs)
    head = samfile.sam_header(case["names"], case["ref_len"])
    assert text.startswith(head)
    return text[len(head):]


def blob(items, dtype):
    """(uint8 array of the items back to back, offsets of `dtype`)"""
    off = np.zeros(len(items) + 1, dtype)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(items), np.uint8).copy(), off


def arrays(case):
    """the host arrays sfgpu_sam_write_text's arguments are made of: dict(hits, offsets, ref, ref_off, q, q_off, s1, s1_off, s2,
    s2_off); absent names / bases are None"""
    out = dict(hits=np.ascontiguousarray(case["hits"]).view(np.uint8).reshape(-1).copy(), offsets=np.ascontiguousarray(case["offsets"], np.uint32))
    out["ref"], out["ref_off"] = blob(case["names"], np.uint64)
    out["q"], out["q_off"] = blob(case["read_names"], np.uint64) if case["read_names"] is not None else (None, None)
    out["s1"] = out["s1_off"] = out["s2"] = out["s2_off"] = None
    if case["seqs"] is not None:
        out["s1"], out["s1_off"] = blob([s[0] if case["paired"] else s for s in case["seqs"]], np.int64)
        if case["paired"]:
            out["s2"], out["s2_off"] = blob([s[1] for s in case["seqs"]], np.int64)
    return out
