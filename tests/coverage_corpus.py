"""The shared corpus of the coverage tests (tests/test_coverage_cpu.py, tests/test_gpu_coverage.py): fourteen transcripts and some
87 000 records, every group built for one edge of csrc/coverfmt.h's rule, with the statement's result computed once.

  0  1 base     one record: the first row of the file; the tests vary ITS name's length, which moves every later row byte by byte
  1  0 bases    neighbours in the array: no slot of its own but the end slot
  2  2 bases
  3  50 bases   an interval that ends exactly at len_t ...
  4  60 bases   ... while this one has an interval that starts at 0
  5  100 bases  pos < 0, a line over the right end, lines wholly off either end, read_len 0
  6  40 bases   p of 0, 1, 2^-32 (q = 1) and 2^-33 (q = 0), 0.3 (truncated, not rounded)
  7  64 bases   a staircase: every base starts a run
  8  30 bases   10 000 records on one identical interval
  9  200 bases  a pair whose mates overlap
 10  120 bases  the records whose alignment slots carry a D in the middle, a leading S, an I, an M that runs past len_t, no operations
 11  65 535 bases   70 000 records of 65 535 bases at p = 1: S exceeds 2^64
 12  300 000 bases  3 000 reads of 100 bases: the scan and the run compaction cross their block boundaries, runs straddle them
 13  10 bases   a name above 4 KB
"""
import functools
import struct

import numpy as np

HIT_DTYPE = np.dtype([("tid", "<u4"), ("pos", "<i4"), ("mate_pos", "<i4"), ("frag_len", "<u4"), ("read_len", "<u2"),
                      ("mate_len", "<u2"), ("fwd", "u1"), ("mate_fwd", "u1"), ("mate_status", "u1"), ("pad_", "u1")])
REF_LEN = np.array([1, 0, 2, 50, 60, 100, 40, 64, 30, 200, 120, 65535, 300000, 10], np.uint32)
M = len(REF_LEN)
NAMES = [b"", b"empty", b"two", b"n" * 49, b"t4", b"clip", b"weights", b"stairs", b"pile", b"pair", b"aligned", b"deep", b"long", b"N" * 5000]
M_OP, I_OP, D_OP, N_OP, S_OP, H_OP, P_OP, EQ_OP, X_OP = range(9)


def word(n, op):
    return n << 4 | op


def _records():
    """-> list of (tid, pos, read_len, p, mate or None, ops or None, aln_pos): ops None = the alignment is <read_len>M at pos"""
    rng = np.random.default_rng(11)
    out = []
    add = lambda tid, pos, n, p=1.0, mate=None, ops=None, apos=None: out.append((tid, pos, n, p, mate, ops, pos if apos is None else apos))      # noqa: E731
    add(0, 0, 1, 0.75)
    add(2, 0, 2, 0.5)
    add(2, 1, 5, 0.25)
    add(3, 40, 10, 0.3)                                    # ends exactly at 50
    add(4, 0, 7, 0.3)                                      # starts at 0 of the next transcript
    add(5, -5, 20); add(5, 90, 30); add(5, -30, 30); add(5, -31, 20); add(5, 100, 10); add(5, 250, 40); add(5, 50, 0); add(5, -3, 200, 0.125)
    for p in (0.0, 1.0, 2.0 ** -32, 2.0 ** -33, 0.3, 1.0 - 2.0 ** -53):
        add(6, 5, 20, p)
    for i in range(64):
        add(7, i, 64 - i, 0.3)                             # base i is covered by i + 1 records
    for _ in range(10000):
        add(8, 3, 17, 0.3)
    add(9, 20, 100, 0.6, mate=(80, 100))                   # mates overlap on [80, 120)
    add(9, 150, 100, 0.4, mate=(-20, 60))
    add(10, 10, 30, 0.5, ops=[word(10, M_OP), word(5, D_OP), word(20, EQ_OP)])
    add(10, 40, 30, 0.5, ops=[word(4, S_OP), word(26, M_OP)], apos=44)
    add(10, 60, 30, 0.25, ops=[word(10, M_OP), word(3, I_OP), word(17, X_OP)])
    add(10, 100, 50, 0.25, ops=[word(50, M_OP)])           # runs past 120
    add(10, 5, 30, 0.7, ops=[])                            # no operations: no interval with alignments, the diagonal without
    add(10, 0, 40, 0.5, ops=[word(2, H_OP), word(5, M_OP), word(10, N_OP), word(1, P_OP), word(5, M_OP), word(0, M_OP), word(300, D_OP), word(8, M_OP)])
    add(10, 30, 20, 0.5, mate=(70, 20), ops=[word(20, M_OP)])
    for _ in range(70000):
        add(11, 0, 65535, 1.0)
    for x in rng.integers(-50, 300000 - 40, 3000).tolist():
        add(12, x, 100, float(rng.integers(1, 1 << 20)) / (1 << 20))
    base12 = int(REF_LEN[:12].astype(np.int64).sum()) + 12  # transcript 12's first slot
    for k, d in ((40, -1), (42, 0), (44, 1), (46, -8), (48, 8)):      # runs that begin and end on and beside multiples of 2048 slots
        add(12, 2048 * k - base12 + d, 2048, 0.5)
    add(13, 2, 5, 0.5)
    return out


@functools.lru_cache(maxsize=None)
def batch():
    """-> (hits HIT_DTYPE[n], offsets uint32[R + 1], p float64[n], (aln_pos int32[2 n], aln_op_off uint64[2 n + 1], aln_ops uint32[])).
    The reads hold 1, 2, 3, 1, 4, ... of the small groups' records in turn (uniform weights then differ from read to read); every
    record of transcripts 8 and 11 is a read of its own."""
    recs = _records()
    n = len(recs)
    hits = np.zeros(n, HIT_DTYPE)
    p = np.zeros(n)
    a_pos, a_cnt, a_ops = np.zeros(2 * n, np.int32), np.zeros(2 * n + 1, np.uint64), []
    for i, (tid, pos, ln, pv, mate, ops, apos) in enumerate(recs):
        hits[i]["tid"], hits[i]["pos"], hits[i]["read_len"], hits[i]["fwd"] = tid, pos, ln, 1
        p[i] = pv
        if mate is not None:
            hits[i]["mate_status"], hits[i]["mate_pos"], hits[i]["mate_len"] = 3, mate[0], mate[1]
        else:
            hits[i]["mate_status"] = i % 3                 # 0, 1, 2: one line each
            hits[i]["mate_pos"], hits[i]["mate_len"] = 7, 9      # (never read)
        w0 = [word(ln, M_OP)] if ops is None else ops
        a_pos[2 * i] = apos
        a_cnt[2 * i + 1] = len(w0)
        a_ops.extend(w0)
        if mate is not None:
            a_pos[2 * i + 1] = mate[0]
            a_cnt[2 * i + 2] = 1
            a_ops.append(word(mate[1], M_OP))
    sizes, i, k = [], 0, 0
    cycle = (1, 2, 3, 1, 4, 0, 1, 5)
    while i < n:
        s = 1 if hits[i]["tid"] in (8, 11) else cycle[k % len(cycle)]
        s = min(s, n - i)
        k += 1
        sizes.append(s)
        i += s
    off = np.zeros(len(sizes) + 1, np.uint32)
    off[1:] = np.cumsum(sizes)
    for a in (hits, off, p, a_pos):
        a.setflags(write=False)
    return hits, off, p, (a_pos, np.cumsum(a_cnt, dtype=np.uint64), np.array(a_ops, np.uint32))


def slices(k):
    """the batch cut into k batches at read boundaries -> list of (hits, offsets, p, alignments)"""
    hits, off, p, (a_pos, a_off, a_ops) = batch()
    R = len(off) - 1
    cuts = [R * j // k for j in range(k + 1)]
    out = []
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        h0, h1 = int(off[r0]), int(off[r1])
        w0, w1 = int(a_off[2 * h0]), int(a_off[2 * h1])
        out.append((hits[h0:h1], off[r0:r1 + 1] - off[r0], p[h0:h1], (a_pos[2 * h0:2 * h1], a_off[2 * h0:2 * h1 + 1] - a_off[2 * h0], a_ops[w0:w1])))
    return out


MODES = ("posterior", "uniform", "aligned")


def mode_batches(mode, k=1):
    """the corpus as coverage_host's batches: "posterior" (p, the diagonal), "uniform" (no p), "aligned" (p and the alignment slots)"""
    return [(h, o, None if mode == "uniform" else p, a if mode == "aligned" else None) for h, o, p, a in slices(k)]


@functools.lru_cache(maxsize=None)
def expected(mode):
    """hits.coverage_host over the corpus -> (runs, summary, stats); computed once, never changed"""
    from sailfish_amd import hits as H
    runs, summary, stats = H.coverage_host(REF_LEN, mode_batches(mode))
    for a in runs + summary:
        a.setflags(write=False)
    return runs, summary, stats


def names(first=None):
    return [NAMES[0] if first is None else first] + NAMES[1:]


def blob(mode):
    """the corpus and its expected result as the stand-alone harness reads it: a header of 8 words, then every array in a block of
    exactly its size"""
    from sailfish_amd import coverage as cov
    (h, o, p, (a_pos, a_off, a_ops)), = slices(1)
    (tid, start, end, total), summary, st = expected(mode)
    text = cov.coverage_text_host(names(), (tid, start, end, total))
    nm = b"".join(names())
    nm_off = np.zeros(M + 1, np.uint64)
    nm_off[1:] = np.cumsum([len(x) for x in names()])
    flags = (1 if mode != "uniform" else 0) | (2 if mode == "aligned" else 0)
    head = struct.pack("<8Q", M, len(o) - 1, len(h), len(a_ops), len(tid), len(text), flags, len(nm))
    stats = np.array([st[k] for k in ("reads", "records", "lines", "intervals", "empty_intervals", "bases_added", "runs", "bases_covered", "residue")], np.uint64)
    parts = [REF_LEN, h, o, p, a_pos, a_off, a_ops, tid, start, end, total, np.concatenate(summary), stats, nm_off]
    return head + b"".join(np.ascontiguousarray(x).tobytes() for x in parts) + nm + text
